"""The SEA search's survivor threshold and the integer shell around it (smallest-bound pick,
survivor lists, survivor passes, key reduction) against the C oracle, bit for bit, on content
whose right answer sits exactly on the threshold 16 LBq - K_b <= U (seaslackcases.py, DESIGN.md
section 4): 256 x 96, 3-frame P-runs on the 128 x 32 and the 128 x 48 tile
(SO_OPT_RUN_TALL_TILES 0 / 1) and the same frames through so_me_full_search.

* r8 / r0 / r15: every 4x4 cell sum of the designed blocks has remainder 8 (K_b = 128, the smallest
  slack), 0 or 15 (K_b = 240, the slack the kernels use for every block); the winner M and a
  candidate T tying with it at a larger |dx| + |dy| have LBq = 16 and SAD = 256 - K_b, and the
  smallest-bound candidate C0 (LBq 0) the same SAD at the largest |dx| + |dy|.  Three layouts put
  designed blocks inside the frame, in the first block row and first / last column, and in the
  last block row (the masked-row path of the smallest-bound pick).
* corners: a texture rolled by (+-16, +-16) per frame: the winners at the window's corners.
* noise: independent noise frames: every candidate passes the bound, so the blocks of the first
  frame leave through the dense fallback (counted) and the later frames' tiles search dense.

The CPU tests (no gpu mark) check that the oracle alone tells these inputs apart: M wins, T and
C0 tie with it in the oracle's own scan, M and T sit on the threshold and fall off a slack one
smaller, and C0 alone has the smallest bound."""
import numpy as np
import pytest

import seaslackcases as C

W, H, NB = C.W, C.H, C.NBX * C.NBY
KEYS = ("split", "mv", "qtc", "tokens", "mae_num", "recon")
QP = 4
CLASSES = (8, 0, 15)


def _threshold_runs(r):
    """Three runs, one per layout first: the designed pair, then the other layouts' current
    frames over the reconstruction."""
    names = list(C.LAYOUTS)
    pairs = {n: C.threshold_pair(r, n, 100 * r + 7 * i + 1) for i, n in enumerate(names)}
    runs = []
    for i, n in enumerate(names):
        cur, ref = pairs[n]
        runs.append(([cur, pairs[names[(i + 1) % 3]][0], pairs[names[(i + 2) % 3]][0]], ref))
    return runs


def _corner_runs():
    f = C.corner_frames()
    return [([f[1], f[2], f[3]], f[0]), ([f[4], f[3], f[2]], f[3])]


def _noise_runs():
    f = C.noise_frames()
    return [([f[1], f[2], f[3]], f[0])]


CASES = {"r8": lambda: _threshold_runs(8), "r0": lambda: _threshold_runs(0), "r15": lambda: _threshold_runs(15),
         "corners": _corner_runs, "noise": _noise_runs}
_EXPECTED = {}


def _expected(name):
    """The case's runs, the oracle's frames of each, and the oracle's block records of every
    (cur, ref) pair a run's frames see: computed once per case."""
    if name not in _EXPECTED:
        from oracle import oracle as O
        runs = CASES[name]()
        frames, pairs = [], []
        for curs, ref0 in runs:
            ref, fr = ref0, []
            for cur in curs:
                e = O.inter_frame(cur, [ref], 16, 16, QP, None, False, 0.015)
                fr.append(e)
                best = np.concatenate([e["mv"][:, 0, :].astype(np.int64), e["mae_num"].reshape(-1, 1)], axis=1)
                pairs.append((cur, ref, best))
                ref = np.ascontiguousarray(e["recon"], dtype=np.uint8)
            frames.append(fr)
        _EXPECTED[name] = (runs, frames, pairs)
    return _EXPECTED[name]


# ---------------------------------------------------------------- CPU: the oracle tells them apart
@pytest.mark.parametrize("layout", list(C.LAYOUTS))
@pytest.mark.parametrize("r", CLASSES)
def test_threshold_blocks_are_on_the_threshold(r, layout):
    from oracle import oracle as O
    cur, ref = C.threshold_pair(r, layout, 100 * r + 1)
    blocks = C.designed_blocks(layout)
    assert len(blocks) >= 9
    three = 0
    for bx, by in blocks:
        p = C.roles(bx, by)
        m, c0 = p[0], p[-1]
        ok, sad, lbq = C.block_candidates(cur, ref, bx, by)
        at = lambda d: (d[0] + 16, d[1] + 16)   # noqa: E731
        target, kb = C.SAD_TARGET[r], C.K_B[r]
        assert C.block_slack(cur, bx, by) == kb
        # the oracle's own scan: M wins at the target SAD, and it is a tie
        assert O.me_block(cur, [ref], bx * 16, by * 16, 16, 16) == (m[0], m[1], 0, target), (bx, by)
        assert int(sad[ok].min()) == target
        ties = {(int(a) - 16, int(b) - 16) for a, b in np.argwhere(ok & (sad == target))}
        assert ties == set(p[:2]) | {c0}, (bx, by, ties)
        assert len(ties) >= 2
        three += len(ties) == 3
        # C0 alone has the smallest bound, so U is the target whichever candidate supplies it
        assert int(lbq[at(c0)]) == 0 and int((ok & (lbq == 0)).sum()) == 1
        # M (and T) sit on the threshold of slack K_b and fall off a slack one smaller
        for d in set(p[:2]) - {c0}:
            assert int(lbq[at(d)]) == 16
            assert 16 * int(lbq[at(d)]) - kb == target
            assert int(lbq[at(d)]) <= (target + kb) >> 4
            assert int(lbq[at(d)]) > (target + kb - 1) >> 4
    assert three >= 4   # blocks with M, T and C0 all three


def test_layouts_cover_the_frame_edges():
    b = {n: C.designed_blocks(n) for n in C.LAYOUTS}
    assert any(by == 0 for _, by in b["first"]) and any(bx == 0 for bx, _ in b["first"])
    assert any(bx == C.NBX - 1 for bx, _ in b["first"])
    assert any(by == C.NBY - 1 for _, by in b["last"])
    assert all(0 < bx < C.NBX - 1 and 0 < by < C.NBY - 1 for bx, by in b["inner"])


def test_corner_frames_win_at_the_corners():
    from oracle import oracle as O
    f = C.corner_frames()
    for k, (dy, dx) in enumerate(C.CORNER_SHIFTS):
        # frame k + 1 is frame k rolled by (dy, dx): block content came from (-dx, -dy)
        assert O.me_block(f[k + 1], [f[k]], 7 * 16, 2 * 16, 16, 16) == (-dx, -dy, 0, 0)


def test_noise_blocks_pass_the_cap():
    f = C.noise_frames()
    for bx, by in ((1, 1), (7, 2), (14, 4)):   # (a corner block has 289 candidates: it cannot pass it)
        ok, sad, lbq = C.block_candidates(f[1], f[0], bx, by)
        k = np.argmin(np.where(ok, lbq, 1 << 30))
        u = int(sad.reshape(-1)[k])
        assert int((ok & (lbq <= (u + 128) >> 4)).sum()) > 384   # even at the smallest slack


# ---------------------------------------------------------------- GPU
def _plane(a, dev):
    import torch
    from streamoptima_amd.engine import alloc_planes
    p = alloc_planes(1, H, W, dev)[0]
    p.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)))
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("tall", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_p_runs_match_oracle(gpu, name, tall):
    import torch
    from streamoptima_amd import _lib
    from streamoptima_amd.engine import Engine
    runs, exp, _ = _expected(name)
    eng = Engine(H, W, 16, 16, False, 0.015, gpu)
    dev_runs = [([_plane(c, gpu) for c in curs], _plane(ref0, gpu), [eng.new_symbols(1) for _ in curs])
                for curs, ref0 in runs]
    with _lib.option(_lib.OPT_RUN_TALL_TILES, tall):
        eng.take_fallback_count()
        eng.encode_p_runs(dev_runs, QP, None)
        torch.cuda.synchronize()
        eng.check_run()
    dense = eng.take_fallback_count()
    print(f"{name} tall {tall}: dense-fallback blocks {dense}")
    for r, (_, _, outs) in enumerate(dev_runs):
        for i, o in enumerate(outs):
            for k in KEYS:
                got, want = getattr(o, k).cpu().numpy(), np.asarray(exp[r][i][k])
                assert got.shape == want.shape, (r, i, k, got.shape, want.shape)
                neq = got.astype(np.int64) != want.astype(np.int64)
                assert not neq.any(), (f"run {r} frame {i} {k}: {int(neq.sum())} values differ from the oracle, "
                                       f"first at {np.flatnonzero(neq.reshape(-1))[:3].tolist()}")
    if name == "noise":
        assert dense >= NB - 4   # the first frame's blocks, one by one (a corner block's 289 or 256 candidates fit the list)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_full_search_matches_oracle(gpu, name):
    import torch
    from streamoptima_amd import _lib
    lib = _lib.load()
    _, _, pairs = _expected(name)
    for n, (cur, ref, want) in enumerate(pairs):
        c, rf = _plane(cur, gpu), _plane(ref, gpu)
        best = torch.empty((NB, 4), dtype=torch.int32, device=gpu)
        rc = lib.so_me_full_search(c.data_ptr(), _lib.ref_array([rf]), 1, H, W, 16, 16, best.data_ptr(), None,
                                   _lib.stream_handle())
        _lib.check(rc, "so_me_full_search")
        torch.cuda.synchronize()
        got = best.cpu().numpy().astype(np.int64)
        neq = (got != want).any(axis=1)
        assert not neq.any(), (f"pair {n}: {int(neq.sum())} blocks differ from the oracle, first "
                               f"{np.flatnonzero(neq)[:3].tolist()}: {got[neq][:3].tolist()} != {want[neq][:3].tolist()}")
