"""The one-GPU plain run on 128 x 48 tiles (SO_OPT_RUN_TALL_TILES; p_run_kernel on
Sea2GeoT<8, 128, 3, true>: 24 blocks per tile, six transform waves, the dword transform scratch
of xform2d_rows_dw) against the C oracle and against the 32-row twin (p_run_short_kernel), on
small frames: an I-frame and three P-frames each.

Shapes (W x H): tile rows of 3 + 1 block rows (64), 3 + 2 (80), two full ones (96), 3 + 3 + 1
(112).  The persistent run covers W % 128 == 0 only, so the 144- and 272-wide frames (a
one-block tile column) are encoded by the per-frame kernels under either option value; 384 x 64
and 256 x 112 carry their tile-row structure through the run itself.
"""
import numpy as np
import pytest
import torch

from streamoptima_amd import _lib

pytestmark = pytest.mark.gpu

QP, FRAMES = 4, 4
KEYS = ("split", "mv", "qtc", "tokens", "recon")
CASES = [(144, 64, "bench", False), (256, 80, "bench", False), (128, 96, "bench", False),
         (272, 112, "bench", False), (384, 64, "bench", False), (256, 112, "bench", False),
         (144, 64, "noise", False), (272, 112, "noise", False), (384, 64, "noise", False),
         (256, 112, "noise", False), (256, 80, "lowtex", True)]
_ORACLE = {}


def _oracle(w, h, content):
    """The oracle's GOP for a shape and content, computed once and shared."""
    key = (w, h, content)
    if key not in _ORACLE:
        from oracle.gop import encode_gop
        from streamoptima_amd.synth import synth_sequence
        seq = synth_sequence(FRAMES, h, w, seed=31, content=content)
        exp = encode_gop(seq, QP, FRAMES)
        for i, r in enumerate(exp):
            d = seq[i].astype(np.int64) - r["recon"].astype(np.int64)
            r["sse_total"] = int((d * d).sum())
        _ORACLE[key] = (seq, exp)
    return _ORACLE[key]


def _encode(gpu, seq, w, h, tall, zero_skip):
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.engine import alloc_planes
    codec = Y_Video_codec(h, w, FRAMES, 16, 16, QP, FRAMES, 0, 0.015, False, device=gpu)
    eng = codec.engine()
    fr = alloc_planes(FRAMES, h, w, gpu)
    fr.copy_(torch.from_numpy(seq))
    with _lib.option(_lib.OPT_RUN_TALL_TILES, tall):
        eng.zero_skip = zero_skip
        res = codec.encode_device(fr, FRAMES, check=False)
        torch.cuda.synchronize()
        eng.check_run()
    host = []
    for s in res["symbols"]:
        d = {k: getattr(s, k).cpu().numpy() for k in KEYS + ("mae_num",)}
        d["frame_type"] = s.frame_type
        host.append(d)
    return host, [int(v) for v in res["sse"].cpu().numpy()]


@pytest.mark.parametrize("w,h,content,zero_skip", CASES)
def test_tall_tiles_match_oracle_and_short_tiles(gpu, w, h, content, zero_skip):
    seq, exp = _oracle(w, h, content)
    tall, sse_t = _encode(gpu, seq, w, h, 1, zero_skip)
    short, sse_s = _encode(gpu, seq, w, h, 0, zero_skip)
    for i in range(FRAMES):
        assert tall[i]["frame_type"] == exp[i]["frame_type"] == short[i]["frame_type"]
        for k in KEYS:
            a, b = tall[i][k], np.asarray(exp[i][k])
            assert a.shape == b.shape, (i, k, a.shape, b.shape)
            bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
            assert bad.size == 0, f"frame {i} {k}: {bad.size} differ from the oracle, first at {bad[:3].tolist()}"
        if "mae_num" in exp[i]:
            assert (tall[i]["mae_num"] == np.asarray(exp[i]["mae_num"])).all(), (i, "mae_num")
        for k in KEYS + ("mae_num",):
            assert np.array_equal(tall[i][k], short[i][k]), f"frame {i} {k}: tall and short tiles differ"
        assert sse_t[i] == exp[i]["sse_total"] == sse_s[i], (i, sse_t[i], exp[i]["sse_total"], sse_s[i])


def test_tile_rows_rule(gpu):
    """Unset: 48-row tiles where a frame offers at least as many of them as the grid has slots
    (4K: 1,350 tiles) and 32-row tiles below that (1088p: 345); 0 / 1 force the choice."""
    lib = _lib.load()
    assert lib.so_get_option(_lib.OPT_RUN_TALL_TILES) == -1
    assert lib.so_p_run_tile_rows(2160, 3840, 1) == 3
    assert lib.so_p_run_tile_rows(1088, 1920, 1) == 2
    with _lib.option(_lib.OPT_RUN_TALL_TILES, 0):
        assert lib.so_p_run_tile_rows(2160, 3840, 1) == 2
    with _lib.option(_lib.OPT_RUN_TALL_TILES, 1):
        assert lib.so_p_run_tile_rows(1088, 1920, 1) == 3
    assert lib.so_get_option(_lib.OPT_RUN_TALL_TILES) == -1
