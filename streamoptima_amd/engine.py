"""Device-resident frame engine: HBM buffers + launches of the gfx950 kernels.

Everything here stays on the GPU: frames, reconstructions, symbols (split / mv / qtc /
tokens / mae) and scratch are torch uint8/int16/int32 tensors allocated once and reused;
each frame is one or two C-ABI calls on the current stream with no host synchronisation.
The Python facade (Encoder.py / decoder.py) builds the reference's data structures from
these tensors only when asked.
"""
from __future__ import annotations

import collections
import contextlib
from dataclasses import dataclass, field

import os

import torch

from . import _lib, runhealth

SLACK = 64  # bytes readable past every plane (kernels read aligned words at row ends)
RUN_TIMEOUT_WORD = runhealth.TIMEOUT_WORD     # so_encode_p_run workspace (include/streamoptima.h)
RUN_FALLBACK_WORD = runhealth.FALLBACK_WORD   # blocks whose SEA search took the dense fallback


def alloc_planes(n: int, h: int, w: int, device, fill: int | None = None) -> torch.Tensor:
    """[n, h, w] uint8 planes laid out back to back with SLACK bytes after the last one."""
    flat = torch.empty(n * h * w + SLACK, dtype=torch.uint8, device=device)
    if fill is not None:
        flat.fill_(fill)
    else:
        flat[n * h * w:].zero_()
    return flat[: n * h * w].view(n, h, w)


def ssim_planes(lib, device, a_planes, b_planes, h: int, w: int, win: int, out, ws: torch.Tensor) -> torch.Tensor:
    """so_ssim_u8 over pairs of uint8 planes (2-D tensors with contiguous rows, one row stride
    per side) into `out` (float64 [n], allocated when None); `ws` is the float64 workspace."""
    a_planes, b_planes = list(a_planes), list(b_planes)
    n = len(a_planes)
    if len(b_planes) != n:
        raise ValueError(f"ssim: {n} planes against {len(b_planes)}")
    out = torch.empty(n, dtype=torch.float64, device=device) if out is None else out
    if out.dtype != torch.float64 or out.numel() != n or not out.is_contiguous() or out.device != ws.device:
        raise ValueError(f"ssim: out must be a contiguous float64 [{n}] tensor on {ws.device}")
    if n == 0:
        return out
    pitches = []
    for name, planes in (("a", a_planes), ("b", b_planes)):
        for t in planes:
            if (t.dtype != torch.uint8 or t.dim() != 2 or t.device != ws.device or t.shape[0] < h or t.shape[1] < w
                    or t.stride(1) != 1 or t.stride(0) != planes[0].stride(0)):
                raise ValueError(f"ssim: {name} planes must be uint8 2-D tensors of at least {h}x{w} on {ws.device} "
                                 "with contiguous rows and one row stride")
        pitches.append(int(planes[0].stride(0)))
    rc = lib.so_ssim_u8(_lib.ptr_array(a_planes), _lib.ptr_array(b_planes), n, int(h), int(w), pitches[0], pitches[1], int(win), out.data_ptr(), ws.data_ptr(),
                        _lib.stream_handle(device))
    _lib.check(rc, "so_ssim_u8")
    return out


def pack_coding_is_bits(coding: str) -> bool:
    """The packed stream's codings: False for "varint", True for "bits"; anything else raises."""
    if coding not in ("varint", "bits"):
        raise ValueError(f"packed stream coding {coding!r} (\"varint\" or \"bits\")")
    return coding == "bits"


PACK_CODINGS = {"varint": 1, "bits": 2, "huff": 3}     # the coding -> its container number


def pack_coding_suffix(coding: str) -> str:
    """The entry points' suffix for a coding of the packed stream: "" for "varint", "_bits" for
    "bits", "_huff" for "huff" (per-frame Huffman tables); anything else raises."""
    if coding not in PACK_CODINGS:
        raise ValueError(f"packed stream coding {coding!r} (\"varint\", \"bits\" or \"huff\")")
    return "" if coding == "varint" else "_" + coding


@dataclass
class FrameSymbols:
    """Per-frame output of the encode path (canonical layout, include/streamoptima.h)."""
    frame_type: int            # 0 = intra, 1 = inter
    split: torch.Tensor        # uint8 [nb]
    mv: torch.Tensor           # int16 [nb, 4, 3] (inter) or [nb, 4] (intra)
    qtc: torch.Tensor          # int16 [nb, bs*bs]
    tokens: torch.Tensor       # int32 [nb]
    mae_num: torch.Tensor      # int32 [nb]  (block MAE * bs^2, -1 = inf)
    recon: torch.Tensor        # uint8 [h, w]
    sse: torch.Tensor | None = None   # int32 [max(nb, h)]: per-block (P) / per-row (I) SSE, zero-padded
    qp_rd: int = 0
    qp_row: list | None = None
    extra: dict = field(default_factory=dict)


@dataclass
class ChromaSymbols:
    """Per-frame output of the chroma path (include/streamoptima.h so_chroma_encode_frame)."""
    frame_type: int                    # the luma frame's
    qtc_u: torch.Tensor                # int16 [nb, 64]
    qtc_v: torch.Tensor
    recon_u: torch.Tensor              # uint8 [h/2, w/2]
    recon_v: torch.Tensor
    tokens: torch.Tensor | None = None   # int32 [2, nb] (U, V); None from recon_chroma
    sse: torch.Tensor | None = None      # int32 [2, nb]
    qp_offset: int = 0


class Engine:
    """Kernels for one frame geometry on one device."""

    def __init__(self, height: int, width: int, block_size: int = 16, search_range: int = 16,
                 vbs: bool = False, lam: float | None = None, device=None, me_mode: int = 0, fme: bool = False,
                 chroma_subpel: bool = False):
        if height % block_size or width % block_size:
            raise ValueError(f"frame {width}x{height} is not a multiple of block_size {block_size}")
        self.h, self.w, self.bs, self.sr = height, width, block_size, search_range
        self.vbs = bool(vbs)
        self.lam = float(lam) if lam is not None else 0.0
        if self.vbs and lam is None:
            raise ValueError("VBSEnable needs lam (calculate_RD_cost multiplies by it)")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.HipPathError("the encode path runs on a ROCm GPU only (no CPU fallback)")
        self.lib = _lib.load()
        self.nbx, self.nby = width // block_size, height // block_size
        self.nb = self.nbx * self.nby
        ps = self.lib.so_p_frame_scratch_elems(height, width, block_size, int(self.vbs))
        is_ = self.lib.so_i_frame_scratch_elems(height, width, block_size)
        self.scratch = torch.empty(max(ps, is_), dtype=torch.int32, device=self.device)
        # ME variant (include/streamoptima.h SO_ME_*): fast_me / FMEEnable
        self.me_mode = int(me_mode)
        self.fme = bool(fme)
        # chroma under FME: the half-sample luma vectors as quarter-sample chroma vectors (opt-in)
        self.chroma_subpel = bool(chroma_subpel)
        self._fme_ws = None
        self._consts: collections.OrderedDict = collections.OrderedDict()   # device_const_i32 (LRU)
        self._pinned_consts: set = set()                                    # ... held by captured graphs
        self._pin_depth = 0   # > 0 inside pinned_consts()
        self.wait_health = runhealth.HealthLog()   # non-fatal wait counts of the persistent runs

    MAX_CONSTS = 4096

    def device_const_i32(self, values) -> torch.Tensor:
        """A read-only int32 device copy of `values`, uploaded once per distinct content, so
        a GOP replayed from a captured HIP graph issues no host->device copy.

        The cache is LRU-bounded at MAX_CONSTS entries, except that an entry looked up while
        a HIP graph is being captured on this device, or inside `with engine.pinned_consts():`,
        is pinned: a graph holds its raw device pointer, so evicting it would make a later replay
        read freed memory.  A constant fetched BEFORE a capture and only used inside it must be
        fetched again inside the capture or under pinned_consts() (the facade looks its constants
        up on every call, so a captured encode re-fetches them).  Pinned entries are dropped only
        by release_consts(), which the owner of such a graph calls once the graph is gone."""
        host = torch.as_tensor(values, dtype=torch.int32).contiguous()
        key = (tuple(host.shape), host.numpy().tobytes())
        t = self._consts.get(key)
        if t is None:
            t = self._consts[key] = host.to(self.device)
            if len(self._consts) > self.MAX_CONSTS:   # evict the least recently used unpinned entry
                for k in self._consts:
                    if k not in self._pinned_consts and k != key:
                        del self._consts[k]
                        break
        else:
            self._consts.move_to_end(key)
        if self._pin_depth > 0 or (self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            self._pinned_consts.add(key)
        return t

    @contextlib.contextmanager
    def pinned_consts(self):
        """Every device constant looked up inside the block is pinned (never LRU-evicted): for
        constants fetched ahead of a graph capture that the graph will use."""
        self._pin_depth += 1
        try:
            yield self
        finally:
            self._pin_depth -= 1

    def release_consts(self) -> None:
        """Drop the cached device constants (ROI offsets, row-QP schedules), pinned ones too.
        Only safe when no captured HIP graph that used them will be replayed again."""
        self._consts.clear()
        self._pinned_consts.clear()

    def fme_workspace(self, nref: int) -> torch.Tensor:
        """Phase planes of the references' frac frames (rebuilt by every FME call)."""
        need = self.lib.so_fme_workspace_bytes(self.h, self.w, nref)
        if self._fme_ws is None or self._fme_ws.numel() < need:
            self._fme_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        return self._fme_ws

    # ---- allocation ----------------------------------------------------------------------
    def new_symbols(self, frame_type: int) -> FrameSymbols:
        d, nb, bs = self.device, self.nb, self.bs
        mv_shape = (nb, 4, 3) if frame_type == 1 else (nb, 4)
        return FrameSymbols(frame_type=frame_type,
                            split=torch.empty(nb, dtype=torch.uint8, device=d),
                            mv=torch.empty(mv_shape, dtype=torch.int16, device=d),
                            qtc=torch.empty((nb, bs * bs), dtype=torch.int16, device=d),
                            tokens=torch.empty(nb, dtype=torch.int32, device=d),
                            mae_num=torch.empty(nb, dtype=torch.int32, device=d),
                            recon=alloc_planes(1, self.h, self.w, d)[0],
                            sse=torch.zeros(max(nb, self.h), dtype=torch.int32, device=d))

    def qp_row_tensor(self, qp_row) -> torch.Tensor | None:
        if qp_row is None:
            return None
        t = torch.as_tensor(list(qp_row), dtype=torch.int32)
        if t.numel() != self.nby:
            raise ValueError(f"qp_row needs {self.nby} entries, got {t.numel()}")
        return self.device_const_i32(t)

    def _check_plane(self, t: torch.Tensor, name: str):
        if t.dtype != torch.uint8 or t.device != self.device or tuple(t.shape) != (self.h, self.w):
            raise ValueError(f"{name} must be a uint8 {self.h}x{self.w} tensor on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")

    # ---- encode -------------------------------------------------------------------------
    def encode_p(self, cur: torch.Tensor, refs: list, qp_rd: int, qp_row=None,
                 out: FrameSymbols | None = None, qp_row_dev: torch.Tensor | None = None,
                 fme_wrap: bool = True, qp_map_dev: torch.Tensor | None = None,
                 reuse_me: bool = False, tokens_only: bool = False) -> FrameSymbols:
        """complete_inter_flow (Encoder.py:1644) for one frame; asynchronous.
        fme_wrap: see so_encode_p_rows_ex (False while refs hold the float64 start frame);
        qp_map_dev: per-block QP (ROI / two-pass RC); reuse_me: keep the ME records of the
        previous encode_p of the same frame (pass 2); tokens_only: pass 1 of two-pass RC (only
        the tokens and the ME records are guaranteed, SO_TOKENS_ONLY)."""
        return self.encode_p_rows(cur, refs, 0, self.nby, qp_rd, out or self.new_symbols(1),
                                  qp_row_dev if qp_row_dev is not None else self.qp_row_tensor(qp_row),
                                  fme_wrap=fme_wrap, qp_map_dev=qp_map_dev, reuse_me=reuse_me, qp_row=qp_row,
                                  tokens_only=tokens_only)

    def encode_i(self, cur: torch.Tensor, qp_rd: int, qp_row=None, out: FrameSymbols | None = None,
                 qp_row_dev: torch.Tensor | None = None, qp_map_dev: torch.Tensor | None = None) -> FrameSymbols:
        """complete_intra_flow (Encoder.py:1582), intra_mode 0, for one frame; asynchronous."""
        return self.encode_i_rows(cur, 0, self.nby, qp_rd, out or self.new_symbols(0),
                                  qp_row_dev if qp_row_dev is not None else self.qp_row_tensor(qp_row),
                                  qp_map_dev=qp_map_dev, qp_row=qp_row)

    def qp_map(self, tokens: torch.Tensor | None, qp_rd: int, qp_row_dev: torch.Tensor | None,
               roi_dev: torch.Tensor | None, out: torch.Tensor, by0: int = 0, by1: int | None = None,
               qp_lo: int = 0, qp_hi: int = 12) -> torch.Tensor:
        """so_qp_map: the per-block QP map of ROI / two-pass RC into `out` (int32 [nb])."""
        by1 = self.nby if by1 is None else by1
        rc = self.lib.so_qp_map(_lib.ptr(tokens), self.h, self.w, self.bs, int(by0), int(by1), int(qp_rd),
                                _lib.ptr(qp_row_dev), _lib.ptr(roi_dev), int(qp_lo), int(qp_hi), out.data_ptr(),
                                _lib.stream_handle(self.device))
        _lib.check(rc, "so_qp_map")
        return out

    # ---- stripes (multi-GPU sharding) --------------------------------------
    def new_stripe_symbols(self, frame_type: int, by0: int, by1: int, recon: torch.Tensor) -> FrameSymbols:
        """Stripe-local symbol buffers for block rows [by0, by1); `recon` is the full plane
        the stripe's rows are written into."""
        d, bs = self.device, self.bs
        nbs = self.nbx * (by1 - by0)
        mv_shape = (nbs, 4, 3) if frame_type == 1 else (nbs, 4)
        return FrameSymbols(frame_type=frame_type,
                            split=torch.empty(nbs, dtype=torch.uint8, device=d),
                            mv=torch.empty(mv_shape, dtype=torch.int16, device=d),
                            qtc=torch.empty((nbs, bs * bs), dtype=torch.int16, device=d),
                            tokens=torch.empty(nbs, dtype=torch.int32, device=d),
                            mae_num=torch.empty(nbs, dtype=torch.int32, device=d),
                            recon=recon,
                            sse=torch.zeros(max(nbs, (by1 - by0) * bs), dtype=torch.int32, device=d),
                            extra={"by0": by0, "by1": by1})

    @staticmethod
    def out_arrays(outs: list) -> tuple:
        """The seven per-frame output pointer arrays of the run entry points, in argument order
        (split, mv, qtc, tokens, mae_num, recon, sse), for a list of FrameSymbols."""
        return tuple(_lib.ptr_array([getattr(o, k) for o in outs])
                     for k in ("split", "mv", "qtc", "tokens", "mae_num", "recon", "sse"))

    @staticmethod
    def _stamp(outs: list, frame_type: int, qp_rd: int, qp_row) -> None:
        """What the encode calls record on the symbols they filled."""
        for o in outs:
            o.frame_type, o.qp_rd = frame_type, int(qp_rd)
            o.qp_row = None if qp_row is None else list(qp_row)

    def _check_offs(self, offs: list, what: str) -> None:
        for o in offs:
            if o.dtype != torch.int32 or o.numel() != self.nb + 1 or not o.is_contiguous():
                raise ValueError(f"{what}: offs must be contiguous int32 [{self.nb + 1}]")

    def _run_workspace(self) -> torch.Tensor:
        """The persistent runs' workspace, allocated on first use."""
        if getattr(self, "_run_ws", None) is None:
            # the timeout count (RUN_TIMEOUT_WORD) is zeroed here once and then only by check_run
            self._run_ws = torch.zeros(self.lib.so_p_run_workspace_elems(self.h, self.w), dtype=torch.int32,
                                       device=self.device)
        return self._run_ws

    def encode_p_rows(self, cur, refs, by0: int, by1: int, qp_rd: int, out: FrameSymbols,
                      qp_row_dev: torch.Tensor | None = None, fme_wrap: bool = True,
                      qp_map_dev: torch.Tensor | None = None, reuse_me: bool = False, qp_row=None,
                      tokens_only: bool = False) -> FrameSymbols:
        """so_encode_p_rows(_ex): block rows [by0, by1) of a P-frame; asynchronous."""
        self._check_plane(cur, "cur")
        for k, r in enumerate(refs):
            self._check_plane(r, f"refs[{k}]")
        if not 1 <= len(refs) <= _lib.MAX_REF:
            raise ValueError(f"nRefFrames must be in [1, {_lib.MAX_REF}]")
        st = _lib.stream_handle(self.device)
        if self.me_mode == _lib.ME_FULL and not self.fme and qp_map_dev is None and not reuse_me and not tokens_only:
            rc = self.lib.so_encode_p_rows(
                cur.data_ptr(), _lib.ref_array(refs), len(refs), self.h, self.w, self.bs, self.sr, int(by0), int(by1),
                int(qp_rd), _lib.ptr(qp_row_dev), int(self.vbs), self.lam, out.split.data_ptr(), out.mv.data_ptr(),
                out.qtc.data_ptr(), out.tokens.data_ptr(), out.mae_num.data_ptr(), out.recon.data_ptr(),
                _lib.ptr(out.sse), self.scratch.data_ptr(), st)
            _lib.check(rc, "so_encode_p_rows")
        else:
            ws = self.fme_workspace(len(refs)) if self.fme else None
            rc = self.lib.so_encode_p_rows_ex(
                cur.data_ptr(), _lib.ref_array(refs), len(refs), self.h, self.w, self.bs, self.sr, int(by0), int(by1),
                int(qp_rd), _lib.ptr(qp_row_dev), _lib.ptr(qp_map_dev), int(self.vbs), self.lam, self.me_mode,
                int(self.fme), int(bool(fme_wrap)), _lib.ptr(ws), (_lib.REUSE_ME if reuse_me else 0) | (_lib.TOKENS_ONLY if tokens_only else 0),
                out.split.data_ptr(), out.mv.data_ptr(), out.qtc.data_ptr(), out.tokens.data_ptr(),
                out.mae_num.data_ptr(), out.recon.data_ptr(), _lib.ptr(out.sse), self.scratch.data_ptr(), st)
            _lib.check(rc, "so_encode_p_rows_ex")
        self._stamp([out], 1, qp_rd, qp_row)
        return out

    # ---- P-frame runs (one persistent launch) ----------------------------------------------
    def pipelined_ok(self, nref: int = 1, vbs_ok: bool = True) -> bool:
        """The configurations encode_p_run covers: the fused search + transform kernel
        (bs 16, sr 16, full search, no FME, one reference) on whole 128-byte rows; VBSEnable
        too unless vbs_ok is False (the two-pass RC run and the stripe hand-off)."""
        return (self.bs == 16 and self.sr == 16 and self.me_mode == _lib.ME_FULL and not self.fme
                and (vbs_ok or not self.vbs) and nref == 1 and self.w % 128 == 0)

    def encode_p_run(self, curs: list, ref0: torch.Tensor, qp_rd: int, outs: list, qp_row=None,
                     qp_row_dev: torch.Tensor | None = None) -> list:
        """so_encode_p_run: a run of consecutive P-frames (frame i predicts from frame i-1's
        reconstruction, ref0 for the first) as one persistent launch whose workgroups start
        a tile of frame i as soon as the rows of frame i-1 its window reads are done, so
        only the run's last frame has a launch tail.  Symbols identical to per-frame
        encode_p; asynchronous."""
        if not self.pipelined_ok():
            raise ValueError("encode_p_run covers bs 16 / sr 16 / full search / no FME / W % 128 == 0")
        n = len(curs)
        if n == 0:
            return []
        qrd = qp_row_dev if qp_row_dev is not None else self.qp_row_tensor(qp_row)
        for t, name in [(ref0, "ref0")] + [(c, "cur") for c in curs]:
            self._check_plane(t, name)
        ws = self._run_workspace()
        with self._zero_skip_option():
            rc = self.lib.so_encode_p_run(
                _lib.ptr_array(curs), n, ref0.data_ptr(), self.h, self.w, self.bs, self.sr, int(qp_rd), _lib.ptr(qrd),
                int(self.vbs), self.lam, *self.out_arrays(outs), ws.data_ptr(), _lib.stream_handle(self.device))
        _lib.check(rc, "so_encode_p_run")
        self._last_run_outs = list(outs)
        self._stamp(outs, 1, qp_rd, qp_row)
        return outs

    def encode_p_run_2pass(self, curs: list, ref0: torch.Tensor, qp_rd: int, outs: list, qp_maps: list,
                           qp_row=None, qp_row_dev: torch.Tensor | None = None, roi_dev: torch.Tensor | None = None,
                           qp_lo: int = 0, qp_hi: int = 12) -> list:
        """so_encode_p_run_2pass: a run of P-frames with two-pass rate control (pass 1 at the
        row QP, per-block QPs from the row's pass-1 token statistics and the ROI, pass 2 at
        those QPs on pass 1's motion vectors) as ONE persistent launch.  qp_maps[i] (int32
        [nb]) receives frame i's QPs.  Symbols identical to encode_p + qp_map + encode_p
        (reuse_me) per frame; asynchronous."""
        if not self.pipelined_ok(vbs_ok=False):
            raise ValueError("encode_p_run_2pass covers bs 16 / sr 16 / full search / no VBS, FME / W % 128 == 0")
        n = len(curs)
        if n == 0:
            return []
        qrd = qp_row_dev if qp_row_dev is not None else self.qp_row_tensor(qp_row)
        for t, name in [(ref0, "ref0")] + [(c, "cur") for c in curs]:
            self._check_plane(t, name)
        for m in qp_maps:
            if m.dtype != torch.int32 or m.numel() != self.nb or m.device != self.device or not m.is_contiguous():
                raise ValueError(f"qp_maps entries must be contiguous int32 [{self.nb}] on {self.device}")
        rc = self.lib.so_encode_p_run_2pass(
            _lib.ptr_array(curs), n, ref0.data_ptr(), self.h, self.w, self.bs, self.sr, int(qp_rd), _lib.ptr(qrd),
            _lib.ptr(roi_dev), int(qp_lo), int(qp_hi), *self.out_arrays(outs), _lib.ptr_array(qp_maps),
            self._run_workspace().data_ptr(), _lib.stream_handle(self.device))
        _lib.check(rc, "so_encode_p_run_2pass")
        self._stamp(outs, 1, qp_rd, qp_row)
        for o, m in zip(outs, qp_maps):
            o.extra["qp_map"] = m
        return outs

    def encode_p_runs(self, runs: list, qp_rd: int, qp_row=None, qp_row_dev: torch.Tensor | None = None) -> list:
        """so_encode_p_runs: several independent P-frame runs -- runs[r] = (curs, ref0, outs),
        frame i of a run predicting from frame i-1's reconstruction and frame 0 from ref0 --
        in ONE persistent launch, interleaved frame by frame (A1 B1 A2 B2 ...) so that a frame
        of every run is in flight at once.  Each run's symbols are identical to encode_p_run
        of that run alone; asynchronous."""
        if not self.pipelined_ok():
            raise ValueError("encode_p_runs covers bs 16 / sr 16 / full search / no FME / W % 128 == 0")
        qrd = qp_row_dev if qp_row_dev is not None else self.qp_row_tensor(qp_row)
        curs, refs, ref_frame, outs, last = [], [], [], [], {}
        for k in range(max((len(r[0]) for r in runs), default=0)):
            for r, (rc, r0, ro) in enumerate(runs):
                if k >= len(rc):
                    continue
                if len(rc) != len(ro):
                    raise ValueError("encode_p_runs: a run's curs and outs differ in length")
                for t, name in ((rc[k], "cur"),) + (((r0, "ref0"),) if k == 0 else ()):
                    self._check_plane(t, name)
                curs.append(rc[k])
                refs.append(r0 if k == 0 else None)
                ref_frame.append(-1 if k == 0 else last[r])
                last[r] = len(outs)
                outs.append(ro[k])
        n = len(curs)
        if n == 0:
            return []
        ws = self._run_workspace()
        with self._zero_skip_option():
            rc = self.lib.so_encode_p_runs(
                _lib.ptr_array(curs), n, _lib.ptr_array(refs), _lib.i32_array(ref_frame), self.h, self.w, self.bs,
                self.sr, int(qp_rd), _lib.ptr(qrd), int(self.vbs), self.lam, *self.out_arrays(outs), ws.data_ptr(),
                _lib.stream_handle(self.device))
        _lib.check(rc, "so_encode_p_runs")
        self._last_run_outs = list(outs)
        self._stamp(outs, 1, qp_rd, qp_row)
        return [r[2] for r in runs]

    def run_timed_out(self) -> bool:
        """True if a dependency wait of any encode_p_run since the last check_run timed out
        (never expected: the run's symbols would then be unreliable).  Synchronises."""
        return runhealth.timed_out(getattr(self, "_run_ws", None))

    def _zero_skip_option(self):
        """SO_OPT_RUN_ZERO_SKIP set around a launch when this engine chose the zero-skip kernel
        (left alone otherwise: the option's default is off)."""
        return _lib.option(_lib.OPT_RUN_ZERO_SKIP, 1) if self.zero_skip else contextlib.nullcontext()

    # the plain run's kernel choice by content (SO_OPT_RUN_ZERO_SKIP): the instantiation that
    # skips the IDCT of all-zero waves when at least this share of the last run's blocks
    # quantised to zero (flat content; exact either way)
    ZERO_SKIP_SHARE = float(os.environ.get("SO_ZERO_SKIP_SHARE", "0.5"))   # A/B: the share that selects it
    zero_skip = False

    def check_run(self, defer_stats: bool = False) -> None:
        """Raise if any encode_p_run since the last check timed out -- naming the first such
        wait from the workspace's diagnostic record (runhealth.describe) -- then clear the
        count; the non-fatal wait counts go to self.wait_health.  Encoder.encode() /
        encode_device(check=True) and bench.py call it once per GOP.  It also picks the
        plain run's kernel for the next runs from the last run's share of all-zero blocks
        (tokens == 1), read in the same synchronised check -- or, with defer_stats, counted
        on the stream into page-locked memory and read at the next check (one GOP later; the
        host-stream region, hoststream.py, does not wait for it)."""
        runhealth.check(getattr(self, "_run_ws", None), self.wait_health, "p_run_kernel")
        pend = getattr(self, "_zero_pending", None)
        if pend is not None:
            self._zero_pending = None
            ev, host, blocks = pend
            ev.synchronize()
            self.zero_skip = int(host[0]) >= self.ZERO_SKIP_SHARE * blocks
        outs = getattr(self, "_last_run_outs", None)
        if outs and not self.vbs:
            self._last_run_outs = None
            zero = torch.stack([(o.tokens == 1).sum() for o in outs]).sum()
            if defer_stats:
                if getattr(self, "_zero_host", None) is None:
                    self._zero_host = torch.empty(1, dtype=torch.int64, pin_memory=True)
                self._zero_host.copy_(zero.view(1), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._zero_pending = (ev, self._zero_host, self.nb * len(outs))
            else:
                self.zero_skip = zero.item() >= self.ZERO_SKIP_SHARE * self.nb * len(outs)

    def take_sad_ops(self) -> int:
        """SAD byte operations the persistent runs' searches executed since the last call
        (SO_P_RUN_SAD_OPS_WORD); clears the count.  Synchronises."""
        ws = getattr(self, "_run_ws", None)
        return 0 if ws is None else runhealth.take_u64(ws, runhealth.SAD_OPS_WORD)

    def take_fallback_count(self) -> int:
        """Blocks of the persistent runs since the last call whose exact SEA search took the
        dense fallback (SO_P_RUN_FALLBACK_WORD); clears the count.  Synchronises."""
        ws = getattr(self, "_run_ws", None)
        if ws is None:
            return 0
        n = int(ws[RUN_FALLBACK_WORD].item())
        ws[RUN_FALLBACK_WORD].zero_()
        return n

    def take_tq_fallback_counts(self) -> tuple:
        """(forward, inverse): wavefronts of the plain persistent runs since the last call whose
        fast transform re-ran the pocketfft sequence (SO_P_RUN_TQ_FALLBACK_WORD); clears the
        counts.  Synchronises."""
        ws = getattr(self, "_run_ws", None)
        if ws is None:
            return 0, 0
        w = ws[runhealth.TQ_FALLBACK_WORD:runhealth.TQ_FALLBACK_WORD + 2]
        n = tuple(int(v) & 0xFFFFFFFF for v in w.cpu().tolist())
        w.zero_()
        return n

    def encode_i_rows(self, cur, by0: int, by1: int, qp_rd: int, out: FrameSymbols,
                      qp_row_dev: torch.Tensor | None = None, qp_map_dev: torch.Tensor | None = None,
                      qp_row=None) -> FrameSymbols:
        """so_encode_i_rows_ex: block rows [by0, by1) of an I-frame; asynchronous."""
        self._check_plane(cur, "cur")
        rc = self.lib.so_encode_i_rows_ex(
            cur.data_ptr(), self.h, self.w, self.bs, self.sr, int(by0), int(by1), int(qp_rd), _lib.ptr(qp_row_dev),
            _lib.ptr(qp_map_dev), int(self.vbs), self.lam, out.split.data_ptr(), out.mv.data_ptr(),
            out.qtc.data_ptr(), out.tokens.data_ptr(), out.mae_num.data_ptr(), out.recon.data_ptr(),
            _lib.ptr(out.sse), self.scratch.data_ptr(), _lib.stream_handle(self.device))
        _lib.check(rc, "so_encode_i_rows_ex")
        self._stamp([out], 0, qp_rd, qp_row)
        return out

    # ---- decode ---------------------------------------------------------------------------
    def recon_inter(self, refs: list, split, mv, qtc, qp: int, qp_row=None, out=None,
                    fme_wrap: bool = True, qp_map_dev: torch.Tensor | None = None) -> torch.Tensor:
        out = out if out is not None else alloc_planes(1, self.h, self.w, self.device)[0]
        qr = self.qp_row_tensor(qp_row)
        ws = self.fme_workspace(len(refs)) if self.fme else None
        rc = self.lib.so_inter_recon_ex(_lib.ref_array(refs), len(refs), self.h, self.w, self.bs, int(qp),
                                        _lib.ptr(qr), _lib.ptr(qp_map_dev), int(self.fme), int(bool(fme_wrap)),
                                        _lib.ptr(ws), split.data_ptr(), mv.data_ptr(), qtc.data_ptr(), out.data_ptr(),
                                        _lib.stream_handle(self.device))
        _lib.check(rc, "so_inter_recon_ex")
        return out

    def recon_intra(self, split, mv, qtc, qp: int, qp_row=None, out=None,
                    qp_map_dev: torch.Tensor | None = None) -> torch.Tensor:
        out = out if out is not None else alloc_planes(1, self.h, self.w, self.device)[0]
        qr = self.qp_row_tensor(qp_row)
        rc = self.lib.so_intra_recon_ex(self.h, self.w, self.bs, int(qp), _lib.ptr(qr), _lib.ptr(qp_map_dev),
                                        split.data_ptr(), mv.data_ptr(), qtc.data_ptr(), out.data_ptr(),
                                        self.scratch.data_ptr(), _lib.stream_handle(self.device))
        _lib.check(rc, "so_intra_recon_ex")
        return out

    # ---- chroma 4:2:0 (so_chroma.hip) -----------------------------------------------------
    def new_chroma_symbols(self, frame_type: int = 0, encode: bool = True) -> ChromaSymbols:
        d, nb = self.device, self.nb
        rec = alloc_planes(2, self.h // 2, self.w // 2, d)
        return ChromaSymbols(frame_type=frame_type,
                             qtc_u=torch.empty((nb, 64), dtype=torch.int16, device=d),
                             qtc_v=torch.empty((nb, 64), dtype=torch.int16, device=d),
                             recon_u=rec[0], recon_v=rec[1],
                             tokens=torch.empty((2, nb), dtype=torch.int32, device=d) if encode else None,
                             sse=torch.empty((2, nb), dtype=torch.int32, device=d) if encode else None)

    def _check_chroma_plane(self, t: torch.Tensor, name: str):
        hc, wc = self.h // 2, self.w // 2
        if t.dtype != torch.uint8 or t.device != self.device or tuple(t.shape) != (hc, wc) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous uint8 {hc}x{wc} tensor on {self.device}")

    def _chroma_args(self, sym: FrameSymbols, refs_u: list, refs_v: list):
        """The luma frame's part of a chroma call: references, motion and the QP source.  Under
        FME, which chroma_subpel has to allow, the callers pass mv_frac_bits 2 to the _ex entry points."""
        if self.fme and not self.chroma_subpel:
            raise NotImplementedError("chroma with FMEEnable: the luma MVs are in half-pel units")
        inter = int(sym.frame_type) == 1
        if inter:
            if len(refs_u) != len(refs_v):
                raise ValueError(f"chroma: {len(refs_u)} U references against {len(refs_v)} V references")
            for k, (ru, rv) in enumerate(zip(refs_u, refs_v)):
                self._check_chroma_plane(ru, f"refs_u[{k}]")
                self._check_chroma_plane(rv, f"refs_v[{k}]")
            if sym.mv.dtype != torch.int16 or tuple(sym.mv.shape) != (self.nb, 4, 3) or sym.split.numel() != self.nb:
                raise ValueError(f"chroma: the luma symbols must be split [{self.nb}] and int16 mv [{self.nb}, 4, 3]")
        qm = sym.extra.get("qp_map")
        if qm is not None and (qm.dtype != torch.int32 or qm.numel() != self.nb or not qm.is_contiguous()):
            raise ValueError(f"chroma: the QP map must be contiguous int32 [{self.nb}]")
        qr = self.qp_row_tensor(sym.qp_row) if sym.qp_row else None
        return (_lib.ref_array(refs_u) if inter else None, _lib.ref_array(refs_v) if inter else None,
                len(refs_u) if inter else 0, self.h, self.w, self.bs, int(sym.frame_type),
                sym.split.data_ptr() if inter else None, sym.mv.data_ptr() if inter else None, int(sym.qp_rd),
                _lib.ptr(qr), _lib.ptr(qm))

    def encode_chroma(self, sym: FrameSymbols, cur_u: torch.Tensor, cur_v: torch.Tensor, refs_u: list, refs_v: list,
                      qp_offset: int = 0, out: ChromaSymbols | None = None) -> ChromaSymbols:
        """so_chroma_encode_frame: U and V of the frame whose luma symbols are `sym` (its frame
        type, split flags and motion vectors, and its QP source: the per-block map in
        sym.extra["qp_map"], else sym.qp_row, else sym.qp_rd), predicted from refs_u / refs_v --
        the chroma reconstructions in the luma reference list's order (ignored by an I-frame).
        One launch, stream-ordered after the luma work that wrote `sym`; asynchronous."""
        self._check_chroma_plane(cur_u, "cur_u")
        self._check_chroma_plane(cur_v, "cur_v")
        args = self._chroma_args(sym, refs_u, refs_v)
        out = out if out is not None and out.tokens is not None else self.new_chroma_symbols()
        if self.fme:   # with chroma_subpel (_chroma_args refused otherwise): half-sample luma vectors
            rc = self.lib.so_chroma_encode_frame_ex(cur_u.data_ptr(), cur_v.data_ptr(), *args, int(qp_offset),
                                                    out.qtc_u.data_ptr(), out.qtc_v.data_ptr(), out.tokens.data_ptr(),
                                                    out.recon_u.data_ptr(), out.recon_v.data_ptr(),
                                                    out.sse.data_ptr(), 2, _lib.stream_handle(self.device))
            _lib.check(rc, "so_chroma_encode_frame_ex")
            out.frame_type, out.qp_offset = int(sym.frame_type), int(qp_offset)
            return out
        rc = self.lib.so_chroma_encode_frame(cur_u.data_ptr(), cur_v.data_ptr(), *args, int(qp_offset),
                                             out.qtc_u.data_ptr(), out.qtc_v.data_ptr(), out.tokens.data_ptr(),
                                             out.recon_u.data_ptr(), out.recon_v.data_ptr(), out.sse.data_ptr(),
                                             _lib.stream_handle(self.device))
        _lib.check(rc, "so_chroma_encode_frame")
        out.frame_type, out.qp_offset = int(sym.frame_type), int(qp_offset)
        return out

    def recon_chroma(self, sym: FrameSymbols, qtc_u: torch.Tensor, qtc_v: torch.Tensor, refs_u: list, refs_v: list,
                     qp_offset: int = 0, out: ChromaSymbols | None = None) -> ChromaSymbols:
        """so_chroma_recon_frame: the decoder's U and V from the quantised coefficients
        (int16 [nb, 64] each) and the luma frame's symbols `sym` (only frame_type, split, mv and
        the QP source are read).  Returns a ChromaSymbols without tokens / sse; asynchronous."""
        for t, name in ((qtc_u, "qtc_u"), (qtc_v, "qtc_v")):
            if (t.dtype != torch.int16 or t.numel() != self.nb * 64 or t.device != self.device
                    or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous int16 [{self.nb}, 64] tensor on {self.device}")
        args = self._chroma_args(sym, refs_u, refs_v)
        if out is None:
            rec = alloc_planes(2, self.h // 2, self.w // 2, self.device)
            out = ChromaSymbols(int(sym.frame_type), qtc_u, qtc_v, rec[0], rec[1])
        else:
            out.qtc_u, out.qtc_v, out.tokens, out.sse = qtc_u, qtc_v, None, None
        if self.fme:
            rc = self.lib.so_chroma_recon_frame_ex(*args, int(qp_offset), qtc_u.data_ptr(), qtc_v.data_ptr(),
                                                   out.recon_u.data_ptr(), out.recon_v.data_ptr(), 2,
                                                   _lib.stream_handle(self.device))
            _lib.check(rc, "so_chroma_recon_frame_ex")
        else:
            rc = self.lib.so_chroma_recon_frame(*args, int(qp_offset), qtc_u.data_ptr(), qtc_v.data_ptr(),
                                                out.recon_u.data_ptr(), out.recon_v.data_ptr(),
                                                _lib.stream_handle(self.device))
            _lib.check(rc, "so_chroma_recon_frame")
        out.frame_type, out.qp_offset = int(sym.frame_type), int(qp_offset)
        return out

    # ---- packed symbol stream (so_pack_frames / so_pack_frames_bits) -----------------------
    def pack_bound(self, nb: int | None = None, coding: str = "varint") -> int:
        bound = getattr(self.lib, f"so_pack{pack_coding_suffix(coding)}_bound")
        return int(bound(int(self.nb if nb is None else nb), self.bs))

    def pack_symbols(self, syms: list, offs: torch.Tensor | None = None, out: torch.Tensor | None = None,
                     totals_ptr: int | None = None, coding: str = "varint"):
        """Each frame's symbols as one packed byte stream on the device (include/streamoptima.h
        so_pack_frames); asynchronous.  Returns (offs int32 [n, nb + 1], out uint8 [n, cap]):
        frame i's stream is out[i, :offs[i, nb]], block b starts at offs[i, b]
        (bitstream.unpack_frame decodes it).  The default capacity never overflows.
        totals_ptr: a device address of n uint32 (hostmem.device_ptr of a page-locked host
        array) that also receives offs[i, nb] (so_pack_frames_ex).
        coding: "varint" (so_pack_frames_ex) or "bits" (so_pack_frames_bits: Exp-Golomb codes,
        about half the bytes; bitstream.unpack_frame_bits decodes it) or "huff" (so_pack_frames_huff:
        Huffman codes from tables built per frame on the device; bitstream.unpack_frame_huff)."""
        name = "so_pack_frames" + (pack_coding_suffix(coding) or "_ex")
        n = len(syms)
        if n == 0:
            raise ValueError("pack_symbols: no frames")
        nb = syms[0].split.numel()
        if any(s.split.numel() != nb for s in syms):
            raise ValueError("pack_symbols: frames with different block counts")
        cap = self.pack_bound(nb, coding) if out is None else out.shape[1]
        offs = torch.empty((n, nb + 1), dtype=torch.int32, device=self.device) if offs is None else offs
        out = torch.empty((n, cap), dtype=torch.uint8, device=self.device) if out is None else out
        if offs.shape != (n, nb + 1) or offs.dtype != torch.int32 or out.shape[0] != n or out.dtype != torch.uint8:
            raise ValueError("pack_symbols: offs must be int32 [n, nb + 1] and out uint8 [n, cap]")
        arr, types = _lib.ptr_array, _lib.i32_array([s.frame_type for s in syms])
        rc = getattr(self.lib, name)(n, types, arr([s.split for s in syms]), arr([s.mv for s in syms]),
                                     arr([s.qtc for s in syms]), nb, self.bs, arr(list(offs)), arr(list(out)),
                                     int(cap), totals_ptr, _lib.stream_handle(self.device))
        _lib.check(rc, name[:-3] if name.endswith("_ex") else name)
        return offs, out

    def unpack_symbols(self, frame_types: list, packed: list, offs: list, coding: str = "varint") -> list:
        """so_unpack_frames (coding "varint"), so_unpack_frames_bits ("bits") or _huff ("huff"): packed streams
        (device uint8) + their block offsets (device int32 [nb + 1], as pack_symbols wrote them)
        -> FrameSymbols with split / mv / qtc (no recon, tokens or metrics).  Raises ValueError
        on a malformed stream (synchronises once)."""
        name = "so_unpack_frames" + pack_coding_suffix(coding)
        n = len(packed)
        syms = [self.new_symbols(int(t)) for t in frame_types]
        err = torch.zeros(1, dtype=torch.int32, device=self.device)
        arr, types = _lib.ptr_array, _lib.i32_array(frame_types)
        rc = getattr(self.lib, name)(n, types, arr(packed), arr(offs), self.nb, self.bs, arr([s.split for s in syms]),
                                     arr([s.mv for s in syms]), arr([s.qtc for s in syms]), err.data_ptr(),
                                     _lib.stream_handle(self.device))
        _lib.check(rc, name)
        bad = int(err.item())
        if bad:
            raise ValueError(f"{name}: malformed packed stream at block {bad - 1}")
        return syms

    # ---- packed chroma stream (so_pack_chroma_frames / so_pack_chroma_frames_bits) ------------
    def pack_chroma_bound(self, coding: str = "varint") -> int:
        return int(getattr(self.lib, f"so_pack_chroma{pack_coding_suffix(coding)}_bound")(self.nb))

    def pack_chroma_symbols(self, csyms: list, offs: torch.Tensor | None = None, out: torch.Tensor | None = None,
                            totals: torch.Tensor | None = None, coding: str = "varint",
                            after: torch.Tensor | None = None, totals_ptr: int | None = None):
        """Each frame's chroma coefficients (ChromaSymbols.qtc_u / .qtc_v) as one packed byte stream
        on the device (include/streamoptima.h so_pack_chroma_frames); asynchronous.  Returns (offs
        int32 [n, nb + 1], out uint8 [n, cap]) as pack_symbols does: frame i's stream is
        out[i, :offs[i, nb]], record b starts at offs[i, b].  The default capacity never overflows.
        totals: a device int32 [n] that also receives offs[i, nb]; totals_ptr: instead of it, a
        device address of n uint32 (hostmem.device_ptr of a page-locked host array).  coding:
        "varint", "bits" or "huff".
        after: the int32 [n, nb + 1] offsets pack_symbols filled for the same frames, earlier on this
        stream (so_pack_chroma_frames_after).  `out` is then required and is the tensor pack_symbols
        wrote, with room for both streams: frame i's chroma records go behind its luma bytes, to
        out[i, after[i, nb] + offs[i, b]], offs staying relative, and the totals receive the
        combined length after[i, nb] + offs[i, nb]."""
        suffix = pack_coding_suffix(coding)
        n, nb = len(csyms), self.nb
        if n == 0:
            raise ValueError("pack_chroma_symbols: no frames")
        for c in csyms:
            for t in (c.qtc_u, c.qtc_v):
                if t.dtype != torch.int16 or t.numel() != nb * 64 or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"pack_chroma_symbols: qtc_u / qtc_v must be contiguous int16 [{nb}, 64] "
                                     f"on {self.device}")
        if after is not None:
            if (after.dtype != torch.int32 or tuple(after.shape) != (n, nb + 1) or after.device != self.device
                    or after.stride(1) != 1):
                raise ValueError(f"pack_chroma_symbols: after must be the int32 [{n}, {nb + 1}] offsets of "
                                 f"pack_symbols on {self.device}, rows contiguous")
            need = self.pack_bound(nb, coding) + self.pack_chroma_bound(coding)
            if out is None or out.dim() != 2 or out.shape[1] < need:
                raise ValueError(f"pack_chroma_symbols: with after, out must be pack_symbols' out with a row "
                                 f"capacity of at least {need} bytes")
        cap = self.pack_chroma_bound(coding) if out is None else out.shape[1]
        offs = torch.empty((n, nb + 1), dtype=torch.int32, device=self.device) if offs is None else offs
        out = torch.empty((n, cap), dtype=torch.uint8, device=self.device) if out is None else out
        if offs.shape != (n, nb + 1) or offs.dtype != torch.int32 or out.shape[0] != n or out.dtype != torch.uint8:
            raise ValueError("pack_chroma_symbols: offs must be int32 [n, nb + 1] and out uint8 [n, cap]")
        if after is not None and (offs.device != self.device or out.device != self.device or offs.stride(1) != 1
                                  or out.stride(1) != 1):
            raise ValueError(f"pack_chroma_symbols: offs and out must be on {self.device} with contiguous rows")
        if totals is not None and (totals.dtype != torch.int32 or totals.numel() != n or not totals.is_contiguous()):
            raise ValueError("pack_chroma_symbols: totals must be a contiguous int32 [n]")
        if totals is not None and totals_ptr is not None:
            raise ValueError("pack_chroma_symbols: totals or totals_ptr, not both")
        tot = _lib.ptr(totals) if totals_ptr is None else int(totals_ptr)
        arr = _lib.ptr_array
        name = "so_pack_chroma_frames" + suffix
        base = ()
        if after is not None:
            name += "_after"
            base = (arr([after[i, nb:] for i in range(n)]),)
        rc = getattr(self.lib, name)(n, arr([c.qtc_u for c in csyms]), arr([c.qtc_v for c in csyms]), nb,
                                     arr(list(offs)), arr(list(out)), *base, int(cap), tot,
                                     _lib.stream_handle(self.device))
        _lib.check(rc, name)
        return offs, out

    def unpack_chroma_symbols(self, packed: list, offs: list, coding: str = "varint") -> list:
        """so_unpack_chroma_frames (coding "varint"), so_unpack_chroma_frames_bits ("bits") or _huff ("huff"):
        packed chroma streams (device uint8) + their record offsets (device int32 [nb + 1]) ->
        [(qtc_u, qtc_v)], int16 [nb, 64] each.  Raises ValueError on a malformed stream
        (synchronises once)."""
        name = "so_unpack_chroma_frames" + pack_coding_suffix(coding)
        n = len(packed)
        if n == 0 or len(offs) != n:
            raise ValueError("unpack_chroma_symbols: one offsets tensor per packed stream, at least one")
        self._check_offs(offs, "unpack_chroma_symbols")
        q = torch.empty((n, 2, self.nb, 64), dtype=torch.int16, device=self.device)
        err = torch.zeros(1, dtype=torch.int32, device=self.device)
        arr = _lib.ptr_array
        rc = getattr(self.lib, name)(n, arr(packed), arr(offs), self.nb, arr([q[i, 0] for i in range(n)]),
                                     arr([q[i, 1] for i in range(n)]), err.data_ptr(),
                                     _lib.stream_handle(self.device))
        _lib.check(rc, name)
        bad = int(err.item())
        if bad:
            raise ValueError(f"{name}: malformed packed chroma stream at record {bad - 1}")
        return [(q[i, 0], q[i, 1]) for i in range(n)]

    # ---- fused decode (so_decode_p_frames / so_decode_chroma_frames) ---------------------------
    @staticmethod
    def _coding_number(coding: str) -> int:
        pack_coding_suffix(coding)
        return PACK_CODINGS[coding]

    def _qp_ptrs(self, qps, n: int, what: str):
        """Per-frame QP sources as a host array of device pointers: each entry None, a device
        int32 tensor (used as it is) or a list (uploaded once per content, device_const_i32).
        Returns (array or None, the tensors to keep alive)."""
        if qps is None or all(q is None for q in qps):
            return None, []
        if len(qps) != n:
            raise ValueError(f"{what}: {len(qps)} entries for {n} frames")
        ts = [q if q is None or isinstance(q, torch.Tensor) else self.device_const_i32(list(q)) for q in qps]
        for t in ts:
            if t is not None and (t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"{what}: a contiguous int32 tensor on {self.device}")
        return _lib.ptr_array(ts), ts

    def decode_p_frames(self, packed: list, offs: list, refs0: list, nref_max: int, qp: int, qp_rows=None,
                        qp_maps=None, coding: str = "varint", out_split=None, out_mv=None, out_recon=None,
                        err: torch.Tensor | None = None):
        """so_decode_p_frames: a run of consecutive luma P-frames from their packed records
        (device uint8) and block offsets (device int32 [nb + 1]) straight to reconstructions, no
        dense coefficients in between.  refs0: the reference list before the run, oldest first;
        frame i predicts from the last min(nref_max, len(refs0) + i) planes of refs0 + the run's
        earlier reconstructions.  qp_rows / qp_maps: per frame None, a device int32 tensor
        ([nby] / [nb]) or a list.  out_*: lists of tensors to write (allocated when None); err: a
        zeroed device int32 [n] that receives 1 + a malformed block's index per frame (allocated
        when None).  Asynchronous: nothing is read back -- the caller checks err.
        Returns (split, mv, recon, err): three lists and the tensor."""
        n = len(packed)
        if len(offs) != n or n == 0:
            raise ValueError("decode_p_frames: one offsets tensor per packed stream, at least one")
        self._check_offs(offs, "decode_p_frames")
        for k, r in enumerate(refs0):
            self._check_plane(r, f"refs0[{k}]")
        d = self.device
        out_split = out_split or [torch.empty(self.nb, dtype=torch.uint8, device=d) for _ in range(n)]
        out_mv = out_mv or [torch.empty((self.nb, 4, 3), dtype=torch.int16, device=d) for _ in range(n)]
        out_recon = out_recon or list(alloc_planes(n, self.h, self.w, d))
        for k, r in enumerate(out_recon):
            self._check_plane(r, f"out_recon[{k}]")
        err = torch.zeros(n, dtype=torch.int32, device=d) if err is None else err
        if err.dtype != torch.int32 or err.numel() < n or err.device != d or not err.is_contiguous():
            raise ValueError(f"decode_p_frames: err must be a contiguous int32 [{n}] on {d}")
        qr, keep_r = self._qp_ptrs(qp_rows, n, "decode_p_frames qp_rows")
        qm, keep_m = self._qp_ptrs(qp_maps, n, "decode_p_frames qp_maps")
        arr = _lib.ptr_array
        rc = self.lib.so_decode_p_frames(n, self._coding_number(coding), arr(packed), arr(offs), self.h, self.w,
                                         self.bs, int(qp), qr, qm, arr(refs0) if refs0 else None, len(refs0),
                                         int(nref_max), arr(out_split), arr(out_mv), arr(out_recon), err.data_ptr(),
                                         _lib.stream_handle(d))
        _lib.check(rc, "so_decode_p_frames")
        return out_split, out_mv, out_recon, err

    def decode_chroma_frames(self, frame_types: list, packed: list, offs: list, split: list, mv: list, refs0_u: list,
                             refs0_v: list, nref_max: int, qp: int, qp_offset: int = 0, qp_rows=None, qp_maps=None,
                             coding: str = "varint", out_u=None, out_v=None, err: torch.Tensor | None = None):
        """so_decode_chroma_frames: U and V of a run of frames from their packed chroma records and
        the frames' luma split / mv (None for an I-frame).  The reference lists start as refs0_u /
        refs0_v, are cleared by an I-frame, take every reconstruction and hold at most nref_max
        planes.  Other arguments as decode_p_frames.  Returns (recon_u, recon_v, err).  Under FME
        with chroma_subpel the mv are the half-sample luma vectors (so_decode_chroma_frames_ex)."""
        if self.fme and not self.chroma_subpel:
            raise NotImplementedError("chroma with FMEEnable: the luma MVs are in half-pel units")
        n = len(packed)
        if n == 0 or len(offs) != n or len(frame_types) != n or len(split) != n or len(mv) != n:
            raise ValueError("decode_chroma_frames: one entry per frame in every list, at least one frame")
        self._check_offs(offs, "decode_chroma_frames")
        if len(refs0_u) != len(refs0_v):
            raise ValueError(f"chroma: {len(refs0_u)} U references against {len(refs0_v)} V references")
        for k, (ru, rv) in enumerate(zip(refs0_u, refs0_v)):
            self._check_chroma_plane(ru, f"refs0_u[{k}]")
            self._check_chroma_plane(rv, f"refs0_v[{k}]")
        d = self.device
        if out_u is None or out_v is None:
            pl = alloc_planes(2 * n, self.h // 2, self.w // 2, d)
            out_u, out_v = list(pl[:n]), list(pl[n:])
        for k, (u, v) in enumerate(zip(out_u, out_v)):
            self._check_chroma_plane(u, f"out_u[{k}]")
            self._check_chroma_plane(v, f"out_v[{k}]")
        err = torch.zeros(n, dtype=torch.int32, device=d) if err is None else err
        if err.dtype != torch.int32 or err.numel() < n or err.device != d or not err.is_contiguous():
            raise ValueError(f"decode_chroma_frames: err must be a contiguous int32 [{n}] on {d}")
        qr, keep_r = self._qp_ptrs(qp_rows, n, "decode_chroma_frames qp_rows")
        qm, keep_m = self._qp_ptrs(qp_maps, n, "decode_chroma_frames qp_maps")
        arr, types = _lib.ptr_array, _lib.i32_array(frame_types)
        args = (n, self._coding_number(coding), types, arr(packed), arr(offs), self.h, self.w, self.bs, arr(split),
                arr(mv), int(qp), qr, qm, int(qp_offset), arr(refs0_u) if refs0_u else None,
                arr(refs0_v) if refs0_v else None, len(refs0_u), int(nref_max), arr(out_u), arr(out_v), err.data_ptr())
        if self.fme:
            rc = self.lib.so_decode_chroma_frames_ex(*args, 2, _lib.stream_handle(d))
            _lib.check(rc, "so_decode_chroma_frames_ex")
        else:
            rc = self.lib.so_decode_chroma_frames(*args, _lib.stream_handle(d))
            _lib.check(rc, "so_decode_chroma_frames")
        return out_u, out_v, err

    # ---- metrics ---------------------------------------------------------------------------
    def sum_rows(self, rows: list, out: torch.Tensor | None = None) -> torch.Tensor:
        """int64 [n]: the sum of each int32 tensor in `rows` (equal lengths), one launch."""
        n = len(rows)
        length = rows[0].numel() if n else 0
        if any(r.numel() != length or r.dtype != torch.int32 or not r.is_contiguous() for r in rows):
            raise ValueError("sum_rows: contiguous int32 tensors of one length")
        out = torch.empty(n, dtype=torch.int64, device=self.device) if out is None else out
        rc = self.lib.so_sum_i32_rows(_lib.ptr_array(rows), n, length, out.data_ptr(), _lib.stream_handle(self.device))
        _lib.check(rc, "so_sum_i32_rows")
        return out

    def ssim(self, a_planes, b_planes, h: int, w: int, win: int = 11, out: torch.Tensor | None = None) -> torch.Tensor:
        """float64 [n] on the device: the SSIM (uniform win x win window, as the reference's
        skimage call) of a_planes[i] against b_planes[i] over their top-left h x w pixels, one
        batched so_ssim_u8 call, no host synchronisation.  The planes are uint8 2-D tensors
        (or [n, H, W] stacks) whose rows are contiguous; a padded plane is measured over its
        picture area through its row stride.  The workspace is cached on the engine."""
        n = len(a_planes)
        need = self.lib.so_ssim_workspace_elems(n, h, w, win)
        ws = getattr(self, "_ssim_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._ssim_ws = torch.empty(max(need, 1), dtype=torch.float64, device=self.device)
        return ssim_planes(self.lib, self.device, a_planes, b_planes, h, w, win, out, ws)

    # ---- colour conversion (so_colour.hip) ---------------------------------------------------
    def rgb_to_yuv420(self, rgb: torch.Tensor, colour=None, layout: str = "hwc", out_y: torch.Tensor | None = None,
                      out_uv: torch.Tensor | None = None, plane_hw=None):
        """8-bit RGB pictures -> (y [F, Hp, Wp], uv [F, 2, Hp/2, Wp/2]): the engine's padded planes
        in alloc_planes layout, every sample outside the picture 128, one so_rgb_to_yuv420 launch on
        the current stream, no host synchronisation.  rgb: uint8 [F, h, w, 3] ("hwc") or
        [F, 3, h, w] ("chw") on the device, h and w even and at most the engine's size; a cropped
        view of a larger picture converts in place (colour.rgb_pointers).  colour: a colour.Colour
        (None: BT.601, full range).  out_y / out_uv: planes to write, of exactly those shapes.
        plane_hw: (Hp, Wp) of the planes when they are not the engine's (even; the picture's own size
        for planes without padding)."""
        from . import colour as _colour
        col = _colour.as_colour(colour)
        ptrs, n, h, w, pitch, plane = _colour.rgb_pointers(rgb, layout, self.device)
        hp, wp = (int(plane_hw[0]), int(plane_hw[1])) if plane_hw else (self.h, self.w)
        if h % 2 or w % 2 or h > hp or w > wp:
            raise ValueError(f"rgb_to_yuv420: a {w}x{h} picture (even, at most the planes' {wp}x{hp})")
        if out_y is None:
            out_y = alloc_planes(n, hp, wp, self.device)
        if out_uv is None:
            out_uv = alloc_planes(2 * n, hp // 2, wp // 2, self.device).view(n, 2, hp // 2, wp // 2)
        py = _colour.plane_pointers(out_y, n, (hp, wp), self.device, "rgb_to_yuv420 out_y")
        pu = _colour.plane_pointers([t[0] for t in out_uv], n, (hp // 2, wp // 2), self.device, "rgb_to_yuv420 out_uv")
        pv = _colour.plane_pointers([t[1] for t in out_uv], n, (hp // 2, wp // 2), self.device, "rgb_to_yuv420 out_uv")
        rc = self.lib.so_rgb_to_yuv420(ptrs, n, h, w, _colour.layout_code(layout), pitch, plane, col.matrix_code,
                                       int(col.full_range), hp, wp, py, pu, pv, _lib.stream_handle(self.device))
        _lib.check(rc, "so_rgb_to_yuv420")
        return out_y, out_uv

    def yuv420_to_rgb(self, y, uv, h: int, w: int, colour=None, layout: str = "hwc",
                      out: torch.Tensor | None = None, plane_hw=None) -> torch.Tensor:
        """The inverse: the h x w picture area of padded planes -> uint8 [F, h, w, 3] ("hwc") or
        [F, 3, h, w] ("chw"), one so_yuv420_to_rgb launch on the current stream.  y: [F, Hp, Wp] or
        a sequence of [Hp, Wp] planes; uv: [F, 2, Hp/2, Wp/2] or a sequence of (u, v) plane pairs
        (Hp, Wp: the engine's size, or plane_hw when given).  out: a tensor or view of the result's shape
        to write into."""
        from . import colour as _colour
        col = _colour.as_colour(colour)
        hp, wp = (int(plane_hw[0]), int(plane_hw[1])) if plane_hw else (self.h, self.w)
        h, w = int(h), int(w)
        if h <= 0 or w <= 0 or h % 2 or w % 2 or h > hp or w > wp:
            raise ValueError(f"yuv420_to_rgb: a {w}x{h} picture (even, at most the planes' {wp}x{hp})")
        ys, uvs = list(y), list(uv)
        n = len(ys)
        if len(uvs) != n:
            raise ValueError(f"yuv420_to_rgb: {n} luma planes, {len(uvs)} chroma pairs")
        if out is None:
            out = torch.empty(_colour.rgb_shape(n, h, w, layout), dtype=torch.uint8, device=self.device)
        ptrs, on, oh, ow, pitch, plane = _colour.rgb_pointers(out, layout, self.device, "yuv420_to_rgb out")
        if (on, oh, ow) != (n, h, w):
            raise ValueError(f"yuv420_to_rgb: out holds {on} pictures of {ow}x{oh}, not {n} of {w}x{h}")
        py = _colour.plane_pointers(ys, n, (hp, wp), self.device, "yuv420_to_rgb y")
        pu = _colour.plane_pointers([t[0] for t in uvs], n, (hp // 2, wp // 2), self.device, "yuv420_to_rgb uv")
        pv = _colour.plane_pointers([t[1] for t in uvs], n, (hp // 2, wp // 2), self.device, "yuv420_to_rgb uv")
        rc = self.lib.so_yuv420_to_rgb(py, pu, pv, n, hp, wp, h, w, col.matrix_code, int(col.full_range),
                                       _colour.layout_code(layout), ptrs, pitch, plane, _lib.stream_handle(self.device))
        _lib.check(rc, "so_yuv420_to_rgb")
        return out

    # ---- scaling (so_scale.hip) --------------------------------------------------------------
    def scale_yuv420(self, y, uv, plan, src_hw=None, out_y: torch.Tensor | None = None,
                     out_uv: torch.Tensor | None = None, out_hw=None):
        """Resample 4:2:0 pictures with a scale.ScalePlan: one so_scale_yuv420 launch on the current
        stream, no host synchronisation.  y: [F, H, W] or a sequence of planes or views with
        contiguous rows; uv: [F, 2, H/2, W/2] or a sequence of (u, v) pairs, None for luma only.
        src_hw: the picture area read from the top-left of every plane (default: the whole plane);
        it must be plan.src_hw.  Returns (y [F, Hp, Wp], uv [F, 2, Hp/2, Wp/2] or None) with the
        plan.dst_hw picture top-left and 128 elsewhere: Hp x Wp is the engine's padded size in
        alloc_planes layout, or out_hw when given (plan.dst_hw itself for planes without padding).
        out_y / out_uv: planes of exactly those shapes to write."""
        from . import scale as _scale
        if not isinstance(plan, _scale.ScalePlan):
            raise ValueError(f"scale_yuv420: plan must be a streamoptima_amd.scale.ScalePlan, got {type(plan).__name__}")
        chroma = uv is not None
        if chroma and not plan.chroma:
            raise ValueError("scale_yuv420: the plan was built without chroma tables")
        ys = list(y)
        n = len(ys)
        hs, ws = _scale.check_size(src_hw if src_hw is not None else tuple(ys[0].shape[-2:]) if n else plan.src_hw,
                                   "scale_yuv420 src_hw", chroma)
        if (hs, ws) != plan.src_hw:
            raise ValueError(f"scale_yuv420: a {ws}x{hs} source, the plan takes {plan.src_hw[1]}x{plan.src_hw[0]}")
        hd, wd = plan.dst_hw
        hp, wp = _scale.check_size(out_hw, "scale_yuv420 out_hw", chroma) if out_hw is not None else (self.h, self.w)
        if hd > hp or wd > wp:
            raise ValueError(f"scale_yuv420: a {wd}x{hd} picture does not fit the {wp}x{hp} planes")
        psy, _, pitch_y = _scale.plane_views(ys, n, (hs, ws), self.device, "scale_yuv420 y")
        psu = psv = pdu = pdv = None
        pitch_c = 0
        if chroma:
            uvs = list(uv)
            psu, _, pitch_c = _scale.plane_views([t[0] for t in uvs], n, (hs // 2, ws // 2), self.device, "scale_yuv420 uv")
            psv, _, pitch_v = _scale.plane_views([t[1] for t in uvs], n, (hs // 2, ws // 2), self.device, "scale_yuv420 uv")
            if n and pitch_v != pitch_c:
                raise ValueError(f"scale_yuv420 uv: the planes of one call share a row pitch ({pitch_c} and {pitch_v})")
        from . import colour as _colour
        if out_y is None:
            out_y = alloc_planes(n, hp, wp, self.device)
        pdy = _colour.plane_pointers(out_y, n, (hp, wp), self.device, "scale_yuv420 out_y")
        if chroma:
            if out_uv is None:
                out_uv = alloc_planes(2 * n, hp // 2, wp // 2, self.device).view(n, 2, hp // 2, wp // 2)
            pdu = _colour.plane_pointers([t[0] for t in out_uv], n, (hp // 2, wp // 2), self.device, "scale_yuv420 out_uv")
            pdv = _colour.plane_pointers([t[1] for t in out_uv], n, (hp // 2, wp // 2), self.device, "scale_yuv420 out_uv")
        rc = self.lib.so_scale_yuv420(psy, psu, psv, n, hs, ws, pitch_y, pitch_c, pdy, pdu, pdv, hd, wd, hp, wp,
                                      *plan.table_args(), _lib.stream_handle(self.device))
        _lib.check(rc, "so_scale_yuv420")
        return out_y, (out_uv if chroma else None)

    # ---- deblocking post-filter (so_deblock.hip) ---------------------------------------------
    def _deblock_side(self, items, n: int, dtype, numel: int, what: str):
        """Per-frame device arrays of so_deblock_yuv420 (split, qp_rows, qp_maps) -> (pointer array or
        None, the tensors kept alive).  items: None, a tensor [n, numel], or a sequence of n entries,
        each None, a tensor of numel elements, or (int32 only) a sequence of ints."""
        from .colour import _on
        if items is None:
            return None, []
        ts = []
        for t in list(items):
            if t is not None and not isinstance(t, torch.Tensor):
                if dtype != torch.int32:
                    raise ValueError(f"deblock_yuv420 {what}: tensors of {dtype}, or None")
                t = self.device_const_i32([int(v) for v in t])
            if t is not None and (t.dtype != dtype or t.numel() != numel or not t.is_contiguous()
                                  or not _on(t, self.device)):
                raise ValueError(f"deblock_yuv420 {what}: contiguous {dtype} tensors of {numel} elements on "
                                 f"{self.device}, or None")
            ts.append(t)
        if len(ts) != n:
            raise ValueError(f"deblock_yuv420 {what}: {len(ts)} entries for {n} frames")
        return _lib.ptr_array(ts), ts

    def deblock_yuv420(self, y, uv, split=None, qp: int = 0, qp_rows=None, qp_maps=None, chroma_qp_offset: int = 0,
                       strength: int = 0, out_y: torch.Tensor | None = None, out_uv: torch.Tensor | None = None):
        """The display-side deblocking post-filter (include/streamoptima.h "Deblocking"): one
        so_deblock_yuv420 launch on the current stream, no host synchronisation.  y: [F, H, W] or a
        sequence of dense [H, W] planes (H, W multiples of the engine's block size: the padded planes
        the decoder holds); uv: [F, 2, H/2, W/2] or a sequence of (u, v) pairs, None for luma only.
        split: per frame the uint8 [nb] split flags or None (no block split); qp_rows / qp_maps: per
        frame an int32 [H / bs] / [nb] device tensor or None (map, then rows, then `qp`).  The sources
        are only read.  Returns (y [F, H, W], uv [F, 2, H/2, W/2] or None), written into out_y /
        out_uv when given (exactly those shapes, no byte shared with a source)."""
        from . import colour as _colour
        ys = list(y)
        n = len(ys)
        chroma = uv is not None
        h, w = (int(ys[0].shape[-2]), int(ys[0].shape[-1])) if n else (self.h, self.w)
        if h <= 0 or w <= 0 or h % self.bs or w % self.bs:
            raise ValueError(f"deblock_yuv420: {w}x{h} planes are not a positive multiple of block_size {self.bs}")
        nb = (h // self.bs) * (w // self.bs)
        psy = _colour.plane_pointers(ys, n, (h, w), self.device, "deblock_yuv420 y")
        psu = psv = pdu = pdv = None
        if chroma:
            uvs = list(uv)
            psu = _colour.plane_pointers([t[0] for t in uvs], n, (h // 2, w // 2), self.device, "deblock_yuv420 uv")
            psv = _colour.plane_pointers([t[1] for t in uvs], n, (h // 2, w // 2), self.device, "deblock_yuv420 uv")
        psplit, keep_s = self._deblock_side(split, n, torch.uint8, nb, "split")
        prow, keep_r = self._deblock_side(qp_rows, n, torch.int32, h // self.bs, "qp_rows")
        pmap, keep_m = self._deblock_side(qp_maps, n, torch.int32, nb, "qp_maps")
        if out_y is None:
            out_y = torch.empty((n, h, w), dtype=torch.uint8, device=self.device)
        pdy = _colour.plane_pointers(out_y, n, (h, w), self.device, "deblock_yuv420 out_y")
        if chroma:
            if out_uv is None:
                out_uv = torch.empty((n, 2, h // 2, w // 2), dtype=torch.uint8, device=self.device)
            pdu = _colour.plane_pointers([t[0] for t in out_uv], n, (h // 2, w // 2), self.device, "deblock_yuv420 out_uv")
            pdv = _colour.plane_pointers([t[1] for t in out_uv], n, (h // 2, w // 2), self.device, "deblock_yuv420 out_uv")
        rc = self.lib.so_deblock_yuv420(psy, psu, psv, n, h, w, self.bs, psplit, int(qp), prow, pmap,
                                        int(chroma_qp_offset), int(strength), pdy, pdu, pdv,
                                        _lib.stream_handle(self.device))
        _lib.check(rc, "so_deblock_yuv420")
        del keep_s, keep_r, keep_m
        return out_y, (out_uv if chroma else None)

    def sse_into(self, a: torch.Tensor, b: torch.Tensor, acc: torch.Tensor) -> None:
        """acc (uint64 view of an int64 device scalar) += sum((a-b)^2)."""
        rc = self.lib.so_sse_u8(a.data_ptr(), b.data_ptr(), a.numel(), acc.data_ptr(),
                                _lib.stream_handle(self.device))
        _lib.check(rc, "so_sse_u8")
