"""File-to-host-frames decode with the transfers overlapped: the receiving counterpart of
hoststream.HostStreamEncoder.

decoder.decode_packed_file loads the whole container, keeps the dense int16 coefficients of every
frame on the device at once and brings every plane down with a blocking copy.  Here the file is
read as it goes (packedfile.open_frames) and decoded by unit -- an I-frame, or up to `chunk`
consecutive P-frames -- with a fixed set of buffers whatever the file's length:

    host                  stage unit k+1 (payloads, lengths, QPs -> page-locked staging)
    copy stream A (H2D)   unit k+1's staging, one copy per frame, one event per unit
    compute stream        unit k: offsets, then so_unpack_frames + so_intra_recon_ex (I) or
                          so_decode_p_frames (P), and so_decode_chroma_frames
    copy stream B (D2H)   unit k-1's Y, U, V planes and error words -> page-locked host frames

The host waits for a unit only after it has queued the next one (nbuf = 2; nbuf = 1 runs the
units one after another).  P-frames and chroma never exist as dense coefficients in device
memory: the fused kernels (so_decode.hip) parse the packed records into LDS and transform them
there.  One dense symbol set serves every I-frame (and, with FMEEnable, every P-frame: the fused
kernel does not predict from the half-pel planes, so those go through so_unpack_frames +
so_inter_recon_ex).

With output="rgb" the compute stream ends a unit by converting its planes (so_yuv420_to_rgb) and
copy stream B brings down one [chunk, h, w, 3] buffer in place of the Y, U and V planes.

With output_size the compute stream first resamples the picture area of the unit's planes
(so_scale_yuv420) into planes of exactly that size; those are what is converted or downloaded.

With deblock (decoder(deblock=True)) every set also holds display planes for its unit.  The unit's
frames are filtered into them on the compute stream behind their reconstruction (so_deblock_yuv420),
and scaling, conversion and the download read the display planes; the ring below keeps the raw
reconstructions, which stay the references.

Reconstructions live in a ring of planes: a plane is written again only after its download
event (the compute stream waits for it) and, by stream order, after its last use as a reference.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, packedfile
from .colour import as_colour
from .engine import PACK_CODINGS, alloc_planes, pack_coding_suffix
from .hostmem import pinned_empty
from .hwqueue import dedicated_stream


def _a16(n: int) -> int:
    return -(-n // 16) * 16


class _Set:
    """One unit in flight: staging on both sides of the H2D copy, offsets, host frames."""

    def __init__(self, hs, dev):
        eng, c = hs.eng, hs.chunk
        self.stage_h = pinned_empty((c, hs.slot))
        self.stage_d = torch.empty((c, hs.slot), dtype=torch.uint8, device=dev)
        self.offs = torch.zeros((c, eng.nb + 1), dtype=torch.int32, device=dev)     # [:, 0] stays 0
        self.coffs = torch.zeros((c, eng.nb + 1), dtype=torch.int32, device=dev)
        self.err = torch.zeros((2, c), dtype=torch.int32, device=dev)               # luma row, chroma row
        self.sy_d = self.suv_d = self.db_y = self.db_uv = None
        if hs.deblock:
            # the unit's display planes: the deblocked frames, which nothing predicts from
            self.db_y = torch.empty((c, eng.h, eng.w), dtype=torch.uint8, device=dev)
            if hs.chroma_ok:
                self.db_uv = torch.empty((c, 2, eng.h // 2, eng.w // 2), dtype=torch.uint8, device=dev)
        if hs.out_hw:
            # the unit's planes at output size, resampled on the compute stream
            ho, wo = hs.out_hw
            self.sy_d = torch.empty((c, ho, wo), dtype=torch.uint8, device=dev)
            if hs.scale_plan.chroma:
                self.suv_d = torch.empty((c, 2, ho // 2, wo // 2), dtype=torch.uint8, device=dev)
        if hs.output == "rgb":
            # the unit's pictures, converted on the compute stream, and their one host copy
            hp, wp = hs.out_hw or (int(hs.dec.h_pixels), int(hs.dec.w_pixels))
            self.rgb_d = torch.empty((c, hp, wp, 3), dtype=torch.uint8, device=dev)
            self.rgb_h = pinned_empty((c, hp, wp, 3))
        elif hs.out_hw:
            self.y_h = pinned_empty(tuple(self.sy_d.shape))
            self.uv_h = pinned_empty(tuple(self.suv_d.shape)) if self.suv_d is not None else None
        else:
            self.y_h = pinned_empty((c, eng.h, eng.w))
            self.uv_h = pinned_empty((c, 2, eng.h // 2, eng.w // 2)) if hs.chroma_ok else None
        self.frames = []          # the unit: (index, frame type, bytes, chroma bytes, rows?, map?, plane)
        self.down = None          # D2H event of the unit


class HostStreamDecoder:
    def __init__(self, dec, chunk: int = 2, nbuf: int = 2, fused: bool = True, output: str = "yuv420", colour=None,
                 output_size=None, scale: str = "lanczos3", deblock=None, deblock_strength=None):
        """dec: a `decoder` (its geometry, Qp, nRefFrames, RCFlag, FMEEnable).  chunk: P-frames
        per unit; nbuf: units in flight.  fused=False decodes P-frames and chroma with the unpack
        and reconstruction kernels on the one dense symbol set instead of the fused kernels (the
        same frames; tools/decode_time.py compares the two).  output: "yuv420" = Y, U and V planes
        to the host; "rgb" = each unit's planes converted on the compute stream (so_yuv420_to_rgb
        with `colour`, a colour.Colour; None: BT.601, full range) and one [chunk, h, w, 3] buffer
        downloaded in their place.  output_size: (ho, wo) = the compute stream ends a unit by resampling
        the picture area of its planes to that size (so_scale_yuv420 with the `scale` filter:
        "bilinear", "bicubic" or "lanczos3") into planes of exactly that size, which are then converted
        (output="rgb": scale, then convert) or downloaded; a luma-only file scales luma alone.  None:
        nothing is staged and nothing resampled.  deblock / deblock_strength (None: dec.deblock,
        dec.deblock_strength): every unit's frames pass the deblocking post-filter (so_deblock_yuv420) on
        the compute stream into display planes of the unit's set; those are then resampled, converted
        or downloaded, and the reconstructions stay the references.  Off: no such plane exists and
        nothing is launched.  Every device and page-locked buffer is allocated here."""
        if output not in ("yuv420", "rgb"):
            raise ValueError(f"output {output!r} (\"yuv420\" or \"rgb\")")
        self.output, self.colour = output, as_colour(colour)
        if output == "rgb" and (dec.h_pixels % 2 or dec.w_pixels % 2):
            raise ValueError(f"output=\"rgb\" needs an even picture size, got {dec.w_pixels}x{dec.h_pixels}")
        self.fused = bool(fused)
        self.deblock = bool(getattr(dec, "deblock", False) if deblock is None else deblock)
        self.deblock_strength = int(getattr(dec, "deblock_strength", 0) if deblock_strength is None
                                    else deblock_strength)
        if not -3 <= self.deblock_strength <= 3:
            raise ValueError(f"deblock_strength {self.deblock_strength} outside [-3, 3]")
        self.out_hw = self.scale_plan = None
        if output_size is not None:
            from . import scale as _scale
            # chroma is resampled when this geometry can carry it; refusals before a buffer is allocated
            chroma = (int(dec.block_size) == 16 and (not dec.FMEEnable or getattr(dec, "chroma_subpel", False))
                      and dec.h_pixels % 2 == 0 and dec.w_pixels % 2 == 0)
            plan = ((int(dec.h_pixels), int(dec.w_pixels)), _scale.check_size(output_size, "output_size", chroma),
                    _scale.check_filter(scale))
            _scale.ScalePlan.check(*plan, chroma=chroma)
            self.out_hw = plan[1]
        eng = dec._eng()
        self.dec, self.eng, self.dev = dec, eng, eng.device
        self.chunk, self.nbuf = max(1, int(chunk)), max(1, int(nbuf))
        self.nref = int(dec.nRefFrames)
        if not 1 <= self.nref <= _lib.MAX_REF:
            raise ValueError(f"nRefFrames {self.nref} outside [1, {_lib.MAX_REF}]")
        self.fme = bool(dec.FMEEnable)
        self.subpel = self.fme and bool(getattr(dec, "chroma_subpel", False))   # chroma from half-sample vectors
        self.chroma_ok = eng.bs == 16 and (not self.fme or self.subpel)
        if output == "rgb" and not self.chroma_ok:
            raise NotImplementedError("output=\"rgb\" needs chroma, which needs block_size 16 and no FMEEnable")
        nb, nby, c = eng.nb, eng.nby, self.chunk
        # a frame's staging slot: u16 lengths | u16 chroma lengths | i32 row QPs | i32 QP map | luma
        # bytes | chroma bytes (the chroma bytes start 16-aligned behind the luma bytes, so one copy
        # of the slot's head carries the frame); capacities are the packers' bounds, any coding
        self.cap_l = max(eng.pack_bound(coding=c) for c in PACK_CODINGS)
        self.cap_c = max(eng.pack_chroma_bound(c) for c in PACK_CODINGS) if self.chroma_ok else 0
        self.o_clens = _a16(2 * nb)
        self.o_qrow = self.o_clens + _a16(2 * nb)
        self.o_qmap = self.o_qrow + _a16(4 * nby)
        self.o_pay = self.o_qmap + _a16(4 * nb)
        self.slot = self.o_pay + _a16(self.cap_l) + _a16(self.cap_c)
        # the same streams as HostStreamEncoder's: a process has few hardware queues (hwqueue.py)
        self.h2d = dedicated_stream(self.dev, "hoststream.h2d")
        self.d2h = dedicated_stream(self.dev, "hoststream.d2h")
        self.comp = dedicated_stream(self.dev, "hoststream.compute")
        if self.out_hw:
            self.scale_plan = _scale.ScalePlan(*plan, chroma=chroma, device=self.dev)
        self.sets = [_Set(self, self.dev) for _ in range(self.nbuf)]
        self.err_h = pinned_empty((self.nbuf, 2, c), torch.int32)        # one slab for every set's words
        self.tmp32 = torch.empty(nb, dtype=torch.int32, device=self.dev)
        # reconstructions: the units in flight, the references, and the unit being queued
        self.nring = self.nref + c * (self.nbuf + 1)
        self.planes = alloc_planes(self.nring, eng.h, eng.w, self.dev)
        self.plane_ev = [None] * self.nring
        self.ref128 = alloc_planes(1, eng.h, eng.w, self.dev, fill=128)[0]
        if self.chroma_ok:
            self.cplanes = alloc_planes(2 * self.nring, eng.h // 2, eng.w // 2, self.dev).view(
                self.nring, 2, eng.h // 2, eng.w // 2)
            self.c128 = alloc_planes(1, eng.h // 2, eng.w // 2, self.dev, fill=128)[0]
        # the fused luma kernel's symbols, read by the unit's chroma: one set for every unit (stream order)
        self.split = torch.empty((c, nb), dtype=torch.uint8, device=self.dev)
        self.mv = torch.empty((c, nb, 4, 3), dtype=torch.int16, device=self.dev)
        # the reusable dense symbol set: I-frames, and P-frames with FMEEnable
        self.d_split = torch.empty(nb, dtype=torch.uint8, device=self.dev)
        self.d_mv = torch.empty((nb, 4, 3), dtype=torch.int16, device=self.dev)      # intra: its first nb * 4
        self.d_qtc = torch.empty((nb, eng.bs * eng.bs), dtype=torch.int16, device=self.dev)
        self.d_qc = (torch.empty((2, nb, 64), dtype=torch.int16, device=self.dev)
                     if self.chroma_ok and not self.fused else None)
        self.fme_ws = eng.fme_workspace(self.nref) if self.fme else None
        torch.cuda.synchronize(self.dev)

    # ---- staging -------------------------------------------------------------------------------
    def _stage(self, s: _Set, j: int, i: int, rec: dict, hdr: dict) -> tuple:
        """Frame i's record into slot j of set s (host side); returns the unit's entry for it."""
        eng, nb = self.eng, self.eng.nb
        ft = rec["frame_type"]
        if ft not in (0, 1):
            raise ValueError(f"frame {i}: frame type {ft}")
        n = len(rec["payload"])
        nc = len(rec["chroma_payload"]) if hdr["chroma"] else 0
        if n > self.cap_l or nc > self.cap_c:
            raise ValueError(f"frame {i}: {n} luma / {nc} chroma bytes, more than any stream of {nb} blocks holds")
        h = s.stage_h[j].numpy()
        h[:2 * nb].view(np.uint16)[:] = rec["block_bytes"]
        rows = None
        if self.dec._rc() and rec["qp_rows"]:
            rows = np.asarray(rec["qp_rows"], np.int32)
            if rows.size != eng.nby or rows.min() < 0 or rows.max() > 20:
                raise ValueError(f"frame {i}: {rows.size} row QPs for {eng.nby} block rows, or one outside 0..20")
            h[self.o_qrow:self.o_qrow + 4 * eng.nby].view(np.int32)[:] = rows
        qmap = rec["qp_map"]
        if qmap is not None:
            if int(qmap.max()) > 20:
                raise ValueError(f"frame {i}: a QP map entry of {int(qmap.max())} (0..20)")
            h[self.o_qmap:self.o_qmap + 4 * nb].view(np.int32)[:] = qmap
        h[self.o_pay:self.o_pay + n] = np.frombuffer(rec["payload"], np.uint8)
        if nc:
            h[self.o_clens:self.o_clens + 2 * nb].view(np.uint16)[:] = rec["chroma_block_bytes"]
            o = self.o_pay + _a16(n)
            h[o:o + nc] = np.frombuffer(rec["chroma_payload"], np.uint8)
        return (i, ft, n, nc, rows is not None, qmap is not None)

    # ---- one unit on the three streams --------------------------------------------------------------
    def _offsets(self, lens16: torch.Tensor, out: torch.Tensor) -> None:
        """u16 lengths (as int16 bits) -> exclusive offsets, out[0] being 0 already."""
        self.tmp32.copy_(lens16)
        self.tmp32.bitwise_and_(0xFFFF)
        torch.cumsum(self.tmp32, 0, dtype=torch.int32, out=out[1:])

    def _queue(self, s: _Set, k: int, hdr: dict, state: dict) -> None:
        eng, nb, lib = self.eng, self.eng.nb, self.eng.lib
        unit, n = s.frames, len(s.frames)
        chroma = hdr["chroma"]
        coding = hdr["coding"]
        suffix = pack_coding_suffix(coding)
        fused = self.fused and coding != "huff"          # the fused decoders do not take "huff": unpack + recon
        with torch.cuda.stream(self.h2d):
            for j, (_, _, nl, nc, _, _) in enumerate(unit):
                m = self.o_pay + _a16(nl) + nc
                s.stage_d[j, :m].copy_(s.stage_h[j, :m], non_blocking=True)
            up = torch.cuda.Event()
            up.record(self.h2d)
        # this unit's planes
        ps = [(state["next_plane"] + j) % self.nring for j in range(n)]
        state["next_plane"] = (state["next_plane"] + n) % self.nring
        comp = self.comp
        with torch.cuda.stream(comp):
            comp.wait_event(up)
            for p in ps:
                if self.plane_ev[p] is not None:
                    comp.wait_event(self.plane_ev[p])       # its last download
                    self.plane_ev[p] = None
            s.err.zero_()
            sh = _lib.stream_handle(self.dev)
            packed, offs, cpacked, coffs, rows, maps = [], [], [], [], [], []
            for j, (_, _, nl, nc, has_rows, has_map) in enumerate(unit):
                d = s.stage_d[j]
                self._offsets(d[:2 * nb].view(torch.int16), s.offs[j])
                packed.append(d[self.o_pay:])
                offs.append(s.offs[j])
                rows.append(d[self.o_qrow:self.o_qrow + 4 * eng.nby].view(torch.int32) if has_rows else None)
                maps.append(d[self.o_qmap:self.o_qmap + 4 * nb].view(torch.int32) if has_map else None)
                if chroma:
                    self._offsets(d[self.o_clens:self.o_clens + 2 * nb].view(torch.int16), s.coffs[j])
                    cpacked.append(d[self.o_pay + _a16(nl):])
                    coffs.append(s.coffs[j])
            outs = [self.planes[p] for p in ps]
            types = [u[1] for u in unit]
            one = ctypes.c_void_p * 1
            if types[0] == 0:                              # an I-frame is a unit of its own
                name = "so_unpack_frames" + suffix
                rc = getattr(lib, name)(1, (ctypes.c_int32 * 1)(0), one(packed[0].data_ptr()), one(offs[0].data_ptr()),
                                        nb, eng.bs, one(self.d_split.data_ptr()), one(self.d_mv.data_ptr()),
                                        one(self.d_qtc.data_ptr()), s.err[0].data_ptr(), sh)
                _lib.check(rc, name)
                rc = lib.so_intra_recon_ex(eng.h, eng.w, eng.bs, int(self.dec.Qp), _lib.ptr(rows[0]), _lib.ptr(maps[0]),
                                           self.d_split.data_ptr(), self.d_mv.data_ptr(), self.d_qtc.data_ptr(),
                                           outs[0].data_ptr(), eng.scratch.data_ptr(), sh)
                _lib.check(rc, "so_intra_recon_ex")
                state["refs"] = [outs[0]]
            elif self.fme or not fused:                    # P-frames off the dense set, one by one
                name = "so_unpack_frames" + suffix
                for j in range(n):
                    rc = getattr(lib, name)(1, (ctypes.c_int32 * 1)(1), one(packed[j].data_ptr()),
                                            one(offs[j].data_ptr()), nb, eng.bs, one(self.d_split.data_ptr()),
                                            one(self.d_mv.data_ptr()), one(self.d_qtc.data_ptr()),
                                            s.err[0, j:].data_ptr(), sh)
                    _lib.check(rc, name)
                    refs = state["refs"]
                    rc = lib.so_inter_recon_ex(_lib.ref_array(refs), len(refs), eng.h, eng.w, eng.bs, int(self.dec.Qp),
                                               _lib.ptr(rows[j]), _lib.ptr(maps[j]), int(self.fme), 1,
                                               _lib.ptr(self.fme_ws), self.d_split.data_ptr(), self.d_mv.data_ptr(),
                                               self.d_qtc.data_ptr(), outs[j].data_ptr(), sh)
                    _lib.check(rc, "so_inter_recon_ex")
                    state["refs"] = (refs + [outs[j]])[-self.nref:]
                    if chroma and fused:                   # while the dense set holds this frame's motion
                        self._fused_chroma(s, j, [1], cpacked[j:j + 1], coffs[j:j + 1], [self.d_split], [self.d_mv],
                                           rows[j:j + 1], maps[j:j + 1], ps[j:j + 1], hdr, state, coding)
                    elif chroma:
                        self._dense_chroma(s, j, 1, cpacked[j], coffs[j], rows[j], maps[j], ps[j], hdr, state, suffix, sh)
                    if self.deblock:                       # before the next unpack overwrites the flags
                        self._deblock(s, j, outs[j:j + 1], ps[j:j + 1], [self.d_split], rows[j:j + 1],
                                      maps[j:j + 1], chroma, hdr)
            else:
                # While the list is short (after an I-frame, nRefFrames > 1) a stream of this
                # project's encoder can name a reference past it: the encoder keeps its list across
                # an I-frame, the decoder clears it (decoder.py), and so_inter_recon_ex resolves such
                # an index to the list's first plane.  Those frames go one per call with the list
                # written out that way, so decode_packed_file's frames come back and the fused
                # kernel's index check still holds against nRefFrames.
                refs, j = state["refs"], 0
                while j < n and len(refs) < self.nref:
                    eng.decode_p_frames(packed[j:j + 1], offs[j:j + 1], refs + [refs[0]] * (self.nref - len(refs)),
                                        self.nref, int(self.dec.Qp), rows[j:j + 1], maps[j:j + 1], coding=coding,
                                        out_split=[self.split[j]], out_mv=[self.mv[j]], out_recon=outs[j:j + 1],
                                        err=s.err[0, j:])
                    refs = (refs + [outs[j]])[-self.nref:]
                    j += 1
                if j < n:
                    eng.decode_p_frames(packed[j:], offs[j:], refs, self.nref, int(self.dec.Qp), rows[j:], maps[j:],
                                        coding=coding, out_split=list(self.split[j:n]), out_mv=list(self.mv[j:n]),
                                        out_recon=outs[j:], err=s.err[0, j:])
                    refs = (refs + outs[j:])[-self.nref:]
                state["refs"] = refs
            if chroma and not fused:
                if types[0] == 0:
                    self._dense_chroma(s, 0, 0, cpacked[0], coffs[0], rows[0], maps[0], ps[0], hdr, state, suffix, sh)
            elif chroma and types[0] == 0:
                state["refs_u"], state["refs_v"] = [], []
                self._fused_chroma(s, 0, types, cpacked, coffs, [None] * n, [None] * n, rows, maps, ps, hdr, state,
                                   coding)
            elif chroma and not self.fme:                  # under FME every frame went with its luma above
                self._fused_chroma(s, 0, types, cpacked, coffs, list(self.split[:n]), list(self.mv[:n]), rows, maps,
                                   ps, hdr, state, coding)
            src_uv = [self.cplanes[p] for p in ps] if chroma else None
            if self.deblock:
                if types[0] == 0:                          # the dense set still holds the I-frame's flags
                    self._deblock(s, 0, outs, ps, [self.d_split], rows, maps, chroma, hdr)
                elif fused and not self.fme:               # the fused P-frames' flags: one launch for the unit
                    self._deblock(s, 0, outs, ps, list(self.split[:n]), rows, maps, chroma, hdr)
                outs, src_uv = s.db_y[:n], (s.db_uv[:n] if chroma else None)
            if self.out_hw:
                eng.scale_yuv420(outs, src_uv, self.scale_plan,
                                 src_hw=self.scale_plan.src_hw, out_y=s.sy_d[:n],
                                 out_uv=s.suv_d[:n] if chroma else None, out_hw=self.out_hw)
                if self.output == "rgb":
                    eng.yuv420_to_rgb(s.sy_d[:n], s.suv_d[:n], *self.out_hw, self.colour, out=s.rgb_d[:n],
                                      plane_hw=self.out_hw)
            elif self.output == "rgb":
                eng.yuv420_to_rgb(outs, src_uv, self.dec.h_pixels, self.dec.w_pixels,
                                  self.colour, out=s.rgb_d[:n])
            done = torch.cuda.Event()
            done.record(comp)
        with torch.cuda.stream(self.d2h):
            self.d2h.wait_event(done)
            if self.output == "rgb":
                s.rgb_h[:n].copy_(s.rgb_d[:n], non_blocking=True)
            elif self.out_hw:
                s.y_h[:n].copy_(s.sy_d[:n], non_blocking=True)
                if chroma:
                    s.uv_h[:n].copy_(s.suv_d[:n], non_blocking=True)
            else:
                for j, p in enumerate(ps):
                    s.y_h[j].copy_(outs[j], non_blocking=True)
                    if chroma:
                        s.uv_h[j].copy_(src_uv[j], non_blocking=True)
            self.err_h[k].copy_(s.err, non_blocking=True)
            s.down = torch.cuda.Event()
            s.down.record(self.d2h)
        for p in ps:
            self.plane_ev[p] = s.down

    def _deblock(self, s, j0, planes, ps, split, rows, maps, chroma, hdr) -> None:
        """The reconstructions `planes` (ring planes ps) of frames j0.. of the unit through
        so_deblock_yuv420 into the set's display planes, one launch on the compute stream."""
        n = len(planes)
        self.eng.deblock_yuv420(planes, [self.cplanes[p] for p in ps] if chroma else None,
                                split=split if self.eng.bs == 16 else None, qp=int(self.dec.Qp), qp_rows=rows,
                                qp_maps=maps, chroma_qp_offset=int(hdr["chroma_qp_offset"]) if chroma else 0,
                                strength=self.deblock_strength, out_y=s.db_y[j0:j0 + n],
                                out_uv=s.db_uv[j0:j0 + n] if chroma else None)

    def _fused_chroma(self, s, j0, types, cpacked, coffs, split, mv, rows, maps, ps, hdr, state, coding) -> None:
        """Frames j0.. of the unit through so_decode_chroma_frames (_ex under FME: Engine picks it),
        their error words from s.err[1, j0]."""
        cu, cv = [self.cplanes[p, 0] for p in ps], [self.cplanes[p, 1] for p in ps]
        self.eng.decode_chroma_frames(types, cpacked, coffs, split, mv, state["refs_u"], state["refs_v"], self.nref,
                                      int(self.dec.Qp), int(hdr["chroma_qp_offset"]), rows, maps, coding=coding,
                                      out_u=cu, out_v=cv, err=s.err[1, j0:])
        state["refs_u"] = (state["refs_u"] + cu)[-self.nref:]
        state["refs_v"] = (state["refs_v"] + cv)[-self.nref:]

    def _dense_chroma(self, s, j, ft, cpacked, coffs, rows, maps, p, hdr, state, suffix, sh) -> None:
        """Frame j of the unit through so_unpack_chroma_frames(_bits, _huff) + so_chroma_recon_frame,
        the luma motion taken from the dense set (fused=False, and every "huff" file)."""
        eng, lib, one = self.eng, self.eng.lib, ctypes.c_void_p * 1
        if self.d_qc is None:                              # a fused decoder's first "huff" file
            self.d_qc = torch.empty((2, eng.nb, 64), dtype=torch.int16, device=self.dev)
        name = "so_unpack_chroma_frames" + suffix
        rc = getattr(lib, name)(1, one(cpacked.data_ptr()), one(coffs.data_ptr()), eng.nb, one(self.d_qc[0].data_ptr()),
                                one(self.d_qc[1].data_ptr()), s.err[1, j:].data_ptr(), sh)
        _lib.check(rc, name)
        if ft == 0:
            state["refs_u"], state["refs_v"] = [], []
        ru, rv = state["refs_u"], state["refs_v"]
        args = (_lib.ref_array(ru) if ft else None, _lib.ref_array(rv) if ft else None, len(ru), eng.h, eng.w, eng.bs,
                ft, self.d_split.data_ptr() if ft else None, self.d_mv.data_ptr() if ft else None, int(self.dec.Qp),
                _lib.ptr(rows), _lib.ptr(maps), int(hdr["chroma_qp_offset"]), self.d_qc[0].data_ptr(),
                self.d_qc[1].data_ptr(), self.cplanes[p, 0].data_ptr(), self.cplanes[p, 1].data_ptr())
        if self.subpel:
            _lib.check(lib.so_chroma_recon_frame_ex(*args, 2, sh), "so_chroma_recon_frame_ex")
        else:
            _lib.check(lib.so_chroma_recon_frame(*args, sh), "so_chroma_recon_frame")
        state["refs_u"] = (ru + [self.cplanes[p, 0]])[-self.nref:]
        state["refs_v"] = (rv + [self.cplanes[p, 1]])[-self.nref:]

    def _retire(self, s: _Set, k: int, hdr: dict, consume) -> None:
        """Wait for the unit in set s and hand its frames on, in order; a malformed record raises
        once the frames before it are delivered."""
        s.down.synchronize()
        hp, wp = self.out_hw or (self.dec.h_pixels, self.dec.w_pixels)
        err = self.err_h[k].numpy()
        unit, s.frames = s.frames, []
        for j, (i, _, _, _, _, _) in enumerate(unit):
            if err[0, j] or err[1, j]:
                what, bad = ("luma", err[0, j]) if err[0, j] else ("chroma", err[1, j])
                raise ValueError(f"frame {i}: malformed packed {what} stream at block {int(bad) - 1}")
            if self.output == "rgb":
                consume(i, s.rgb_h[j].numpy())
                continue
            y = s.y_h[j].numpy()[:hp, :wp]
            u = v = None
            if hdr["chroma"]:
                uv = s.uv_h[j].numpy()
                u, v = uv[0, :hp // 2, :wp // 2], uv[1, :hp // 2, :wp // 2]
            consume(i, y, u, v)

    # ---- the interface -----------------------------------------------------------------------------
    def decode_file(self, path: str, consume) -> dict:
        """Decode the container at `path`; consume(i, y, u, v) is called for every frame in order
        with host uint8 arrays cropped to the picture (u, v None for a luma-only file), valid
        inside the call.  With output="rgb" it is consume(i, rgb), rgb a host uint8 [h, w, 3]
        array, and a luma-only file raises ValueError before any frame is queued.  Returns
        {"frames", "frame_type", "coding", "layout"}.  A malformed file or record raises ValueError
        after every earlier frame has been delivered; no later frame is delivered."""
        eng = self.eng
        hdr, frames = packedfile.open_frames(path)
        try:
            if (hdr["h"], hdr["w"], hdr["bs"], hdr["nb"]) != (eng.h, eng.w, eng.bs, eng.nb):
                raise ValueError(f"{path}: {hdr['w']}x{hdr['h']} bs {hdr['bs']} does not match this decoder")
            if self.output == "rgb" and not hdr["chroma"]:
                raise ValueError(f"{path}: a luma-only file has no chroma to make RGB from (output=\"rgb\")")
            if hdr["chroma"] and self.fme and not self.subpel:
                raise NotImplementedError("chroma with FMEEnable is not built")
            if hdr["chroma"] and eng.bs != 16:
                raise NotImplementedError("chroma needs block_size 16")
            state = {"refs": [self.ref128], "next_plane": 0}
            if hdr["chroma"]:
                state["refs_u"], state["refs_v"] = [self.c128], [self.c128]
            self.plane_ev = [None] * self.nring
            caller = torch.cuda.current_stream(self.dev)
            self.comp.wait_stream(caller)
            types, pending, failed = [], [], None
            k, cur = 0, None          # the unit being gathered: its number and its set

            def free(s):
                while any(p[0] is s for p in pending):
                    ps, pk = pending.pop(0)
                    self._retire(ps, pk, hdr, consume)

            def flush():
                nonlocal k, cur
                if cur is not None and cur.frames:
                    self._queue(cur, k % self.nbuf, hdr, state)
                    pending.append((cur, k % self.nbuf))
                    k += 1
                    while len(pending) > self.nbuf - 1:
                        ps, pk = pending.pop(0)
                        self._retire(ps, pk, hdr, consume)
                cur = None

            it, i = iter(frames), 0
            while True:
                try:
                    rec = next(it)
                except StopIteration:
                    break
                except ValueError as e:
                    failed = e
                    break
                if rec["frame_type"] == 0 or (cur is not None and cur.frames[0][1] == 0):
                    flush()
                if cur is None:
                    cur = self.sets[k % self.nbuf]
                    free(cur)
                try:
                    cur.frames.append(self._stage(cur, len(cur.frames), i, rec, hdr))
                except ValueError as e:
                    failed = e
                    break
                types.append(rec["frame_type"])
                i += 1
                if len(cur.frames) == self.chunk or rec["frame_type"] == 0:
                    flush()
            flush()
            while pending:
                ps, pk = pending.pop(0)
                self._retire(ps, pk, hdr, consume)
            if failed is not None:
                raise failed
            return {"frames": i, "frame_type": types, "coding": hdr["coding"], "layout": hdr["layout"]}
        finally:
            frames.close()
            for st in (self.h2d, self.comp, self.d2h):     # nothing in flight, whatever happened
                st.synchronize()
            for s in self.sets:
                s.frames = []

    def decode_to_yuv(self, path: str, out_path: str) -> dict:
        """The decoded frames as a planar file, Y | U | V per frame at picture size (Y alone for a
        luma-only file): decoder.save_yuv420's / save_decoded_frames' bytes."""
        if self.output == "rgb":
            raise ValueError("decode_to_yuv needs output=\"yuv420\" (this decoder delivers RGB: decode_to_rgb)")
        with open(out_path, "wb") as f:
            def consume(i, y, u, v):
                f.write(np.ascontiguousarray(y).tobytes())
                if u is not None:
                    f.write(np.ascontiguousarray(u).tobytes())
                    f.write(np.ascontiguousarray(v).tobytes())
            return self.decode_file(path, consume)

    def decode_to_rgb(self, path: str, out_path: str) -> dict:
        """The decoded frames as raw RGB24 at picture size, frame after frame (output="rgb")."""
        if self.output != "rgb":
            raise ValueError("decode_to_rgb needs a decoder built with output=\"rgb\"")
        with open(out_path, "wb") as f:
            return self.decode_file(path, lambda i, rgb: f.write(rgb.tobytes()))
