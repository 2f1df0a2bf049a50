"""Host-to-host GOP encode with the transfers overlapped (BASELINE.md §4's timed region:
pinned host Y planes in, symbols out).

The reference reads frames from host memory and writes its bitstream text to files
(Encoder.py:1790-1898, transmit_bitstream :1544-1580).  Here the three engines of the card
work at once:

    copy stream A (H2D)   frame 0 | frames 1..C | frames C+1..2C | ... | next GOP's frames ...
    compute stream        I-frame | P-run 1..C (+ pack) | P-run C+1..2C (+ pack) | ...
    copy stream B (D2H)                  packed chunk 0 | packed chunk 1 | ...

A P-run chunk waits for its frames' upload events only; the packed symbol stream of a chunk
(Engine.pack_symbols: varint split / MVs / RLE token lists, 2.4x smaller than the int16
QTC) is downloaded as soon as its byte counts are known, while the next chunk encodes.
The host waits for a chunk's byte counts only after it has enqueued the following chunk, so
the compute stream never idles on the host.  Symbols are those of encode_device (the chunks
are persistent P-runs with the previous chunk's reconstruction as their reference).

encode_stream() runs several GOPs back to back with two sets of frame / packed buffers: the
next GOP's upload is queued before the current GOP encodes, so the H2D engine never waits for
the compute stream (a GOP then costs about its upload time).

With input="rgb" the host hands over 8-bit RGB pictures at picture size instead of padded planes:
copy stream A uploads a unit's pictures and converts them right behind the copy (so_rgb_to_yuv420)
into the same device planes, inside the unit's upload event; everything after that is unchanged.

With source_size=(hs, ws) the host hands over pictures of another size than the one that is coded:
a unit's planes (or RGB pictures, converted at source size) land in staging planes of that size and
copy stream A resamples them (so_scale_yuv420) into the same device planes, again inside the unit's
upload event.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from .engine import alloc_planes
from .hostmem import device_ptr, pinned_empty
from .hwqueue import dedicated_stream


class _Buffers:
    """One GOP in flight: device frames, packed streams and their pinned host copies."""

    def __init__(self, eng, nframes: int, dev, chroma: bool = False, lengths: bool = False, rgb_hw=None,
                 src_hw=None, coding: str = "varint"):
        nb, F = eng.nb, nframes
        self.frames_dev = alloc_planes(F, eng.h, eng.w, dev)
        # source_size: where a unit's planes land at source size before so_scale_yuv420 writes frames_dev / uv_dev
        self.src_y = self.src_uv = None
        if src_hw:
            self.src_y = torch.empty((F, *src_hw), dtype=torch.uint8, device=dev)
            if chroma:
                self.src_uv = torch.empty((F, 2, src_hw[0] // 2, src_hw[1] // 2), dtype=torch.uint8, device=dev)
        # input="rgb": where a unit's pictures land before so_rgb_to_yuv420 writes frames_dev / uv_dev
        self.rgb_dev = torch.empty((F, *rgb_hw, 3), dtype=torch.uint8, device=dev) if rgb_hw else None
        self.offs = torch.empty((F, nb + 1), dtype=torch.int32, device=dev)
        # a row: luma, then chroma, by the coding's bounds
        cap = eng.pack_bound(coding=coding) + (eng.pack_chroma_bound(coding) if chroma else 0)
        self.packed = torch.empty((F, cap), dtype=torch.uint8, device=dev)
        self.packed_h = pinned_empty(tuple(self.packed.shape))
        # the small host arrays in one page-locked slab (an allocation there is 2 MB at least):
        # int64 sse [F] | int64 chroma sums [F, 4] | int32 luma lengths [F] | int32 combined lengths [F]
        slab = pinned_empty((F * (8 + 32 + 4 + 4),))
        self.sse_h = slab[:8 * F].view(torch.int64)
        self.csum_h = slab[8 * F:40 * F].view(torch.int64).view(F, 4)
        self.tot_h = slab[40 * F:44 * F].view(torch.int32)
        self.all_h = slab[44 * F:48 * F].view(torch.int32)
        # the packs' last passes store each frame's length here: luma's into tot_h
        # (so_pack_frames_ex), luma + chroma into all_h (so_pack_chroma_frames_after)
        self.tot_dptr = device_ptr(slab) + 40 * F
        self.all_dptr = device_ptr(slab) + 44 * F
        self.len_h = self.all_h if chroma else self.tot_h     # what a frame's download copies
        if chroma:
            self.uv_dev = alloc_planes(F * 2, eng.h // 2, eng.w // 2, dev).view(F, 2, eng.h // 2, eng.w // 2)
            self.coffs = torch.empty((F, nb + 1), dtype=torch.int32, device=dev)
        if lengths:
            # per-block byte counts: diff(offs) on the compute stream (a block is at most 1725 bytes
            # in any coding, a chroma record 979), row 0 luma, row 1 chroma, and their host copy
            k = 2 if chroma else 1
            self.diff32 = torch.empty((k, F, nb), dtype=torch.int32, device=dev)
            self.blen = torch.empty((k, F, nb), dtype=torch.int16, device=dev)
            self.blen_h = pinned_empty((k, F, nb), torch.int16)
        self.enc_done = None      # compute-stream event: this set's frames are no longer read
        self.d2h_done = None      # D2H-stream event: this set's packed streams are downloaded
        self.gop = None           # (index, frame types) of the GOP it holds


class _PackedViews:
    """Frame i's packed stream as packed_h[i, :bytes[i]], made when asked for."""

    def __init__(self, packed_h, nbytes):
        self._p, self._n = packed_h, nbytes

    def __len__(self):
        return len(self._n)

    def __getitem__(self, i):
        return self._p[i, :self._n[i]]

    def __iter__(self):
        return (self[i] for i in range(len(self._n)))


class HostStreamEncoder:
    def __init__(self, codec, nframes: int, chunk: int = 2, nbuf: int = 1, upload: str = "chunk",
                 lengths: bool = False, input: str = "yuv420", source_size=None, scale: str = "lanczos3",
                 coding: str = "varint"):
        """coding: the packed stream's coding, "varint", "bits" or "huff" (Engine.pack_symbols); the
        buffers are sized by its bounds and write_packed writes its version word.
        upload: "chunk" = one H2D copy per encode unit (the I-frame, each P-run chunk), "frame"
        = one per frame.  lengths: the results also hold each frame's per-block byte counts
        ("block_bytes", and "chroma_block_bytes" with a chroma=True codec), which write_packed needs.
        input: "yuv420" = padded Y (and UV) planes from the host; "rgb" (chroma=True codecs) = pinned
        uint8 [F, h, w, 3] pictures at picture size, no padding on the host: each unit's pictures are
        uploaded as they are and converted behind the copy on the H2D stream (so_rgb_to_yuv420 with the
        codec's `colour`) into the same device planes, before the unit's event is recorded.
        source_size: (hs, ws) = the host's pictures have this size, not the coded one: unpadded pinned
        uint8 [F, hs, ws] planes (with a chroma=True codec uv [F, 2, hs/2, ws/2]) or [F, hs, ws, 3] RGB
        pictures, uploaded into staging planes per buffer set and resampled behind the copy on the H2D
        stream (so_scale_yuv420 with the `scale` filter: "bilinear", "bicubic" or "lanczos3") to the
        codec's h_pixels x w_pixels, padded with 128.  None: nothing is staged and nothing resampled."""
        from .engine import pack_coding_suffix
        pack_coding_suffix(coding)                         # refuses an unknown coding
        self.coding = coding
        if input not in ("yuv420", "rgb"):
            raise ValueError(f"input {input!r} (\"yuv420\" or \"rgb\")")
        if input == "rgb" and not codec.chroma:
            raise ValueError("input=\"rgb\" needs a chroma=True codec (RGB for a luma-only codec is not built)")
        self.input = input
        self.scale_plan = host_plan = None
        if source_size is not None:
            from . import scale as _scale
            # every refusal (sizes, filter, a ratio beyond the tap bound) before a buffer is allocated
            host_plan = (_scale.check_size(source_size, "source_size", bool(codec.chroma)),
                         _scale.check_size((codec.h_pixels, codec.w_pixels), "the coded picture", bool(codec.chroma)),
                         _scale.check_filter(scale))
            _scale.ScalePlan.check(*host_plan, chroma=bool(codec.chroma))
        eng = codec.engine()
        self.codec, self.eng, self.nframes, self.chunk = codec, eng, int(nframes), int(chunk)
        if upload not in ("chunk", "frame"):
            raise ValueError("upload must be 'chunk' or 'frame'")
        self.upload = upload
        self.dev = codec.device
        # the three engines' streams each on a hardware queue of its own (hwqueue.py): on a
        # shared queue a stream's event wait stalls the others and the region runs serially
        self.h2d = dedicated_stream(self.dev, "hoststream.h2d")
        self.d2h = dedicated_stream(self.dev, "hoststream.d2h")
        self.comp = dedicated_stream(self.dev, "hoststream.compute")
        self.syms = None
        self.chroma, self.lengths = bool(codec.chroma), bool(lengths)
        # like the luma symbols, one set of ChromaSymbols serves every buffer set: the compute
        # stream packs a GOP's symbols before the next GOP's work overwrites them
        self.csyms = [eng.new_chroma_symbols() for _ in range(self.nframes)] if self.chroma else None
        self.src_hw = host_plan[0] if host_plan else None
        self.rgb_hw = (self.src_hw or (int(codec.h_pixels), int(codec.w_pixels))) if input == "rgb" else None
        if host_plan:
            self.scale_plan = _scale.ScalePlan(*host_plan, chroma=self.chroma, device=self.dev)
        self.bufs = [_Buffers(eng, self.nframes, self.dev, self.chroma, self.lengths, self.rgb_hw, self.src_hw,
                              self.coding)
                     for _ in range(max(1, int(nbuf)))]

    @property
    def frames_dev(self):
        return self.bufs[0].frames_dev

    def _check(self, frames_host):
        if self.input == "rgb":
            shape = tuple(self.bufs[0].rgb_dev.shape)
            if (not isinstance(frames_host, torch.Tensor) or frames_host.dtype != torch.uint8
                    or tuple(frames_host.shape) != shape or not frames_host.is_contiguous() or not frames_host.is_pinned()):
                raise ValueError(f"input=\"rgb\": frames must be pinned contiguous uint8 {list(shape)} (picture size)")
            return
        if self.src_hw:
            shape = tuple(self.bufs[0].src_y.shape)
            if (not isinstance(frames_host, torch.Tensor) or frames_host.dtype != torch.uint8
                    or tuple(frames_host.shape) != shape or not frames_host.is_contiguous() or not frames_host.is_pinned()):
                raise ValueError(f"source_size: frames must be pinned contiguous uint8 {list(shape)} (source size, unpadded)")
            return
        if tuple(frames_host.shape) != tuple(self.bufs[0].frames_dev.shape) or not frames_host.is_pinned():
            raise ValueError("frames_host must be pinned uint8 of the encoder's padded frame shape")

    def _check_uv(self, uv_gops, ngops: int) -> list:
        """One pinned uint8 [F, 2, Hp/2, Wp/2] per GOP with a chroma=True codec, none otherwise."""
        if self.input == "rgb":
            if uv_gops is not None:
                raise ValueError("uv planes were given, but input=\"rgb\" makes them from the RGB pictures")
            return [None] * ngops
        if not self.chroma:
            if uv_gops is not None:
                raise ValueError("uv planes were given, but the codec was built with chroma=False")
            return [None] * ngops
        shape = tuple((self.bufs[0].src_uv if self.src_hw else self.bufs[0].uv_dev).shape)
        if uv_gops is None or len(uv_gops) != ngops:
            raise ValueError(f"a chroma=True codec needs uv planes: one pinned uint8 {list(shape)} tensor per GOP")
        for uv in uv_gops:
            if (not isinstance(uv, torch.Tensor) or uv.dtype != torch.uint8 or tuple(uv.shape) != shape
                    or not uv.is_contiguous() or not uv.is_pinned()):
                raise ValueError(f"uv planes must be pinned contiguous uint8 {list(shape)} "
                                 f"({'source size, unpadded' if self.src_hw else 'padded with 128'})")
        return list(uv_gops)

    def _units(self, intra_dur: int) -> list:
        """The frame ranges encode_device works on in turn: each I-frame, and the P-runs of at
        most `chunk` frames between them."""
        r, i = [], 0
        while i < self.nframes:
            j = i + 1
            if i % intra_dur != 0:
                while j < self.nframes and j % intra_dur != 0 and j - i < self.chunk:
                    j += 1
            r.append((i, j))
            i = j
        return r

    def _upload(self, b: _Buffers, frames_host, intra_dur: int, uv_host=None) -> list:
        """Queue the GOP's upload; returns per frame the event after the copy that carries it
        (one copy per encode unit: 16.6 MB copies ran at 52.6 GB/s, 8.3 MB ones at 50.0 on the
        GPU box, tools/s4_links.py).  A unit's U and V planes follow its Y planes, inside the
        same event."""
        up = [None] * self.nframes
        units = self._units(intra_dur) if self.upload == "chunk" else [(i, i + 1) for i in range(self.nframes)]
        with torch.cuda.stream(self.h2d):
            if b.enc_done is not None:
                self.h2d.wait_event(b.enc_done)      # the GOP that last used these frames is encoded
            for k0, k1 in units:
                # with source_size the unit lands in the staging planes and is resampled below
                y_to, uv_to = (b.src_y, b.src_uv) if self.src_hw else (b.frames_dev, getattr(b, "uv_dev", None))
                if self.input == "rgb":
                    b.rgb_dev[k0:k1].copy_(frames_host[k0:k1], non_blocking=True)
                    self.eng.rgb_to_yuv420(b.rgb_dev[k0:k1], self.codec.colour, out_y=y_to[k0:k1],
                                           out_uv=uv_to[k0:k1], plane_hw=self.src_hw)
                else:
                    y_to[k0:k1].copy_(frames_host[k0:k1], non_blocking=True)
                if uv_host is not None:
                    uv_to[k0:k1].copy_(uv_host[k0:k1], non_blocking=True)
                if self.src_hw:
                    self.eng.scale_yuv420(y_to[k0:k1], uv_to[k0:k1] if self.chroma else None, self.scale_plan,
                                          out_y=b.frames_dev[k0:k1], out_uv=b.uv_dev[k0:k1] if self.chroma else None)
                ev = torch.cuda.Event()
                ev.record(self.h2d)
                up[k0:k1] = [ev] * (k1 - k0)
        return up

    def _result(self, b: _Buffers) -> dict:
        nbytes = b.len_h.tolist()
        res = {"packed": _PackedViews(b.packed_h, nbytes), "bytes": nbytes,
               "sse": b.sse_h.clone(), "frame_type": b.gop[1]}
        if self.chroma:
            res["luma_bytes"] = b.tot_h.tolist()
            res["chroma_sse"] = b.csum_h[:, :2].clone()
            res["chroma_tokens"] = b.csum_h[:, 2:].clone()
        if self.lengths:
            lens = b.blen_h.numpy().view(np.uint16)
            res["block_bytes"] = lens[0]
            if self.chroma:
                res["chroma_block_bytes"] = lens[1]
        return res

    def encode(self, frames_host: torch.Tensor, intra_dur: int, uv_host: torch.Tensor | None = None) -> dict:
        """frames_host: pinned uint8 [F, Hp, Wp] (input="rgb": [F, h, w, 3] at picture size, and no
        uv_host).  Returns {"packed": [host uint8 view per
        frame], "bytes": [...], "sse": host int64 [F], "frame_type": [...]} once everything
        is in host memory (the views stay valid until the next call).
        With a chroma=True codec, uv_host: pinned uint8 [F, 2, Hp/2, Wp/2], padded with 128
        (Y_Video_codec._upload_uv_padded's layout); "packed"[i] is then frame i's luma stream
        followed by its chroma stream, "bytes" the combined length, and the result also holds
        "luma_bytes" (where to split) and "chroma_sse" / "chroma_tokens", host int64 [F, 2] (U, V).
        With lengths=True: "block_bytes" and, with chroma, "chroma_block_bytes", host uint16 [F, nb]."""
        out = []
        self.encode_stream([frames_host], intra_dur, lambda k, r: out.append(r),
                           uv_gops=None if uv_host is None else [uv_host])
        return out[0]

    def write_packed(self, path: str, result: dict, qp_rows: list | None = None) -> int:
        """A result of an encoder built with lengths=True as a packed container
        (packedfile.write_frames; decoder.decode_packed_file reads it): the file
        transmit_packed / transmit_packed420 writes for the same GOP.  qp_rows: the frames'
        per-row QPs under rate control (encode_device's "qp_rows").  Returns the file size."""
        from . import packedfile
        if "block_bytes" not in result:
            raise ValueError("write_packed needs the per-block lengths: build the encoder with lengths=True")
        if (self.codec.RCFlag is not None and self.codec.RCFlag >= 3) or self.codec.roi_block_offsets() is not None:
            raise NotImplementedError("write_packed: the stream does not download per-block QP maps (ROI / two-pass RC)")
        frames = []
        for i, ft in enumerate(result["frame_type"]):
            p = result["packed"][i].numpy()
            f = {"frame_type": ft, "qp_rows": qp_rows[i] if qp_rows else [], "block_bytes": result["block_bytes"][i]}
            if self.chroma:
                n = result["luma_bytes"][i]
                f.update(payload=p[:n], chroma_payload=p[n:], chroma_block_bytes=result["chroma_block_bytes"][i])
            else:
                f["payload"] = p
            frames.append(f)
        return packedfile.write_frames(path, self.eng.h, self.eng.w, self.eng.bs, self.eng.nb, self.coding, frames,
                                       chroma_qp_offset=self.codec.chroma_qp_offset if self.chroma else None)

    def encode_stream(self, gops: list, intra_dur: int, consume, trace: list | None = None,
                      uv_gops: list | None = None) -> None:
        """Encode GOPs back to back; consume(k, result) is called for GOP k, in order, once its
        symbols are in host memory and before its buffers are reused (the result's views are
        valid only inside the call).  With two buffer sets (nbuf=2) GOP k+1's upload runs
        during GOP k's encode.  uv_gops: with a chroma=True codec, each GOP's chroma planes
        (encode's uv_host)."""
        for g in gops:
            self._check(g)
        uv_gops = self._check_uv(uv_gops, len(gops))
        caller = torch.cuda.current_stream(self.dev)
        self.comp.wait_stream(caller)       # the caller's earlier work on the inputs / buffers
        with torch.cuda.stream(self.comp):
            self._encode_stream(gops, intra_dur, consume, trace, uv_gops)

    def _encode_stream(self, gops: list, intra_dur: int, consume, trace, uv_gops) -> None:
        eng, comp, nb = self.eng, self.comp, len(self.bufs)
        if self.syms is None:
            self.syms = [eng.new_symbols(0 if i % intra_dur == 0 else 1) for i in range(self.nframes)]
        pending, waiting = [], []      # chunks whose byte counts are on their way; finished GOPs

        def mark(label, stream):       # tools/stream_probe.py: (label, event, host time)
            if trace is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(stream)
                trace.append((label, ev, time.perf_counter()))

        def drain(upto_len):
            while len(pending) > upto_len:
                b, k0, k1, ev = pending.pop(0)
                ev.synchronize()                    # byte counts of frames [k0, k1) are in len_h
                self.d2h.wait_event(ev)
                mark(f"d2h_go {k0}", self.d2h)
                with torch.cuda.stream(self.d2h):
                    for i in range(k0, k1):
                        n = int(b.len_h[i])
                        b.packed_h[i, :n].copy_(b.packed[i, :n], non_blocking=True)
                    if self.lengths:
                        for r in range(b.blen.shape[0]):     # contiguous rows: plain async copies
                            b.blen_h[r, k0:k1].copy_(b.blen[r, k0:k1], non_blocking=True)
                if k1 == self.nframes:              # the GOP's last chunk: its download is queued
                    b.d2h_done = torch.cuda.Event()
                    b.d2h_done.record(self.d2h)
                    mark(f"d2h_end {b.gop[0] if b.gop else '?'}", self.d2h)

        def retire(b):
            """Hand GOP b.gop to the caller (its chunks all drained) and free the set."""
            if any(p[0] is b for p in pending):
                drain(0)
            while waiting and waiting[0] is b:
                waiting.pop(0)
                b.enc_done.synchronize()            # its SSE copy (compute stream)
                b.d2h_done.synchronize()            # its packed streams (D2H stream)
                consume(b.gop[0], self._result(b))
                b.gop = None

        ups = {}
        for k, g in enumerate(gops):
            b = self.bufs[k % nb]
            if b.gop is not None:
                retire(b)                            # GOP k - nb: long finished when nb > 1
            if k == 0 or nb == 1:
                ups[k] = self._upload(b, g, intra_dur, uv_gops[k])
                mark(f"up_end {k}", self.h2d)
            if nb > 1 and k + 1 < len(gops):       # the next GOP's upload, queued before this encode
                ups[k + 1] = self._upload(self.bufs[(k + 1) % nb], gops[k + 1], intra_dur, uv_gops[k + 1])
                mark(f"up_end {k + 1}", self.h2d)
            up = ups.pop(k)
            if b.d2h_done is not None:
                comp.wait_event(b.d2h_done)         # this set's previous packed streams are down
            b.gop = (k, None)
            mark(f"enc_start {k}", comp)

            def wait_input(k0, k1, up=up):
                comp.wait_event(up[k1 - 1])
                mark(f"chunk_go {k0}", comp)

            def on_output(k0, k1, syms, csyms=None, b=b):
                # the scan stores the frames' lengths straight into tot_h (so_pack_frames_ex)
                eng.pack_symbols(syms, b.offs[k0:k1], b.packed[k0:k1], totals_ptr=b.tot_dptr + 4 * k0,
                                 coding=self.coding)
                if csyms is not None:
                    # the chroma records behind each frame's luma bytes, the combined lengths into all_h
                    eng.pack_chroma_symbols(csyms, b.coffs[k0:k1], b.packed[k0:k1], after=b.offs[k0:k1],
                                            totals_ptr=b.all_dptr + 4 * k0, coding=self.coding)
                if self.lengths:
                    for r, o in enumerate((b.offs, b.coffs) if csyms is not None else (b.offs,)):
                        torch.sub(o[k0:k1, 1:], o[k0:k1, :-1], out=b.diff32[r, k0:k1])
                        b.blen[r, k0:k1].copy_(b.diff32[r, k0:k1])
                ev = torch.cuda.Event()
                ev.record(comp)
                mark(f"chunk_end {k0}", comp)
                pending.append((b, k0, k1, ev))
                drain(1)                             # the chunk before this one

            res = self.codec.encode_device(b.frames_dev, intra_dur, symbols=self.syms, check=False,
                                           chunk=self.chunk, wait_input=wait_input, on_output=on_output,
                                           **({"uv_dev": b.uv_dev, "chroma_symbols": self.csyms} if self.chroma else {}))
            b.sse_h.copy_(res["sse"], non_blocking=True)
            if self.chroma:
                b.csum_h.copy_(res["chroma_sums"], non_blocking=True)
            b.enc_done = torch.cuda.Event()
            b.enc_done.record(comp)
            mark(f"enc_end {k}", comp)
            b.gop = (k, res["frame_type"])
            waiting.append(b)
        drain(0)
        for b in list(waiting):
            retire(b)
        comp.synchronize()
        eng.check_run(defer_stats=True)
