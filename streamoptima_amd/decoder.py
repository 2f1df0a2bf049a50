"""Drop-in `decoder` (the reference's decoder.py surface) on the MI355X path.

decode() reconstructs frames from symbols with the same gfx950 kernels as the encoder's
reconstruction (decoder.py:97-211 inter, :330-432 intra mode 0, :487-545 GOP loop incl.
its reference-list handling: an I-frame CLEARS the list, decoder.py:520).  With
FMEEnable the references are the frac frames (decoder.py:102-103, 468-483); after the
I-frame reset the list holds uint8 reconstructions only, so their row sums always wrap.
"""
from __future__ import annotations

import numpy as np
import torch

from . import bitstream as _bs
from .bitstream import entropy_encoder_block  # noqa: F401  (API parity helpers live there)
from .engine import Engine, FrameSymbols, alloc_planes


def _canon_frame(frame_type, mvs, residuals, bs):
    """reference per-block lists -> canonical arrays (split, mv, qtc)."""
    nb = len(mvs)
    split = np.zeros(nb, np.uint8)
    qtc = np.zeros((nb, bs * bs), np.int16)
    mv = np.zeros((nb, 4, 3) if frame_type == 1 else (nb, 4), np.int16)
    sb2 = (bs // 2) ** 2
    for i, (m, r) in enumerate(zip(mvs, residuals)):
        if m[0] == 0:
            mv[i, 0] = m[1]
            qtc[i] = np.asarray(r[1]).reshape(-1)
        else:
            split[i] = 1
            for j in range(4):
                mv[i, j] = m[1][j]
                qtc[i, j * sb2:(j + 1) * sb2] = np.asarray(r[1][j]).reshape(-1)
    return split, mv, qtc


class decoder:
    def __init__(self, intra_mode, intra_dur, block_size, frames, height, width, Qp, nRefFrames, FMEEnable, lam,
                 VBSEnable, VBSoverlay=None, RCFlag=None, targetBR=None, frame_rate=30, qp_rate_tables=None,
                 ParallelMode=0, device=None, chroma_subpel=False, deblock=False, deblock_strength=0):
        self.intra_mode = intra_mode
        self.intra_dur = intra_dur
        self.block_size = block_size
        self.sub_block_size = block_size // 2
        self.frames = frames
        self.h_pixels = height
        self.w_pixels = width
        self.num_blocks_per_row = width / block_size
        self.decoded_vid = None
        self.decoded_vid_f = False
        self.Qp = Qp
        self.nRefFrames = nRefFrames
        self.FMEEnable = FMEEnable
        # build extension: with FMEEnable, read the half-sample luma vectors as quarter-sample chroma
        # vectors (DESIGN.md "Chroma with FMEEnable").  Like FMEEnable itself the precision is not in any
        # file: it is this argument, and it must be what the encoder was given
        self.chroma_subpel = bool(chroma_subpel)
        # build extension: the display-side deblocking post-filter (DESIGN.md "Deblocking").  The frames
        # every decode call returns and saves are filtered; the references stay the raw reconstructions,
        # so the stream decodes as it always did.  deblock_strength (-3..3) shifts the filter's QP
        if int(deblock_strength) < -3 or int(deblock_strength) > 3:
            raise ValueError(f"deblock_strength {deblock_strength} outside [-3, 3]")
        if deblock and block_size not in (8, 16):
            raise NotImplementedError("deblock needs block_size 8 or 16")
        self.deblock = bool(deblock)
        self.deblock_strength = int(deblock_strength)
        self.lam = lam
        self.VBSEnable = VBSEnable
        self.VBSoverlay = VBSoverlay
        self.RCFlag = RCFlag
        self.frame_rate = frame_rate
        self.qr_rate_tables = qp_rate_tables
        self.ParallelMode = ParallelMode
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self._engine = None
        self.decoded_chroma = None          # [(U, V)] host planes of decode_chroma
        self.decoded_chroma_device = None   # [(U, V)] device planes of decode_symbols

    def _eng(self, engine=None) -> Engine:
        if engine is not None:
            return engine
        bs = self.block_size
        hp = -(-self.h_pixels // bs) * bs
        wp = -(-self.w_pixels // bs) * bs
        if self._engine is None:
            self._engine = Engine(hp, wp, bs, 16, False, 0.0, self.device, fme=bool(self.FMEEnable),
                                  chroma_subpel=self.chroma_subpel)
        return self._engine

    def _rc(self):
        return self.RCFlag is not None and self.RCFlag > 0

    def _chroma_loop(self, eng, syms, qtcs, qp_offset):
        """The chroma GOP loop: per frame (U, V) device planes from the luma symbols `syms` and
        the coefficients qtcs[i] = (qtc_u, qtc_v).  The reference list follows the luma one's
        handling below (one all-128 plane at first, cleared by an I-frame)."""
        c128 = alloc_planes(1, eng.h // 2, eng.w // 2, eng.device, fill=128)[0]
        refs_u, refs_v = [c128], [c128]
        out = []
        n = len(syms)
        for i, (s, (qu, qv)) in enumerate(zip(syms, qtcs)):
            if s.frame_type == 0:
                refs_u, refs_v = [], []
            c = eng.recon_chroma(s, qu, qv, refs_u, refs_v, qp_offset)
            out.append((c.recon_u, c.recon_v))
            if i < n - 1:
                if len(refs_u) >= self.nRefFrames:
                    refs_u.pop(0)
                    refs_v.pop(0)
                refs_u.append(c.recon_u)
                refs_v.append(c.recon_v)
        return out

    def _deblock_frames(self, eng, planes, splits, qp_rows, qp_maps, chroma=None, qp_offset=0):
        """The display frames of a decoded sequence: one so_deblock_yuv420 launch over the luma planes
        and, with `chroma` ([(U, V)] device planes), U and V.  The sources stay as they are (they are
        the references).  Returns ([y], [(u, v)] or None)."""
        n = len(planes)
        if eng.bs == 8:
            splits = None    # no VBS at block size 8: the flags are all zero, and the filter refuses them
        rows = [r if (self._rc() and r is not None and len(r)) else None for r in qp_rows]
        ys, uvs = eng.deblock_yuv420(planes, chroma, split=splits, qp=self.Qp, qp_rows=rows, qp_maps=qp_maps,
                                     chroma_qp_offset=int(qp_offset), strength=self.deblock_strength)
        return [ys[i] for i in range(n)], (None if chroma is None else [(uvs[i, 0], uvs[i, 1]) for i in range(n)])

    def decode_symbols(self, symbols, engine=None, chroma_symbols=None):
        """GOP decode straight from device symbols (the encoder's closed loop).  With
        chroma_symbols (the encoder's ChromaSymbols per frame) U and V are rebuilt too, into
        self.decoded_chroma_device; the return value stays the luma planes.  With deblock=True
        both are the filtered display frames (the reference lists keep the raw reconstructions)."""
        eng = self._eng(engine)
        out = self._decode_symbols(symbols, eng, chroma_symbols)
        if self.deblock and out:
            qo = chroma_symbols[0].qp_offset if chroma_symbols else 0
            out, c = self._deblock_frames(eng, out, [s.split for s in symbols], [s.qp_row for s in symbols],
                                          [s.extra.get("qp_map") for s in symbols],
                                          self.decoded_chroma_device if chroma_symbols is not None else None, qo)
            if c is not None:
                self.decoded_chroma_device = c
        return out

    def _decode_symbols(self, symbols, eng, chroma_symbols=None):
        if chroma_symbols is not None:
            lum = [FrameSymbols(s.frame_type, s.split, s.mv, None, None, None, None, qp_rd=self.Qp,
                                qp_row=s.qp_row if self._rc() else None,
                                extra={"qp_map": s.extra["qp_map"]} if "qp_map" in s.extra else {})
                   for s in symbols]
            self.decoded_chroma_device = self._chroma_loop(
                eng, lum, [(c.qtc_u, c.qtc_v) for c in chroma_symbols],
                chroma_symbols[0].qp_offset if chroma_symbols else 0)
        ref_frames = [alloc_planes(1, eng.h, eng.w, eng.device, fill=128)[0]]
        out = []
        n = len(symbols)
        for i, s in enumerate(symbols):
            qp_row = s.qp_row if self._rc() else None
            qm = s.extra.get("qp_map")      # ROI / two-pass per-block QP (build extension)
            if s.frame_type == 0:
                rec = eng.recon_intra(s.split, s.mv, s.qtc, self.Qp, qp_row, qp_map_dev=qm)
                ref_frames = []
            else:
                rec = eng.recon_inter(ref_frames, s.split, s.mv, s.qtc, self.Qp, qp_row, qp_map_dev=qm)
            out.append(rec)
            if i < n - 1:
                if len(ref_frames) >= self.nRefFrames:
                    ref_frames.pop(0)
                ref_frames.append(rec)
        return out

    def decode(self, frame_type_seq, residual_file, Qp_per_row_per_frame, mv_file, intra_mode=None, intra_dur=None,
               block_size=None, frames=None, width=None, height=None, save_decoded_frames=True, qp_maps=None,
               _filter=True):
        """decoder.py:487-545 with the per-frame lists of the encoded package.  qp_maps: per
        frame per-block QPs (ROI / two-pass RC build extension) or None.  With deblock=True the raw
        planes and their split flags and QPs are kept for decode_chroma, whose launch filters Y, U and
        V together (_filter=False, decode_bitstream's: this call then leaves the filtering to it)."""
        bs = block_size or self.block_size
        frames = frames or self.frames
        eng = self._eng()
        ref_frames = [alloc_planes(1, eng.h, eng.w, eng.device, fill=128)[0]]
        decoded, side = [], []
        for i in range(frames):
            ft = frame_type_seq[i]
            split, mv, qtc = _canon_frame(ft, mv_file[i], residual_file[i], bs)
            split_d = torch.from_numpy(split).to(eng.device)
            mv_d = torch.from_numpy(mv).to(eng.device)
            qtc_d = torch.from_numpy(qtc).to(eng.device)
            qp_row = Qp_per_row_per_frame[i] if self._rc() else None
            qm = None
            if qp_maps is not None and qp_maps[i] is not None:
                qm = torch.as_tensor(np.asarray(qp_maps[i], np.int32)).to(eng.device)
            if ft == 0:
                rec = eng.recon_intra(split_d, mv_d, qtc_d, self.Qp, qp_row, qp_map_dev=qm)
                ref_frames = []
            else:
                rec = eng.recon_inter(ref_frames, split_d, mv_d, qtc_d, self.Qp, qp_row, qp_map_dev=qm)
            decoded.append(rec)
            side.append((split_d, qp_row, qm))
            if i < frames - 1:
                if len(ref_frames) >= self.nRefFrames:
                    ref_frames.pop(0)
                ref_frames.append(rec)
        self._raw_luma = (decoded, side) if self.deblock else None
        if self.deblock and decoded and _filter:
            decoded, _ = self._deblock_frames(eng, decoded, [t[0] for t in side], [t[1] for t in side],
                                              [t[2] for t in side])
        host = [d.cpu().numpy()[: self.h_pixels, : self.w_pixels] for d in decoded]
        if save_decoded_frames:
            self.decoded_vid_f = True
            self.decoded_vid = host
        return host

    def decode_chroma(self, frame_type_seq, mv_file, chroma_residuals, Qp_per_row_per_frame, qp_maps=None,
                      chroma_qp_offset=0):
        """U and V of every frame from the package's per-frame lists: mv_file as decode() takes
        it (the luma motion), chroma_residuals[i] = (qtc_u, qtc_v) as int16 [nb, 64] arrays or the
        package's "chroma approx residual" entry.  Returns per-frame (U, V) cropped to the picture.
        With deblock=True the filter's one launch covers Y, U and V, so decode() of the same frames
        comes first (it keeps the raw luma planes); the filtered luma of that launch is kept in
        self._display_luma (device planes)."""
        if self.FMEEnable and not self.chroma_subpel:
            raise NotImplementedError("chroma with FMEEnable is not built")
        if self.block_size != 16:
            raise NotImplementedError("chroma needs block_size 16")
        raw = getattr(self, "_raw_luma", None)
        if self.deblock and (raw is None or len(raw[0]) != len(frame_type_seq)):
            raise ValueError("decode_chroma with deblock=True filters U and V in one launch with the luma planes "
                             "decode() keeps: call decode() on the same frames first")
        eng = self._eng()
        syms, qtcs = [], []
        for i, ft in enumerate(frame_type_seq):
            nb = len(mv_file[i])
            split_d = mv_d = None
            if ft == 1:
                split = np.zeros(nb, np.uint8)
                mv = np.zeros((nb, 4, 3), np.int16)
                for b, m in enumerate(mv_file[i]):
                    if m[0] == 0:
                        mv[b, 0] = m[1]
                    else:
                        split[b] = 1
                        mv[b] = m[1]
                split_d = torch.from_numpy(split).to(eng.device)
                mv_d = torch.from_numpy(mv).to(eng.device)
            extra = {}
            if qp_maps is not None and qp_maps[i] is not None:
                extra["qp_map"] = torch.as_tensor(np.asarray(qp_maps[i], np.int32)).to(eng.device)
            syms.append(FrameSymbols(ft, split_d, mv_d, None, None, None, None, qp_rd=self.Qp,
                                     qp_row=list(Qp_per_row_per_frame[i]) if self._rc() else None, extra=extra))
            pair = []
            for q in chroma_residuals[i]:
                if isinstance(q, list):   # the package's [(0, QTC 8 x 8)] per block
                    q = np.stack([np.asarray(b) for _, b in q])
                pair.append(torch.from_numpy(np.ascontiguousarray(np.asarray(q).reshape(nb, 64).astype(np.int16)))
                            .to(eng.device))
            qtcs.append(tuple(pair))
        dev = self._chroma_loop(eng, syms, qtcs, int(chroma_qp_offset))
        if self.deblock and dev:
            planes, side = raw
            self._display_luma, dev = self._deblock_frames(eng, planes, [t[0] for t in side], [t[1] for t in side],
                                                           [t[2] for t in side], dev, int(chroma_qp_offset))
        h2, w2 = self.h_pixels // 2, self.w_pixels // 2
        self.decoded_chroma = [(u.cpu().numpy()[:h2, :w2], v.cpu().numpy()[:h2, :w2]) for u, v in dev]
        return self.decoded_chroma

    def save_yuv420(self, filename):
        """The decoded frames as a planar 4:2:0 file (Y | U | V per frame, picture size): needs
        decode() / decode_bitstream() with chroma."""
        if not self.decoded_vid_f or self.decoded_chroma is None:
            raise ValueError("save_yuv420 needs decoded luma and chroma frames")
        with open(filename, "wb") as f:
            for y, (u, v) in zip(self.decoded_vid, self.decoded_chroma):
                f.write(np.ascontiguousarray(y).tobytes())
                f.write(np.ascontiguousarray(u).tobytes())
                f.write(np.ascontiguousarray(v).tobytes())

    # ---- text bitstream (decoder.py:547-710) ----------------------------------------------
    def entropy_decoder_block(self, encoded_block, block_size):
        return _bs.entropy_decoder_block(encoded_block, block_size)

    def differential_decoder_frame(self, mv_for_frame):
        return _bs.differential_decoder_frame(mv_for_frame, self.RCFlag, self.num_blocks_per_row)

    def entropy_decoder_frame(self, residual_for_frame, block_size):
        return _bs.entropy_decoder_frame(residual_for_frame, block_size)

    def decode_differential_entropy(self, all_mv_f, all_residual_f, block_size):
        """decoder.py:666-684: the two text files -> per-frame symbol lists."""
        frame_type_seq, mv_for_vid, qp_for_vid, res_for_vid = [], [], [], []
        with open(all_mv_f) as f:
            for line in f:
                ft, mvs, qps = self.differential_decoder_frame(line)
                frame_type_seq.append(ft)
                mv_for_vid.append(mvs)
                qp_for_vid.append(qps)
        with open(all_residual_f) as f:
            for line in f:
                res_for_vid.append(self.entropy_decoder_frame(line, block_size))
        return frame_type_seq, mv_for_vid, qp_for_vid, res_for_vid

    def decode_bitstream(self, mv_file, residual_file, intra_mode=None, intra_dur=None, block_size=None, frames=None,
                         width=None, height=None, save_decoded_frames=True, qp_map_file=None,
                         chroma_residual_file=None, chroma_qp_offset=0):
        """decoder.py:686-709: parse the transmitted text bitstream (transmit_bitstream)
        on the host, reconstruct every frame on the GPU.  qp_map_file: the per-block QP
        lines of ROI / two-pass RC (build extension).  chroma_residual_file: the chroma lines
        of transmit_bitstream; U and V are then rebuilt too (self.decoded_chroma, save_yuv420)."""
        bs = block_size or self.block_size
        ft, mvs, qps, res = self.decode_differential_entropy(mv_file, residual_file, bs)
        self.mv_per_frame = mvs
        self.residuals_per_frame = res
        maps = None
        if qp_map_file is not None:
            with open(qp_map_file) as f:
                maps = [(_bs.parse_qp_map_line(line, qps[i] if self._rc() else None, self.Qp, self.num_blocks_per_row)
                         if line.strip() else None) for i, line in enumerate(f)]
        chroma = chroma_residual_file is not None
        host = self.decode(ft, res, qps, mvs, intra_mode, intra_dur, bs, frames, width, height, save_decoded_frames,
                           qp_maps=maps, _filter=not chroma)     # with chroma one launch filters Y, U and V below
        if chroma_residual_file is not None:
            with open(chroma_residual_file) as f:
                cres = [_bs.parse_chroma_residual_line(line) for line in f if line.strip()]
            n = len(host)
            self.decode_chroma(ft[:n], mvs[:n], cres[:n], qps[:n], qp_maps=maps, chroma_qp_offset=chroma_qp_offset)
            if self.deblock and n:
                host = [d.cpu().numpy()[: self.h_pixels, : self.w_pixels] for d in self._display_luma]
                if save_decoded_frames:
                    self.decoded_vid = host
        return host

    def decode_packed_file(self, path: str, save_decoded_frames=True):
        """Encoder.transmit_packed's or transmit_packed420's file (packedfile.py, both layouts): the
        packed streams go to the GPU, so_unpack_frames (or so_unpack_frames_bits / _huff, by the file's
        coding) restores split / mv / qtc of every block in parallel, and the frames are rebuilt
        by the same kernels as decode().  Per-block QP maps in the file are applied.  With chroma
        in the file so_unpack_chroma_frames (_bits, _huff) restores the coefficients and U and V are
        rebuilt too (self.decoded_chroma, save_yuv420)."""
        from . import packedfile
        eng = self._eng()
        meta = packedfile.read(path, eng.device)
        if (meta["h"], meta["w"], meta["bs"], meta["nb"]) != (eng.h, eng.w, eng.bs, eng.nb):
            raise ValueError(f"{path}: {meta['w']}x{meta['h']} bs {meta['bs']} does not match this decoder")
        chroma = meta["chroma_packed"] is not None
        if chroma and self.FMEEnable and not self.chroma_subpel:
            raise NotImplementedError("chroma with FMEEnable is not built")
        if chroma and self.block_size != 16:
            raise NotImplementedError("chroma needs block_size 16")
        syms = eng.unpack_symbols(meta["frame_types"], meta["packed"], meta["offs"], coding=meta["coding"])
        for s, q in zip(syms, meta["qp_rows"]):
            s.qp_row = q or None
        for s, m in zip(syms, meta["qp_maps"] or []):
            if m is not None:
                s.extra["qp_map"] = m
        if chroma:
            qtcs = eng.unpack_chroma_symbols(meta["chroma_packed"], meta["chroma_offs"], coding=meta["coding"])
            lum = [FrameSymbols(s.frame_type, s.split, s.mv, None, None, None, None, qp_rd=self.Qp,
                                qp_row=s.qp_row if self._rc() else None,
                                extra={"qp_map": s.extra["qp_map"]} if "qp_map" in s.extra else {}) for s in syms]
            dev = self._chroma_loop(eng, lum, qtcs, int(meta["chroma_qp_offset"]))
        decoded = self._decode_symbols(syms, eng)
        if self.deblock and decoded:
            decoded, fdev = self._deblock_frames(eng, decoded, [s.split for s in syms], [s.qp_row for s in syms],
                                                 [s.extra.get("qp_map") for s in syms], dev if chroma else None,
                                                 int(meta["chroma_qp_offset"]) if chroma else 0)
            dev = fdev if chroma else None
        if chroma:
            h2, w2 = self.h_pixels // 2, self.w_pixels // 2
            self.decoded_chroma_device = dev
            self.decoded_chroma = [(u.cpu().numpy()[:h2, :w2], v.cpu().numpy()[:h2, :w2]) for u, v in dev]
        host = [d.cpu().numpy()[: self.h_pixels, : self.w_pixels] for d in decoded]
        if save_decoded_frames:
            self.decoded_vid_f = True
            self.decoded_vid = host
        return host

    def decode_packed_stream(self, path: str, out_path: str | None = None, consume=None, chunk: int = 2,
                             nbuf: int = 2, output: str = "yuv420", colour=None, output_size=None,
                             scale: str = "lanczos3", deblock=None, deblock_strength=None) -> dict:
        """decode_packed_file's frames without its footprint (hostdecode.HostStreamDecoder): the file
        is read as it goes, P-frames and chroma are decoded from the packed records straight to
        pixels (so_decode_p_frames, so_decode_chroma_frames; a "huff" file through the unpack and
        reconstruction entry points instead), and upload, decode and download overlap
        with a fixed set of buffers whatever the file's length.  out_path: write the frames as a
        planar file (Y | U | V per frame; Y alone for a luma-only file) -- save_yuv420's /
        save_decoded_frames' bytes.  consume(i, y, u, v): called per frame in order with host arrays
        cropped to the picture, valid inside the call.  One of the two.  output="rgb" (with `colour`,
        a colour.Colour; None: BT.601, full range) converts every frame on the device: the file is
        then raw RGB24 and the call consume(i, rgb) with rgb [h, w, 3]; a luma-only file raises
        ValueError.  output_size=(ho, wo) resamples every frame on the device to that size (`scale`:
        "bilinear", "bicubic" or "lanczos3") before it is converted or downloaded; the frames, the
        file and the arrays consume receives then have that size.  deblock / deblock_strength: the
        deblocking post-filter for this stream (None: this decoder's own setting); the frames are
        filtered on the device before they are resampled, converted or downloaded.  The stream decoder
        is kept with this instance.  Returns {"frames",
        "frame_type", "coding", "layout"}."""
        from .colour import as_colour
        from .hostdecode import HostStreamDecoder
        if (out_path is None) == (consume is None):
            raise ValueError("decode_packed_stream: give out_path or consume")
        deblock = self.deblock if deblock is None else bool(deblock)
        strength = self.deblock_strength if deblock_strength is None else int(deblock_strength)
        key = (int(chunk), int(nbuf), output, as_colour(colour), None if output_size is None else tuple(output_size),
               scale, deblock, strength)
        if getattr(self, "_stream_dec", None) is None or self._stream_dec[0] != key:
            self._stream_dec = (key, HostStreamDecoder(self, chunk=chunk, nbuf=nbuf, output=output, colour=colour,
                                                       output_size=output_size, scale=scale, deblock=deblock,
                                                       deblock_strength=strength))
        hs = self._stream_dec[1]
        if out_path is None:
            return hs.decode_file(path, consume)
        return hs.decode_to_rgb(path, out_path) if output == "rgb" else hs.decode_to_yuv(path, out_path)

    def decode_to_rgb(self, path: str, out_path: str, colour=None, chunk: int = 2, nbuf: int = 2, output_size=None,
                      scale: str = "lanczos3", deblock=None, deblock_strength=None) -> dict:
        """The packed file at `path` as raw RGB24 at picture size (or at output_size), frame after
        frame: decode_packed_stream with output="rgb"."""
        return self.decode_packed_stream(path, out_path=out_path, chunk=chunk, nbuf=nbuf, output="rgb", colour=colour,
                                         output_size=output_size, scale=scale, deblock=deblock,
                                         deblock_strength=deblock_strength)

    def save_decoded_frames(self, filename="yuv/decoded_bitstream_frames.yuv"):
        if not self.decoded_vid_f:
            print("[ERROR] No decoded frames available.")
            return
        with open(filename, "wb") as f:
            for data in self.decoded_vid:
                f.write(data.tobytes())
