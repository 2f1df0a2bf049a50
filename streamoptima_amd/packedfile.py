"""A binary container for the packed symbol stream (so_pack_frames) -- the compact counterpart of
the reference's two text files (transmit_bitstream, Encoder.py:1544-1573; decode_bitstream,
decoder.py:686-709).  Little endian.  The version word is layout << 16 | coding: coding 1 is the
varint coding of the streams (so_pack_frames, so_pack_chroma_frames), coding 2 the "bits" coding
(so_pack_frames_bits, so_pack_chroma_frames_bits), coding 3 the "huff" coding (so_pack_frames_huff,
so_pack_chroma_frames_huff), whose per-frame Huffman tables are the first bytes of block 0 (chroma
record 0) and are counted in its length: a "huff" frame whose first block is shorter than its
tables (323 bytes, chroma 301) is rejected like lengths that do not add up.

Layout 0 (version 1, 2 or 3): luma only, no per-block QP maps.

    header   b"SOPK" | u32 version | u32 H | u32 W | u32 bs | u32 nframes | u32 nb
    frame    u8 frame_type | u16 nqp | i8 qp[nqp] (per-row QPs under rate control, else 0)
             | u32 nbytes | u16 block_bytes[nb] | bytes[nbytes]

Layout 1: what layout 0 cannot carry -- chroma 4:2:0 and the per-block QP maps of ROI / two-pass
rate control.

    header   b"SOPK" | u32 (1 << 16 | coding) | u32 H | u32 W | u32 bs | u32 nframes | u32 nb
             | u32 flags (bit 0: chroma, bit 1: QP maps; any other bit set is rejected)
             | i32 chroma_qp_offset
    frame    the layout-0 frame record
             | if flags & 2:  u8 has_map | u8 qp_map[nb] when has_map     (absolute per-block QPs)
             | if flags & 1:  u32 cbytes | u16 cblock_bytes[nb] | bytes[cbytes]

block_bytes (cblock_bytes) lets the GPU decoder (so_unpack_frames, so_unpack_chroma_frames) start
every block (chroma record) in parallel: the offsets are their exclusive prefix sums.  The
writer (write_frames: host data in; write packs device symbols and calls it) picks layout 0
whenever it can, so a luma-only GOP without QP maps gives the file it always gave.

The precision of the motion vectors is not in the file: like FMEEnable itself (half-sample luma
vectors), which the reference's decoder takes as a constructor argument, it belongs to the
decoder.  That holds for chroma under FMEEnable too: a file written by a codec with
chroma_subpel=True has the same layout 1 as any other, and is read by a decoder built with
FMEEnable=True and chroma_subpel=True; one built without chroma_subpel refuses it.
"""
from __future__ import annotations

import struct

import numpy as np
import torch

MAGIC = b"SOPK"
VERSIONS = {"varint": 1, "bits": 2, "huff": 3}   # the stream's coding -> the version word's low half
HUFF_TABLE_BYTES = {"block": 323, "chroma record": 301}   # at the head of a "huff" frame's first block / record
FLAG_CHROMA, FLAG_QP_MAPS = 1, 2


def _section(lens, payload, nb: int, what: str) -> bytes:
    """u32 nbytes | u16 lengths[nb] | bytes: one frame's luma blocks or chroma records."""
    lens = np.asarray(lens).reshape(-1)
    data = payload if isinstance(payload, (bytes, bytearray)) else np.ascontiguousarray(
        np.asarray(payload, dtype=np.uint8)).tobytes()
    if lens.size != nb:
        raise ValueError(f"{what}: {lens.size} lengths for {nb} blocks")
    if lens.size and (int(lens.min()) < 0 or int(lens.max()) > 0xFFFF):
        raise ValueError(f"{what}: a length does not fit a u16")
    if int(lens.astype(np.int64).sum()) != len(data):
        raise ValueError(f"{what}: the lengths add up to {int(lens.astype(np.int64).sum())}, the payload has "
                         f"{len(data)} bytes")
    return struct.pack("<I", len(data)) + lens.astype("<u2").tobytes() + data


def write_frames(path: str, h: int, w: int, bs: int, nb: int, coding: str, frames: list,
                 chroma_qp_offset: int | None = None) -> int:
    """Write the container from host data; returns its size.  frames: one dict per frame with
    "frame_type", "qp_rows" (the per-row QPs under rate control, else empty), "block_bytes" ([nb]
    lengths) and "payload" (the frame's packed luma bytes); optionally "qp_map" ([nb] absolute QPs
    in 0..255, or None); optionally "chroma_block_bytes" and "chroma_payload", for all frames or
    for none.  chroma_qp_offset goes into the header of a file with chroma.  Layout 0 when no frame
    has chroma or a QP map, else layout 1.  This is the one statement of the format's write side."""
    if coding not in VERSIONS:
        raise ValueError(f"packed stream coding {coding!r} (\"varint\", \"bits\" or \"huff\")")
    has_c = ["chroma_payload" in f or "chroma_block_bytes" in f for f in frames]
    if any(has_c) and not all("chroma_payload" in f and "chroma_block_bytes" in f for f in frames):
        raise ValueError("chroma_block_bytes and chroma_payload: both, and for every frame or for none")
    maps_h = []
    for i, f in enumerate(frames):
        m = f.get("qp_map")
        m = None if m is None else np.asarray(m).astype(np.int64).reshape(-1)
        if m is not None and (m.size != nb or int(m.min()) < 0 or int(m.max()) > 255):
            raise ValueError(f"frame {i}: the QP map must hold {nb} QPs in 0..255")
        maps_h.append(m)
    flags = (FLAG_CHROMA if any(has_c) else 0) | (FLAG_QP_MAPS if any(m is not None for m in maps_h) else 0)
    hdr = MAGIC + struct.pack("<6I", (1 << 16 if flags else 0) | VERSIONS[coding], h, w, bs, len(frames), nb)
    if flags:
        hdr += struct.pack("<Ii", flags, int(chroma_qp_offset or 0) if flags & FLAG_CHROMA else 0)
    recs = []
    for i, f in enumerate(frames):
        q = list(f.get("qp_rows") or [])
        rec = (struct.pack("<BH", int(f["frame_type"]), len(q)) + np.asarray(q, np.int8).tobytes()
               + _section(f["block_bytes"], f["payload"], nb, f"frame {i}"))
        if flags & FLAG_QP_MAPS:
            m = maps_h[i]
            rec += b"\0" if m is None else b"\1" + m.astype(np.uint8).tobytes()
        if flags & FLAG_CHROMA:
            rec += _section(f["chroma_block_bytes"], f["chroma_payload"], nb, f"frame {i} chroma")
        recs.append(rec)
    with open(path, "wb") as fh:        # nothing is written when an input is refused
        fh.write(hdr)
        for rec in recs:
            fh.write(rec)
    return len(hdr) + sum(len(r) for r in recs)


def write(path: str, eng, symbols: list, qp_rows: list | None = None, coding: str = "varint",
          chroma_symbols: list | None = None) -> int:
    """Pack `symbols` (FrameSymbols on the device) in `coding` ("varint", "bits" or "huff") and write the
    container (write_frames); returns its size.  chroma_symbols: the frames' ChromaSymbols, packed
    in the same coding (layout 1).  Per-block QP maps (s.extra["qp_map"]) are written too (layout 1)."""
    if coding not in VERSIONS:
        raise ValueError(f"packed stream coding {coding!r} (\"varint\", \"bits\" or \"huff\")")
    if chroma_symbols is not None and len(chroma_symbols) != len(symbols):
        raise ValueError(f"{len(chroma_symbols)} chroma frames against {len(symbols)} luma frames")

    def host(offs, out):
        offs_h = offs.cpu().numpy().astype(np.int64)
        return [(np.diff(o), out[i, :int(o[-1])].cpu().numpy()) for i, o in enumerate(offs_h)]
    luma = host(*eng.pack_symbols(symbols, coding=coding))
    chroma = host(*eng.pack_chroma_symbols(chroma_symbols, coding=coding)) if chroma_symbols else None
    frames = []
    for i, s in enumerate(symbols):
        m = s.extra.get("qp_map")
        f = {"frame_type": int(s.frame_type), "qp_rows": qp_rows[i] if qp_rows and qp_rows[i] else [],
             "block_bytes": luma[i][0], "payload": luma[i][1], "qp_map": None if m is None else m.cpu().numpy()}
        if chroma is not None:
            f["chroma_block_bytes"], f["chroma_payload"] = chroma[i]
        frames.append(f)
    qp_offset = int(chroma_symbols[0].qp_offset) if chroma_symbols else None
    return write_frames(path, eng.h, eng.w, eng.bs, eng.nb, coding, frames, chroma_qp_offset=qp_offset)


def open_frames(path):
    """The container read as it goes: -> (header, frames).  header: {"h", "w", "bs", "nb", "coding",
    "layout", "nframes", "chroma" (bool), "has_qp_maps" (bool), "chroma_qp_offset" (None without
    chroma)} -- read()'s fields without the per-frame lists.  frames: an iterator of one host record
    per frame, {"frame_type", "qp_rows" (list), "block_bytes" (uint16 [nb]), "payload" (bytes),
    "qp_map" (uint8 [nb] or None), "chroma_block_bytes", "chroma_payload" (None without chroma)}:
    write_frames' input.  Nothing but the current frame's record is held, no read asks for more
    than one section of a frame, and no device is touched.  The ValueErrors are read()'s -- bad
    magic, version or flags here; lengths that do not add up, a file that ends inside a frame and
    bytes after the last frame from the iterator, at the frame where they become visible (the
    last frame is not yielded when bytes follow it).  path: a file name, or an open binary file
    object (which is not closed)."""
    own = not hasattr(path, "read")
    f = open(path, "rb") if own else path
    name = path if own else getattr(path, "name", "<file>")
    try:
        head = f.read(28)
        if head[:4] != MAGIC:
            raise ValueError(f"{name}: not a packed StreamOptima bitstream")
        if len(head) < 28:
            raise ValueError(f"{name}: the file ends inside the header")
        version, h, w, bs, nframes, nb = struct.unpack_from("<6I", head, 4)
        layout = version >> 16
        coding = {v: c for c, v in VERSIONS.items()}.get(version & 0xFFFF)
        if coding is None or layout > 1:
            raise ValueError(f"{name}: container version {version}")
        flags, qp_offset = 0, None
        if layout == 1:
            ext = f.read(8)
            if len(ext) < 8:
                raise ValueError(f"{name}: the file ends inside the header")
            flags, qp_offset = struct.unpack("<Ii", ext)
            if flags & ~(FLAG_CHROMA | FLAG_QP_MAPS):
                raise ValueError(f"{name}: unknown container flags {flags:#x}")
    except BaseException:
        if own:
            f.close()
        raise
    header = {"h": h, "w": w, "bs": bs, "nb": nb, "coding": coding, "layout": layout, "nframes": nframes,
              "chroma": bool(flags & FLAG_CHROMA), "has_qp_maps": bool(flags & FLAG_QP_MAPS),
              "chroma_qp_offset": qp_offset if flags & FLAG_CHROMA else None}

    def take(n: int) -> bytes:
        data = f.read(n) if n else b""
        if len(data) != n:
            raise ValueError(f"{name}: the file ends inside a frame")
        return data

    def section(what: str):
        (nbytes,) = struct.unpack("<I", take(4))
        lens = np.frombuffer(take(2 * nb), np.uint16)
        if int(lens.astype(np.int64).sum()) != nbytes:
            raise ValueError(f"{name}: {what} lengths do not add up to the frame's byte count")
        if coding == "huff" and nb and int(lens[0]) < HUFF_TABLE_BYTES[what]:
            raise ValueError(f"{name}: the first {what} is shorter than the frame's Huffman tables")
        return lens, take(nbytes)

    def frames():
        try:
            for i in range(nframes):
                ft, nqp = struct.unpack("<BH", take(3))
                rec = {"frame_type": int(ft), "qp_rows": np.frombuffer(take(nqp), np.int8).astype(int).tolist()}
                rec["block_bytes"], rec["payload"] = section("block")
                rec["qp_map"] = None
                if flags & FLAG_QP_MAPS:
                    has = take(1)[0]
                    if has > 1:
                        raise ValueError(f"{name}: QP map marker {has}")
                    if has:
                        rec["qp_map"] = np.frombuffer(take(nb), np.uint8)
                rec["chroma_block_bytes"] = rec["chroma_payload"] = None
                if flags & FLAG_CHROMA:
                    rec["chroma_block_bytes"], rec["chroma_payload"] = section("chroma record")
                if i == nframes - 1 and f.read(1):
                    raise ValueError(f"{name}: bytes after the last frame")
                yield rec
            if nframes == 0 and f.read(1):
                raise ValueError(f"{name}: bytes after the last frame")
        finally:
            if own:
                f.close()

    return header, frames()


def read(path: str, device) -> dict:
    """-> {"h", "w", "bs", "nb", "coding", "frame_types", "qp_rows", "packed": [device uint8],
    "offs": [device int32 [nb + 1]], "layout", "qp_maps", "chroma_packed", "chroma_offs",
    "chroma_qp_offset"}.  "coding" is "varint", "bits" or "huff".  In layout 1: "qp_maps" holds per frame
    a device int32 [nb] or None (None itself when the file carries no maps), "chroma_packed" /
    "chroma_offs" the chroma streams like "packed" / "offs" (None without chroma); in layout 0
    all four are None."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != MAGIC:
        raise ValueError(f"{path}: not a packed StreamOptima bitstream")
    version, h, w, bs, nframes, nb = struct.unpack_from("<6I", data, 4)
    layout = version >> 16
    coding = {v: c for c, v in VERSIONS.items()}.get(version & 0xFFFF)
    if coding is None or layout > 1:
        raise ValueError(f"{path}: container version {version}")
    p = 4 + 24
    flags, qp_offset = 0, None
    if layout == 1:
        flags, qp_offset = struct.unpack_from("<Ii", data, p)
        p += 8
        if flags & ~(FLAG_CHROMA | FLAG_QP_MAPS):
            raise ValueError(f"{path}: unknown container flags {flags:#x}")

    def section(p: int, what: str):
        (nbytes,) = struct.unpack_from("<I", data, p)
        p += 4
        lens = np.frombuffer(data, np.uint16, nb, p).astype(np.int64)
        p += 2 * nb
        o = np.zeros(nb + 1, np.int64)
        np.cumsum(lens, out=o[1:])
        if o[-1] != nbytes:
            raise ValueError(f"{path}: {what} lengths do not add up to the frame's byte count")
        if coding == "huff" and nb and int(lens[0]) < HUFF_TABLE_BYTES[what]:
            raise ValueError(f"{path}: the first {what} is shorter than the frame's Huffman tables")
        if p + nbytes > len(data):
            raise ValueError(f"{path}: the file ends inside a frame")
        return (p + nbytes, torch.from_numpy(o.astype(np.int32)).to(device),
                torch.frombuffer(bytearray(data[p:p + nbytes]), dtype=torch.uint8).to(device) if nbytes
                else torch.zeros(0, dtype=torch.uint8, device=device))

    fts, qps, packed, offs, maps, cpacked, coffs = [], [], [], [], [], [], []
    try:
        for _ in range(nframes):
            ft, nqp = struct.unpack_from("<BH", data, p)
            p += 3
            qps.append(np.frombuffer(data, np.int8, nqp, p).astype(int).tolist())
            p += nqp
            p, o, b = section(p, "block")
            fts.append(int(ft))
            offs.append(o)
            packed.append(b)
            if flags & FLAG_QP_MAPS:
                has = data[p]
                p += 1
                if has > 1:
                    raise ValueError(f"{path}: QP map marker {has}")
                maps.append(torch.from_numpy(np.frombuffer(data, np.uint8, nb, p).astype(np.int32)).to(device)
                            if has else None)
                p += nb if has else 0
            if flags & FLAG_CHROMA:
                p, o, b = section(p, "chroma record")
                coffs.append(o)
                cpacked.append(b)
    except (struct.error, IndexError):
        raise ValueError(f"{path}: the file ends inside a frame") from None
    if p != len(data):
        raise ValueError(f"{path}: {len(data) - p} bytes after the last frame")
    return {"h": h, "w": w, "bs": bs, "nb": nb, "coding": coding, "frame_types": fts, "qp_rows": qps, "packed": packed,
            "offs": offs, "layout": layout,
            "qp_maps": maps if flags & FLAG_QP_MAPS else None,
            "chroma_packed": cpacked if flags & FLAG_CHROMA else None,
            "chroma_offs": coffs if flags & FLAG_CHROMA else None,
            "chroma_qp_offset": qp_offset if flags & FLAG_CHROMA else None}
