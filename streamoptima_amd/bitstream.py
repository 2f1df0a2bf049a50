"""Text bitstream of the reference (host-side formatting of the GPU symbols).

  * entropy_encoder_block   — Encoder.py:1086-1131: anti-diagonal scan, RLE tokens
                              (-count, values... for non-zero runs, count for zero runs,
                              a trailing zero run as a single 0).  Values keep the input's
                              element type (np.int64 for the package arrays), so str()
                              of the list matches the reference byte for byte.
  * differential_encoder_frame — Encoder.py:1419-1520 (MV / QP differential line,
                              including the reference's split-under-RC intra quirk).
  * entropy_encoder_frame   — Encoder.py:1522-1542.
  * varints / unpack_frame  — host decoder of the packed symbol stream the GPU writes
                              (so_pack_frames, include/streamoptima.h; format in so_pack.hip).
"""
from __future__ import annotations

import ast
import re
from functools import lru_cache

import numpy as np


@lru_cache(maxsize=8)
def scan_order(n: int) -> np.ndarray:
    """flat indices i*n+j in the order entropy_encoder_block visits them."""
    order = []
    for k in range(2 * n - 1):
        i, j = (0, k) if k < n else (k - n + 1, n - 1)
        while i < n and j >= 0:
            order.append(i * n + j)
            i += 1
            j -= 1
    return np.array(order, dtype=np.int64)


def entropy_encoder_block(residual_block, block_size) -> list:
    arr = np.asarray(residual_block)
    vals = arr.reshape(-1)[scan_order(block_size)] if arr.ndim == 2 else arr.reshape(-1)
    nz = vals != 0
    out = []
    n = len(vals)
    if n == 0:
        return out
    # boundaries of maximal runs
    change = np.flatnonzero(nz[1:] != nz[:-1]) + 1
    starts = np.concatenate(([0], change))
    ends = np.concatenate((change, [n]))
    for s, e in zip(starts.tolist(), ends.tolist()):
        if nz[s]:
            out.append(-(e - s))
            out.extend(vals[s:e])      # numpy scalars, like residual_block[i][j]
        elif e == n:
            out.append(0)
        else:
            out.append(e - s)
    return out


def token_count(residual_block, block_size) -> int:
    vals = np.asarray(residual_block).reshape(-1)
    nz = vals != 0
    return int(nz.sum() + 1 + (nz[1:] != nz[:-1]).sum()) if vals.size else 0


def differential_encoder_frame(frame_type, mv_for_frame, Qp_for_frame, rc_flag, num_blocks_per_row) -> str:
    rc = rc_flag is not None and rc_flag > 0
    parts = []
    ref_qp = 0
    diff_qp = None
    if frame_type == 0:
        ref = 0
        for j, mv in enumerate(mv_for_frame):
            rc_row = rc and j % num_blocks_per_row == 0
            if rc_row:
                diff_qp = Qp_for_frame[int(j // num_blocks_per_row)] - ref_qp
            if mv[0] == 0:
                d = mv[1] - ref
                s = (f"{diff_qp}@0'({d})" if rc_row else f"0'({d})")
                parts.append(s if j == 0 else ";" + s)
                ref = mv[1]
            else:
                for k, sb in enumerate(mv[1]):
                    d = sb - ref
                    if k == 0:
                        parts.append(f";{d}@1'({d}," if rc_row else f";1'({d},")
                    elif k == 3:
                        parts.append(f"{d})")
                    else:
                        parts.append(f"{d},")
                    ref = sb
            if rc_row:
                ref_qp = Qp_for_frame[int(j // num_blocks_per_row)]
    else:
        ref = (0, 0, 0)
        for j, mv in enumerate(mv_for_frame):
            rc_row = rc and j % num_blocks_per_row == 0
            if rc_row:
                diff_qp = Qp_for_frame[int(j // num_blocks_per_row)] - ref_qp
            if mv[0] == 0:
                m = mv[1]
                d = (m[0] - ref[0], m[1] - ref[1], m[2] - ref[2])
                s = (f"{diff_qp}@0'{d}" if rc_row else f"0'{d}")
                parts.append(s if j == 0 else ";" + s)
                ref = m
            else:
                for k, sb in enumerate(mv[1]):
                    d = (sb[0] - ref[0], sb[1] - ref[1], sb[2] - ref[2])
                    if k == 0:
                        parts.append(f";{diff_qp}@1'({d}," if rc_row else f";1'({d},")
                    elif k == 3:
                        parts.append(f"{d})")
                    else:
                        parts.append(f"{d},")
                    ref = sb
            if rc_row:
                ref_qp = Qp_for_frame[int(j // num_blocks_per_row)]
    return "".join(parts)


def entropy_encoder_frame(frame_residuals, block_size) -> str:
    parts = []
    for i, residual in enumerate(frame_residuals):
        if residual[0] == 0:
            s = "0'(" + str(entropy_encoder_block(residual[1], block_size)) + ")"
            parts.append(s if i == 0 else ";" + s)
        else:
            for k, sb in enumerate(residual[1]):
                t = str(entropy_encoder_block(sb, block_size // 2))
                if k == 0:
                    parts.append(";1'(" + t + ",")
                elif k == 3:
                    parts.append(t + ")")
                else:
                    parts.append(t + ",")
    return "".join(parts)


# ---- parsers (decoder.py:547-690) ------------------------------------------------------------
# The reference parses with eval(); the tokens are int / tuple / list literals -- numpy 2
# prints the package's values as np.int64(v) -- so unwrapping those and ast.literal_eval
# read exactly the same values without executing anything.
_NP_SCALAR = re.compile(r"np\.u?int(?:8|16|32|64)\((-?\d+)\)")


def _literal(text: str):
    return ast.literal_eval(_NP_SCALAR.sub(r"\1", text))

def entropy_decoder_block(encoded_block, block_size) -> list:
    """decoder.py:547-586: RLE tokens -> block_size x block_size list of lists (anti-diagonal
    scan; a zero token ends the block, trailing positions stay 0)."""
    arr = []
    i = 0
    while i < len(encoded_block):
        t = encoded_block[i]
        if t < 0:
            arr.extend(encoded_block[i + 1:i + 1 - t])
            i += -t
        else:
            if t == 0:
                break
            arr.extend([0] * t)
        i += 1
    out = np.zeros(block_size * block_size, dtype=int)
    order = scan_order(block_size)
    m = min(len(arr), len(order))
    out[order[:m]] = arr[:m]
    return out.reshape(block_size, block_size).tolist()


def differential_decoder_frame(line: str, rc_flag, num_blocks_per_row):
    """decoder.py:589-644: '<type>|...' -> (frame_type, per-block mvs, per-row QPs)."""
    rc = rc_flag is not None and rc_flag > 0
    raw = line.strip().split("|")
    frame_type = int(raw[0])
    mvs, qps = [], []
    ref_qp = 0
    ref = 0 if frame_type == 0 else (0, 0, 0)
    for j, tok in enumerate(raw[1].split(";")):
        if rc and j % num_blocks_per_row == 0:
            q, tok = tok.split("@")
            ref_qp = ref_qp + int(_literal(q))
            qps.append(ref_qp)
        split, body = tok.split("'")
        v = _literal(body)
        if frame_type == 0:
            if split == "0":
                ref = ref + int(v)
                mvs.append((0, ref))
            else:
                sub = []
                for d in v:
                    ref = ref + d
                    sub.append(ref)
                mvs.append((1, sub))
        else:
            if split == "0":
                ref = (ref[0] + v[0], ref[1] + v[1], ref[2] + v[2])
                mvs.append((0, ref))
            else:
                sub = []
                for d in v:
                    ref = (ref[0] + d[0], ref[1] + d[1], ref[2] + d[2])
                    sub.append(ref)
                mvs.append((1, sub))
    return frame_type, mvs, qps


def entropy_decoder_frame(line: str, block_size) -> list:
    """decoder.py:646-664: residual RLE line -> [(0, QTC) | (1, [QTC x 4])]."""
    out = []
    for tok in line.strip().split(";"):
        split, body = tok.split("'")
        v = _literal(body)
        if split == "0":
            out.append((0, np.array(entropy_decoder_block(v, block_size))))
        else:
            out.append((1, [np.array(entropy_decoder_block(sb, block_size // 2)) for sb in v]))
    return out


# ---- packed symbol stream (so_pack_frames) -----------------------------------------------------
def varints(buf) -> np.ndarray:
    """Zigzag LEB128 varints -> int64 values (vectorised over the whole stream)."""
    b = np.asarray(buf, dtype=np.uint8).reshape(-1)
    if b.size == 0:
        return np.zeros(0, dtype=np.int64)
    ends = np.flatnonzero((b & 0x80) == 0)
    if ends.size == 0 or ends[-1] != b.size - 1:
        raise ValueError("packed stream ends inside a varint")
    starts = np.concatenate(([0], ends[:-1] + 1))
    lens = ends - starts + 1
    if int(lens.max()) > 5:
        raise ValueError("a varint of more than 5 bytes in the packed stream")
    z = np.zeros(ends.size, dtype=np.int64)
    for k in range(int(lens.max())):
        m = lens > k
        z[m] |= (b[starts[m] + k].astype(np.int64) & 0x7F) << (7 * k)
    return (z >> 1) ^ -(z & 1)


def _token_list(order, nn: int, token, coefs, what: str) -> np.ndarray:
    """One (sub-)block's token list read through token() / coefs(n) -> its nn coefficients,
    row-major: "-L" and L values, "Z" zeros, "0" the trailing zeros, the end also at nn."""
    q = np.zeros(nn, dtype=np.int16)
    k = 0
    while k < nn:
        t = token()
        if t < 0:
            if -t > nn - k:
                raise ValueError(f"{what}: a list of {-t} values at position {k} of {nn}")
            q[order[k:k - t]] = coefs(-t)
            k -= t
        elif t == 0:
            break
        else:
            if t > nn - k:
                raise ValueError(f"{what}: a run of {t} zeros at position {k} of {nn}")
            k += t
    return q


class _BitReader:
    """MSB-first reader of the "bits" coding; `stream` names the stream in the error messages."""

    def __init__(self, buf, stream: str):
        self.data = bytes(np.asarray(buf, dtype=np.uint8).reshape(-1))
        self.nbits = 8 * len(self.data)
        self.pos = 0
        self.stream = stream

    def peek(self, n: int) -> int:
        """The next n <= 40 bits (zeros past the end)."""
        by = self.pos >> 3
        w = int.from_bytes(self.data[by:by + 8].ljust(8, b"\0"), "big")
        return (w >> (64 - (self.pos & 7) - n)) & ((1 << n) - 1)

    def take(self, n: int) -> int:
        if self.pos + n > self.nbits:
            raise ValueError(f"{self.stream} ends inside a code")
        v = self.peek(n)
        self.pos += n
        return v

    def ue(self, k: int = 0) -> int:
        """se_k: the signed value of an order-k code."""
        zeros = 17 - self.peek(17).bit_length()       # zeros past the end: caught by take
        if zeros > 16:
            raise ValueError(f"a prefix of more than 16 zero bits in the {self.stream}")
        z = self.take(2 * zeros + 1 + k) - (1 << k)
        if z > 65535:
            raise ValueError(f"a value outside int16 in the {self.stream}")
        return (z >> 1) ^ -(z & 1)

    def pad(self) -> int:
        """The bits up to the next byte boundary (0 when well-formed)."""
        return self.take(-self.pos % 8)

    def left(self) -> int:
        return (self.nbits - self.pos) // 8


def unpack_frame(buf, nb: int, bs: int, frame_type: int) -> dict:
    """One frame's packed stream -> {"split", "mv", "qtc"} in the canonical symbol layout
    (mv entries past the first of an unsplit block are 0).  Raises ValueError on malformed
    input, by the rules of so_unpack_frames (include/streamoptima.h):
      * a varint is 1-5 bytes; a sixth continuation byte, or a varint running off the end of
        the bytes, is malformed;
      * split is 0, or 1 at block size 16; anything else is malformed;
      * every mv value and every coefficient lies in [-32768, 32767], else malformed;
      * a token -L needs 1 <= L <= nn - k, a token Z > 0 needs Z <= nn - k (k: the coefficients
        of the (sub-)block covered so far, nn its size); a token 0 ends the (sub-)block, and a
        list also ends at k == nn;
      * all bytes must be consumed.
    Accepted though not canonical (unambiguous, never written by so_pack_frames): an over-long
    varint of up to 5 bytes whose value fits, a 0 value inside a -L list, a zero run that
    reaches exactly nn written as Z instead of 0.  Block boundaries are not known here, so a
    varint or a list running from one block into the next is seen only where the stream stops
    parsing."""
    va = varints(buf)
    # whatever its role (split, mv, token, coefficient), no value of a well-formed stream
    # leaves int16
    if va.size and (int(va.min()) < -32768 or int(va.max()) > 32767):
        raise ValueError("a value outside int16 in the packed stream")
    v = va.tolist()
    inter = frame_type == 1
    split = np.zeros(nb, dtype=np.uint8)
    mv = np.zeros((nb, 4, 3) if inter else (nb, 4), dtype=np.int16)
    qtc = np.zeros((nb, bs * bs), dtype=np.int16)
    sb = bs // 2
    p = 0

    def take(n: int) -> list:
        nonlocal p
        if p + n > len(v):
            raise IndexError
        p += n
        return v[p - n:p]

    try:
        for b in range(nb):
            sp = take(1)[0]
            if sp != 0 and not (sp == 1 and bs == 16):
                raise ValueError(f"block {b}: split {sp}")
            split[b] = sp
            nmv = (4 if sp else 1) * (3 if inter else 1)
            mv[b].reshape(-1)[:nmv] = take(nmv)
            for n, off in ([(sb, j * sb * sb) for j in range(4)] if sp else [(bs, 0)]):
                qtc[b, off:off + n * n] = _token_list(scan_order(n), n * n, lambda: take(1)[0], take, f"block {b}")
    except IndexError:
        raise ValueError(f"packed stream ends inside block {b}") from None
    if p != len(v):
        raise ValueError(f"{len(v) - p} values after the last block")
    return {"split": split, "mv": mv, "qtc": qtc}


def unpack_frame_bits(buf, nb: int, bs: int, frame_type: int) -> dict:
    """One frame's packed stream in the "bits" coding (so_pack_frames_bits; the format is in
    include/streamoptima.h) -> {"split", "mv", "qtc"} as unpack_frame.  Parses sequentially and
    skips to the next byte boundary after each block, so it needs no offsets.  Raises
    ValueError on malformed input, by the rules of so_unpack_frames_bits: a ue prefix of more
    than 16 zero bits, a decoded z > 65535, a code running past the last byte, split = 1 at
    block size 8, the token rules of unpack_frame, a set pad bit, bytes after the last block."""
    r = _BitReader(buf, "packed stream")
    inter = frame_type == 1
    split = np.zeros(nb, dtype=np.uint8)
    mv = np.zeros((nb, 4, 3) if inter else (nb, 4), dtype=np.int16)
    qtc = np.zeros((nb, bs * bs), dtype=np.int16)
    sb = bs // 2
    for b in range(nb):
        sp, kk = r.take(1), r.take(2)
        if sp and bs != 16:
            raise ValueError(f"block {b}: split at block size {bs}")
        split[b] = sp
        nmv = (4 if sp else 1) * (3 if inter else 1)
        mv[b].reshape(-1)[:nmv] = [r.ue() for _ in range(nmv)]
        coefs = lambda n: [r.ue(kk) for _ in range(n)]   # noqa: E731
        for n, off in ([(sb, j * sb * sb) for j in range(4)] if sp else [(bs, 0)]):
            qtc[b, off:off + n * n] = _token_list(scan_order(n), n * n, r.ue, coefs, f"block {b}")
        if r.pad():
            raise ValueError(f"block {b}: a set bit in the padding")
    if r.left():
        raise ValueError(f"{r.left()} bytes after the last block")
    return {"split": split, "mv": mv, "qtc": qtc}


# ---- packed chroma stream (so_pack_chroma_frames / so_pack_chroma_frames_bits) -------------------
def _chroma_lists(nb: int, token, coefs, start_of_record, end_of_record) -> dict:
    """nb records of two 8x8 token lists (U's, then V's) read through token() / coefs(n);
    start_of_record() runs before U's list, end_of_record(b) after V's."""
    q = np.zeros((2, nb, 64), dtype=np.int16)
    for b in range(nb):
        start_of_record()
        for j in range(2):
            q[j, b] = _token_list(scan_order(8), 64, token, coefs, f"record {b}")
        end_of_record(b)
    return {"qtc_u": q[0], "qtc_v": q[1]}


def unpack_chroma_frame(buf, nb: int) -> dict:
    """One frame's packed chroma stream in the varint coding (so_pack_chroma_frames; the format is
    in include/streamoptima.h) -> {"qtc_u", "qtc_v"}, int16 [nb, 64] each.  Raises ValueError on
    malformed input, by the rules of so_unpack_chroma_frames: a varint running past 5 bytes or off
    the end, a zigzag value of 2^16 or more, a token -L with L > 64 - k or Z > 64 - k, bytes left
    after the last record's V list.  Record boundaries are not known here (no offsets), so a
    varint or a list running from one record into the next is seen only where parsing stops."""
    va = varints(buf)
    if va.size and (int(va.min()) < -32768 or int(va.max()) > 32767):
        raise ValueError("a value outside int16 in the packed chroma stream")
    v = va.tolist()
    p = 0

    def nxt() -> int:
        nonlocal p
        if p >= len(v):
            raise ValueError("packed chroma stream ends inside a record")
        p += 1
        return v[p - 1]

    out = _chroma_lists(nb, nxt, lambda n: [nxt() for _ in range(n)], lambda: None, lambda b: None)
    if p != len(v):
        raise ValueError(f"{len(v) - p} values after the last record")
    return out


def unpack_chroma_frame_bits(buf, nb: int) -> dict:
    """One frame's packed chroma stream in the "bits" coding (so_pack_chroma_frames_bits) ->
    {"qtc_u", "qtc_v"} as unpack_chroma_frame.  Parses sequentially and skips to the next byte
    boundary after each record, so it needs no offsets.  Raises ValueError on malformed input, by
    the rules of so_unpack_chroma_frames_bits: a ue prefix of more than 16 zero bits, a decoded
    z > 65535, a code running past the last byte, the token rules of unpack_chroma_frame, a set
    pad bit, bytes after the last record."""
    r = _BitReader(buf, "packed chroma stream")
    kk = 0

    def start_of_record() -> None:
        nonlocal kk
        kk = r.take(2)

    def end_of_record(b: int) -> None:
        if r.pad():
            raise ValueError(f"record {b}: a set bit in the padding")

    out = _chroma_lists(nb, r.ue, lambda n: [r.ue(kk) for _ in range(n)], start_of_record, end_of_record)
    if r.left():
        raise ValueError(f"{r.left()} bytes after the last record")
    return out


# ---- the "huff" coding of both streams (so_pack_frames_huff / so_pack_chroma_frames_huff) ---------
_HUFF_SYMS, _HUFF_MAXLEN = 43, 15


def _huff_cls(p: int) -> int:
    return min(p.bit_length(), 6)


class _HuffReader(_BitReader):
    """The bit reader with values read through a frame's Huffman tables, which sit at its head:
    ntab tables of 43 four-bit code lengths (include/streamoptima.h)."""

    def __init__(self, buf, stream: str, ntab: int):
        super().__init__(buf, stream)
        nnib = ntab * _HUFF_SYMS
        nbytes = (nnib + 1) // 2
        if len(self.data) < nbytes:
            raise ValueError(f"the {stream} is shorter than its tables")
        nib = [x for c in self.data[:nbytes] for x in (c >> 4, c & 15)]
        if any(nib[nnib:]):
            raise ValueError(f"a set spare nibble after the tables of the {stream}")
        self.pos = 8 * nbytes
        self.tables = []
        for t in range(ntab):
            lens = nib[t * _HUFF_SYMS:(t + 1) * _HUFF_SYMS]
            if sum(1 << (_HUFF_MAXLEN - n) for n in lens if n) > 1 << _HUFF_MAXLEN:
                raise ValueError(f"table {t} of the {stream}: Kraft sum above 1")
            rows, code = [], 0                   # per length: (first code, its symbols by symbol)
            for n in range(1, _HUFF_MAXLEN + 1):
                syms = [s for s in range(_HUFF_SYMS) if lens[s] == n]
                rows.append((code, syms))
                code = (code + len(syms)) << 1
            self.tables.append(rows)

    def value(self, t: int) -> int:
        top = self.peek(_HUFF_MAXLEN)
        for n, (first, syms) in enumerate(self.tables[t], 1):
            c = (top >> (_HUFF_MAXLEN - n)) - first
            if 0 <= c < len(syms):
                self.take(n)
                s = syms[c]
                z = s if s < 32 else 1 << (s - 27) | self.take(s - 27)
                return (z >> 1) ^ -(z & 1)
        raise ValueError(f"a bit pattern that matches no code of table {t} in the {self.stream}")

    def token_list(self, order, nn: int, tok0: int, what: str) -> np.ndarray:
        """_token_list with the tables picked by position; tok0: the first token table."""
        k = 0

        def token() -> int:
            return self.value(tok0 + _huff_cls(k))

        def coefs(n: int) -> list:
            return [self.value(tok0 + 7 + _huff_cls(k + i)) for i in range(n)]

        q = np.zeros(nn, dtype=np.int16)
        while k < nn:
            t = token()
            if t < 0:
                if -t > nn - k:
                    raise ValueError(f"{what}: a list of {-t} values at position {k} of {nn}")
                q[order[k:k - t]] = coefs(-t)
                k -= t
            elif t == 0:
                break
            else:
                if t > nn - k:
                    raise ValueError(f"{what}: a run of {t} zeros at position {k} of {nn}")
                k += t
        return q


def unpack_frame_huff(buf, nb: int, bs: int, frame_type: int) -> dict:
    """One frame's packed stream in the "huff" coding (so_pack_frames_huff; the format is in
    include/streamoptima.h) -> {"split", "mv", "qtc"} as unpack_frame.  Reads the 15 tables at the
    frame's head, then parses sequentially, skipping to the next byte boundary after each block,
    so it needs no offsets.  Raises ValueError on malformed input, by the rules of
    so_unpack_frames_huff: bytes shorter than the tables, a table with a Kraft sum above 1, a set
    spare nibble, a bit pattern that matches no code, a code running past the last byte, split = 1
    at block size 8, the token rules of unpack_frame, a set pad bit, bytes after the last block."""
    r = _HuffReader(buf, "packed stream", 15)
    inter = frame_type == 1
    split = np.zeros(nb, dtype=np.uint8)
    mv = np.zeros((nb, 4, 3) if inter else (nb, 4), dtype=np.int16)
    qtc = np.zeros((nb, bs * bs), dtype=np.int16)
    sb = bs // 2
    for b in range(nb):
        sp = r.take(1)
        if sp and bs != 16:
            raise ValueError(f"block {b}: split at block size {bs}")
        split[b] = sp
        nmv = (4 if sp else 1) * (3 if inter else 1)
        mv[b].reshape(-1)[:nmv] = [r.value(0) for _ in range(nmv)]
        for n, off in ([(sb, j * sb * sb) for j in range(4)] if sp else [(bs, 0)]):
            qtc[b, off:off + n * n] = r.token_list(scan_order(n), n * n, 1, f"block {b}")
        if r.pad():
            raise ValueError(f"block {b}: a set bit in the padding")
    if r.left():
        raise ValueError(f"{r.left()} bytes after the last block")
    return {"split": split, "mv": mv, "qtc": qtc}


def unpack_chroma_frame_huff(buf, nb: int) -> dict:
    """One frame's packed chroma stream in the "huff" coding (so_pack_chroma_frames_huff) ->
    {"qtc_u", "qtc_v"} as unpack_chroma_frame: the 14 tables at the frame's head, then the records
    in sequence.  Raises ValueError by the rules of so_unpack_chroma_frames_huff."""
    r = _HuffReader(buf, "packed chroma stream", 14)
    q = np.zeros((2, nb, 64), dtype=np.int16)
    for b in range(nb):
        for j in range(2):
            q[j, b] = r.token_list(scan_order(8), 64, 0, f"record {b}")
        if r.pad():
            raise ValueError(f"record {b}: a set bit in the padding")
    if r.left():
        raise ValueError(f"{r.left()} bytes after the last record")
    return {"qtc_u": q[0], "qtc_v": q[1]}


# ---- chroma residual line (build extension: chroma 4:2:0) ------------------------------------------
def chroma_residual_line(u_blocks, v_blocks) -> str:
    """One frame's chroma coefficients: U's entropy_encoder_frame line at block size 8, '|', V's
    (every chroma block is unsplit: one 8x8 transform per 16x16 luma block)."""
    return entropy_encoder_frame(u_blocks, 8) + "|" + entropy_encoder_frame(v_blocks, 8)


def parse_chroma_residual_line(line: str):
    """-> (qtc_u, qtc_v), int16 [nb, 64] each."""
    parts = line.strip().split("|")
    if len(parts) != 2:
        raise ValueError("a chroma residual line holds U's blocks, '|', V's blocks")
    out = []
    for part in parts:
        blocks = entropy_decoder_frame(part, 8)
        if any(s != 0 for s, _ in blocks):
            raise ValueError("chroma blocks are never split")
        out.append(np.stack([np.asarray(b) for _, b in blocks]).reshape(len(blocks), 64).astype(np.int16))
    if out[0].shape != out[1].shape:
        raise ValueError(f"chroma residual line: {out[0].shape[0]} U blocks against {out[1].shape[0]} V blocks")
    return out[0], out[1]


# ---- per-block QP map line (build extension: ROI / two-pass RC) --------------------------------
def qp_map_line(qp_map, qp_rows, base_qp, num_blocks_per_row) -> str:
    """Per-block QPs as comma-separated deltas against the row's QP (the per-row QP the
    reference line already carries, or the frame QP without rate control)."""
    nbx = int(num_blocks_per_row)
    q = np.asarray(qp_map).reshape(-1, nbx)
    base = np.asarray(qp_rows if qp_rows else [base_qp] * q.shape[0]).reshape(-1, 1)
    return ",".join(str(int(v)) for v in (q - base).reshape(-1))


def parse_qp_map_line(line: str, qp_rows, base_qp, num_blocks_per_row) -> np.ndarray:
    nbx = int(num_blocks_per_row)
    d = np.array([int(t) for t in line.strip().split(",")], np.int32).reshape(-1, nbx)
    base = np.asarray(qp_rows if qp_rows else [base_qp] * d.shape[0], np.int32).reshape(-1, 1)
    return (d + base).reshape(-1).astype(np.int32)
