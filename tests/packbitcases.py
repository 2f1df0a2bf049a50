"""Test helper: edge-case symbols for the "bits" coding of the packed stream (the format:
tests/packbitsref.py), numpy only.

corpus(kind, frame_type) -> (split, mv, qtc) as packcases.corpus, which it starts with unchanged
(all four kinds, both frame types), followed by blocks aimed at the bit-granular codes:
  * every value v with zz(v) + 1 in {2^n - 1, 2^n, 2^n + 1}, n = 1..16, and -32768 -- where a
    code's length changes -- as coefficients (together and one per block) and as mv values;
  * blocks whose canonical order k is 0, 1, 2 and 3, and exact ties between neighbouring orders;
  * a family of blocks whose lengths step through every pad length 0..7;
  * every coefficient -32768 with every mv -32768: the longest block;
  * an all-zero block with zero mv: the shortest (1 byte intra);
  * split blocks mixing an empty and a full sub-block.
Every block is a vector over its scan positions placed through packcases.placement, as there.

mutants(block, bs, frame_type) -> deterministic single-block damage built from the model's
layout of a well-formed block."""
from functools import lru_cache

import numpy as np

import packbitsref
import packcases

KINDS = packcases.KINDS
block_size = packcases.block_size
used_mv = packcases.used_mv
SHORT = 24                                       # bytes: the mutants' base blocks


def unzz(z: int) -> int:
    return z >> 1 if not z & 1 else -(z >> 1) - 1


def edge_values() -> list:
    """Every int16 v with zz(v) + 1 in {2^n - 1, 2^n, 2^n + 1}, n = 1..16 (0 and -32768 included)."""
    ms = sorted({m for n in range(1, 17) for m in (2 ** n - 1, 2 ** n, 2 ** n + 1)} | {65536})
    return [unzz(m - 1) for m in ms if 1 <= m <= 65536]


# (values, canonical k): one order strictly best, or an exact tie (the smaller order wins)
# the last: a coefficient's longest canonical code, 32 bits (no value is shorter at order 0 than
# at order 2, so next to a -32768 the canonical order is never 0)
FORCE_K = (([1], 0), ([2], 1), ([12], 2), ([100], 3), ([1, -1], 0), ([-2, -1], 1), ([-4, -2], 2),
           ([-1, -32768, -1, -1], 1))


def extra_vectors(nn: int) -> list:
    """[(scan-domain vector, mv fill or None)]: None = the cycling edge values."""
    q = nn // 4
    ev = edge_values()
    nz = [v for v in ev if v]
    out = []

    def add(v, mvfill=None):
        v = np.asarray(v, np.int16)
        assert v.shape == (nn,)
        out.append((v, mvfill))

    v = np.zeros(nn, np.int16)
    v[:len(nz)] = nz                                # all of them, one run
    add(v)
    v = np.zeros(nn, np.int16)
    v[nn - len(nz):] = nz[::-1]
    add(v)
    for i, x in enumerate(nz):                      # one per block, at moving positions
        v = np.zeros(nn, np.int16)
        v[(i * 5) % nn] = x
        add(v)
    for vals, _ in FORCE_K:
        for reps in (1, 3, q):                      # the same mix, so the same order, at three sizes
            v = np.zeros(nn, np.int16)
            w = (vals * reps)[:nn]
            v[:len(w)] = w
            add(v, 0)
    for j in range(1, 25):                          # lengths stepping through every pad length
        v = np.zeros(nn, np.int16)
        v[:j] = 1
        add(v, 0)
        v = np.zeros(nn, np.int16)
        v[1:2 * j:2] = -3
        add(v, 1)
    add(np.full(nn, -32768), -32768)                # the longest
    add(np.zeros(nn), 0)                            # the shortest; twice: split and unsplit in "m16"
    add(np.zeros(nn), 0)
    for full in ((0,), (1,), (3,), (0, 2), (1, 3), (0, 1, 2), (1, 2, 3)):
        for val in (-32768, 1):
            v = np.zeros(nn, np.int16)
            for j in full:
                v[j * q:(j + 1) * q] = val
            add(v)
    return out


@lru_cache(maxsize=None)
def corpus(kind: str, frame_type: int):
    s0, m0, q0 = packcases.corpus(kind, frame_type)
    bs = block_size(kind)
    nn = bs * bs
    extra = extra_vectors(nn)
    n = len(extra)
    b = np.arange(n)
    split = {"u16": b * 0, "s16": b * 0 + 1, "m16": b % 2, "u8": b * 0}[kind].astype(np.uint8)
    qtc = np.zeros((n, nn), np.int16)
    shape = (n, 4, 3) if frame_type == 1 else (n, 4)
    ev = np.array(edge_values(), np.int16)
    mv = ev[(np.arange(int(np.prod(shape))) * 7 + 2) % ev.size].reshape(shape)
    for i, (v, mvfill) in enumerate(extra):
        qtc[i, packcases.placement(bs, bool(split[i]))] = v
        if mvfill is not None:
            mv[i] = mvfill
    out = (np.concatenate([s0, split]), np.concatenate([m0, mv]), np.concatenate([q0, qtc]))
    for a in out:
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def block_bytes(kind: str, frame_type: int) -> tuple:
    """Every corpus block's bytes from the model's writer."""
    split, mv, qtc = corpus(kind, frame_type)
    return tuple(packbitsref.pack_blocks_bits(split, mv, qtc, block_size(kind), frame_type))


def mutant_base(kind: str, frame_type: int, n: int = 20) -> list:
    """The bytes of n corpus blocks of at most SHORT bytes, spread over the corpus and over the
    lengths: the valid frame the mutants start from."""
    short = sorted({x for x in block_bytes(kind, frame_type) if len(x) <= SHORT}, key=lambda x: (len(x), x))
    return [short[i] for i in np.linspace(0, len(short) - 1, n).astype(int)]


def mutants(block: bytes, bs: int, frame_type: int):
    """[(name, bytes)]: every single-bit flip, the last byte cut, one byte appended (0x00 and
    0x80), each pad bit set, k rewritten to each other order with the stream left alone."""
    lay = packbitsref.block_bits_layout(block, bs, frame_type)
    out = []

    def flip(bit):
        raw = bytearray(block)
        raw[bit >> 3] ^= 0x80 >> (bit & 7)
        return bytes(raw)

    for bit in range(8 * len(block)):
        out.append((f"bit {bit}", flip(bit)))
    out.append(("last byte cut", block[:-1]))
    out.append(("0x00 appended", block + b"\x00"))
    out.append(("0x80 appended", block + b"\x80"))
    pad = next(x for x in lay if x[0] == "pad")
    for bit in range(pad[1], pad[2]):
        out.append((f"pad bit {bit}", flip(bit)))       # also among the flips: named here
    k = next(x for x in lay if x[0] == "k")[3]
    for other in range(4):
        if other != k:
            raw = bytearray(block)
            raw[0] = (raw[0] & 0x9F) | (other << 5)     # bits 1-2 of the first byte
            out.append((f"k {k} -> {other}", bytes(raw)))
    return out
