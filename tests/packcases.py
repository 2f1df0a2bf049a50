"""Test helper: edge-case symbols for the packed stream (so_pack.hip), numpy only.

corpus(kind, frame_type) -> (split uint8 [nb], mv int16 [nb, 4, 3] or [nb, 4], qtc int16
[nb, bs * bs]) for kind "u16" (block size 16, unsplit), "s16" (every block split), "m16" (a
mix) and "u8" (block size 8).  Every block is written as a vector over its scan positions and
placed through bitstream.scan_order: 256 (64) positions unsplit, 4 x scan_order(8) at offsets
0 / 64 / 128 / 192 when split.  mv entries an unsplit block does not use hold non-zero values
on purpose (the packer must not read them); used_mv() is what a decoder returns.

mutations(block, bs, frame_type) -> deterministic single-block damage, for the differential
tests of the decoders against packref.unpack_block_strict."""
from functools import lru_cache

import numpy as np

import packref
from streamoptima_amd.bitstream import scan_order

KINDS = ("u16", "s16", "m16", "u8")
VALUES = (0, 1, -1, 63, -64, 64, -65, 8191, -8192, 8192, -8193, 32767, -32768)
RUN_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)
LONG = 128                                       # bytes: mutation_base, mutations


def block_size(kind: str) -> int:
    return 8 if kind == "u8" else 16


def placement(bs: int, split: bool) -> np.ndarray:
    """Element index of every scan position of a block."""
    if not split:
        return scan_order(bs)
    sb = bs // 2
    return np.concatenate([j * sb * sb + scan_order(sb) for j in range(4)])


def scan_vectors(nn: int) -> list:
    """The corpus in the scan domain: int16 vectors of nn positions."""
    q = nn // 4
    nz = [v for v in VALUES if v]
    dense = np.array([((i * 7) % 5 + 1) * (1 if i % 3 else -1) for i in range(nn)], np.int16)
    out = []

    def add(v):
        assert v.shape == (nn,)
        out.append(v.astype(np.int16))

    # one non-zero at each position; one zero at each position of a dense block
    for p in range(nn):
        v = np.zeros(nn, np.int16)
        v[p] = nz[p % len(nz)]
        add(v)
    for p in range(nn):
        v = dense.copy()
        v[p] = 0
        add(v)
    # runs of 7 in zeros and runs of 0 in sevens, from every 7th position
    for s in range(0, nn, 7):
        for length in RUN_LENGTHS:
            e = min(nn, s + length)
            v = np.zeros(nn, np.int16)
            v[s:e] = 7
            add(v)
            v = np.full(nn, 7, np.int16)
            v[s:e] = 0
            add(v)
    # around the sub-block boundaries (q, 2q, 3q when split)
    for c in (q, 2 * q, 3 * q):
        v = dense.copy()
        v[c - q // 3:c] = 0                    # a zero run ending exactly at the boundary
        add(v)
        v = dense.copy()
        v[c - q // 4:c + q // 3] = 0           # a zero run crossing it
        add(v)
        v = np.zeros(nn, np.int16)
        v[c - q // 4:c + q // 3] = dense[c - q // 4:c + q // 3]   # a non-zero run crossing it
        add(v)
        v = np.zeros(nn, np.int16)
        v[c - 1:c + 1] = 9                     # the shortest crossing run
        add(v)
    for j in range(4):
        v = dense.copy()
        v[j * q:(j + 1) * q] = 0               # an all-zero sub-block among dense ones
        add(v)
        v = np.zeros(nn, np.int16)
        v[j * q:(j + 1) * q] = dense[j * q:(j + 1) * q]
        add(v)
    add(np.zeros(nn, np.int16))
    add(dense)
    # alternating, both phases, every value -32768: the longest token stream
    for phase in (0, 1):
        v = np.zeros(nn, np.int16)
        v[phase::2] = -32768
        add(v)
    # +-32767 everywhere: with every mv -32768 (below) the most bytes a block can have
    add(np.where(np.arange(nn) % 2, 32767, -32767))
    # every value of VALUES, as runs and isolated
    for shift in range(len(VALUES)):
        add(np.array([VALUES[(i + shift) % len(VALUES)] for i in range(nn)]))
    for shift in range(0, len(VALUES), 4):
        v = np.zeros(nn, np.int16)
        v[::3] = [VALUES[(i + shift) % len(VALUES)] for i in range(len(v[::3]))]
        add(v)
    # random density, values in +-300
    rng = np.random.default_rng(nn)
    for _ in range(200):
        v = np.where(rng.random(nn) < rng.random(), rng.integers(-300, 301, nn), 0)
        add(v)
    return out


@lru_cache(maxsize=None)
def corpus(kind: str, frame_type: int):
    bs = block_size(kind)
    nn = bs * bs
    vecs = scan_vectors(nn)
    nb = len(vecs)
    b = np.arange(nb)
    split = {"u16": b * 0, "s16": b * 0 + 1, "m16": (b % 3 == 1) | (b % 7 == 3), "u8": b * 0}[kind].astype(np.uint8)
    qtc = np.zeros((nb, nn), np.int16)
    for i, v in enumerate(vecs):
        qtc[i, placement(bs, bool(split[i]))] = v
    shape = (nb, 4, 3) if frame_type == 1 else (nb, 4)
    mv = np.array(VALUES, np.int16)[(np.arange(int(np.prod(shape))) * 5 + 3) % len(VALUES)].reshape(shape)
    extreme = next(i for i, v in enumerate(vecs) if abs(int(v[0])) == 32767 and (np.abs(v) == 32767).all())
    mv[extreme - 2:extreme + 1] = -32768      # the two alternating blocks and the +-32767 one
    if kind == "m16":
        split[extreme - 2:extreme + 1] = 1
        for i in range(extreme - 2, extreme + 1):
            qtc[i] = 0
            qtc[i, placement(bs, True)] = vecs[i]
    for a in (split, mv, qtc):
        a.setflags(write=False)
    return split, mv, qtc


def used_mv(split, mv) -> np.ndarray:
    """mv as a decoder returns it: entries past the first of an unsplit block are 0."""
    out = np.array(mv)
    out[np.asarray(split) == 0, 1:] = 0
    return out


@lru_cache(maxsize=None)
def block_bytes(kind: str, frame_type: int) -> tuple:
    """Every corpus block's bytes from the plain-Python writer."""
    split, mv, qtc = corpus(kind, frame_type)
    bs = block_size(kind)
    return tuple(packref.pack_frame(split[b:b + 1], mv[b:b + 1], qtc[b:b + 1], bs, frame_type)
                 for b in range(split.size))


def mutation_base(kind: str, frame_type: int, n: int = 64) -> list:
    """The bytes of n corpus blocks, spread over the corpus: the valid frame the mutations start
    from.  Blocks of at most LONG bytes, in which every byte is mutated on its own (what a
    decoder does with a byte should not depend on how many follow), and to confirm that two long
    ones, mutated at their ends and tokens only (mutations): the corpus' longest block, dense in
    int16 extremes, and the shortest long one with the two-byte token 64 or -65 (the longest
    but one where tokens never need two bytes)."""
    every = block_bytes(kind, frame_type)
    blocks = [x for x in every if len(x) <= LONG]
    by_len = sorted((x for x in every if len(x) > LONG), key=len)
    bs = block_size(kind)
    toks = [{v for r, s, e, v, *_ in packref.block_layout(x, bs, frame_type) if r == "token"} for x in by_len]
    two = [x for x, t in zip(by_len, toks) if t & {64, -65}] or [x for x, t in zip(by_len, toks) if max(t) > 63]
    long_ones = [by_len[-1], two[0] if two else by_len[-2]]
    return [blocks[i] for i in np.linspace(0, len(blocks) - 1, n).astype(int)] + long_ones


def mutations(block: bytes, bs: int, frame_type: int, prev_byte: int = 0x80):
    """[(name, bytes)]: single-block damage and non-canonical rewrites of a well-formed block.
    prev_byte: the byte an offset one too small would pull in from the block before.  The
    continuation bit of every byte is flipped; in a block of more than LONG bytes only that of
    the first and last four bytes and of every token's bytes."""
    lay = packref.block_layout(block, bs, frame_type)
    out = []

    def put(name, start, end, repl):
        out.append((name, block[:start] + bytes(repl) + block[end:]))

    for bit in range(8):
        put(f"split^{1 << bit}", 0, 1, [block[0] ^ (1 << bit)])
    where = range(len(block))
    if len(block) > LONG:
        where = sorted(set(range(4)) | set(range(len(block) - 4, len(block)))
                       | {i for r, s, e, *_ in lay if r == "token" for i in range(s, e)})
    for i in where:
        put(f"cont@{i}", i, i + 1, [block[i] ^ 0x80])
    by_role = {r: [x for x in lay if x[0] == r] for r in ("split", "mv", "token", "coef")}
    picks = [x[0] for x in by_role.values() if x] + [x[-1] for x in by_role.values() if len(x) > 1]
    for role, s, e, val, k, nn in picks:
        for big in (32768, -32769, 40000, 2 ** 31):
            put(f"{role}@{s}={big}", s, e, packref.varint(big))
        put(f"{role}@{s} in 5 bytes", s, e, packref.varint_padded(val, 5))
        put(f"{role}@{s} in 6 bytes", s, e, packref.varint_padded(val, 6))
    toks = by_role["token"]
    for role, s, e, val, k, nn in toks[:2] + [x for x in toks[2:-2] if x[2] - x[1] == 2][:2] + toks[-2:]:
        sign = -1 if val < 0 else 1
        put(f"token@{s}={sign}*(nn-k)", s, e, packref.varint(sign * (nn - k)))
        put(f"token@{s}={sign}*(nn-k+1)", s, e, packref.varint(sign * (nn - k + 1)))
        put(f"token@{s}=-(nn-k)", s, e, packref.varint(-(nn - k)))
        put(f"token@{s}=0", s, e, packref.varint(0))
    out.append(("last byte cut", block[:-1]))
    out.append(("one byte before", bytes([prev_byte]) + block))
    out.append(("one byte after", block + b"\x00"))
    return out
