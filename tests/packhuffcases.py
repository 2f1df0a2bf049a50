"""Test helper: hand-made frames for the "huff" coding of the packed stream (the model:
tests/packhuffref.py), numpy only -- a small valid frame, and one damaged copy of it for every rule
that makes a stream malformed, next to valid streams whose tables are not the canonical ones; frames
whose histograms bind the 15-bit length limit of the table build (limit_frames); and the seeded
corpus of single records, record mutants and table mutants for the decoder's host build under
sanitizers and for the GPU unpack (host_cases, gpu_frames)."""
from functools import lru_cache

import numpy as np

import packchromaref as R
import packhuffref as H


def small_frame():
    """A 6-block inter frame at bs 16 (block 1 split) whose symbols are few, so every code is short."""
    nb = 6
    split = np.array([0, 1, 0, 0, 0, 0], np.uint8)
    mv = np.zeros((nb, 4, 3), np.int16)
    mv[:, :, 0] = np.arange(nb)[:, None] - 2
    mv[:, :, 1] = 1
    qtc = np.zeros((nb, 256), np.int16)
    qtc[0, :3] = [5, -3, 1]
    qtc[1, 0], qtc[1, 64], qtc[1, 200] = 40, -7, 2
    qtc[2, 17] = -300
    qtc[4, :] = 1
    return split, mv, qtc


def malformed_cases():
    """[(name, blocks, the block a decoder reports or None when well-formed)] -- one hand-made case
    for each malformed rule, and valid streams a decoder must accept."""
    split, mv, qtc = small_frame()
    good = H.pack_blocks_huff(split, mv, qtc, 16, 1)
    tables = H.parse_tables(good[0], 15)
    T = H.LUMA_TABLE_BYTES
    out = [("canonical", good, None)]

    def with_block(b, data):
        x = list(good)
        x[b] = bytes(data)
        return x

    def with_tables(tb):
        return with_block(0, H.table_bytes(tb) + good[0][T:])
    # valid, not canonical: every used symbol of every table at one equal length
    flat = []
    for t in tables:
        used = sum(1 for n in t if n)
        n = max(1, (used - 1).bit_length())
        flat.append([n if x else 0 for x in t])
    out.append(("equal lengths", H.pack_blocks_huff(split, mv, qtc, 16, 1, tables=flat), None))
    # valid: an incomplete table (Kraft sum below 1): every length one longer
    longer = [[x + 1 if x else 0 for x in t] for t in tables]
    assert all(max(t) <= 15 for t in longer)
    out.append(("incomplete tables", H.pack_blocks_huff(split, mv, qtc, 16, 1, tables=longer), None))
    # tables: Kraft sum above 1 (three codes of length 1)
    over = [list(t) for t in tables]
    over[3][:3] = [1, 1, 1]
    out.append(("kraft above 1", with_tables(over), 0))
    # tables: the spare nibble set
    raw = bytearray(good[0])
    raw[T - 1] |= 1
    out.append(("spare nibble", with_block(0, raw), 0))
    # frame bytes shorter than the tables
    out.append(("short tables", with_block(0, good[0][:T - 1]), 0))
    out.append(("empty block 0", with_block(0, b""), 0))
    # a bit pattern that matches no code: an incomplete mv table, block 3's first mv code replaced by 15 ones
    lon = H.pack_blocks_huff(split, mv, qtc, 16, 1, tables=longer)
    x = list(lon)
    x[3] = bytes([x[3][0] | 0x7F, 0xFF]) + x[3][2:]
    out.append(("no code matches", x, 3))
    # a code past the block's last byte
    out.append(("code past the end", with_block(2, good[2][:-1]), 2))
    out.append(("empty block", with_block(5, b""), 5))
    # 8 or more bits after the last list; a set pad bit
    out.append(("a byte appended", with_block(3, good[3] + b"\x00"), 3))
    # the token rules: code -L = -256 at position 0 of a split block's 64-coefficient list
    heads, records = H.luma_records(split, mv, qtc, 16, 1)
    rec = list(records[1])
    first_tok = 12                                   # after the split block's 12 mv values
    assert rec[first_tok][0] == H.LUMA_TOK and rec[first_tok][1] == -1
    big = records[4][3]                              # block 4's token: -256 in table tok0
    assert big == (H.LUMA_TOK, -256)
    rec[first_tok] = big
    both = H.count_tables([r for r in records], 15)
    forged = H._encode([records[0], rec] + records[2:], heads, both)
    out.append(("list longer than the sub-block", forged, 1))
    return out


def pad_case():
    """A block with pad bits, one of them set."""
    split, mv, qtc = small_frame()
    good = H.pack_blocks_huff(split, mv, qtc, 16, 1)
    heads, records = H.luma_records(split, mv, qtc, 16, 1)
    codes = [H.canonical_codes(t) for t in H.parse_tables(good[0], 15)]
    for b in range(1, 6):
        nbits = 1 + sum(len(codes[t][H.symbol(v)[0]]) + len(H.symbol(v)[1]) for t, v in records[b])
        if nbits % 8:
            x = list(good)
            x[b] = good[b][:-1] + bytes([good[b][-1] | 1])
            return x, b
    raise AssertionError("no block with padding")


def all_cases():
    """malformed_cases() and the pad case: [(name, blocks, bad block or None)] at bs 16, inter."""
    x, b = pad_case()
    return malformed_cases() + [("pad bit set", x, b)]


def split_at_bs8():
    """One all-zero inter block at bs 8 with its split bit set: ([bytes], 0)."""
    s8, m8, q8 = np.zeros(1, np.uint8), np.zeros((1, 4, 3), np.int16), np.zeros((1, 64), np.int16)
    one = H.pack_blocks_huff(s8, m8, q8, 8, 1)
    return [one[0][:H.LUMA_TABLE_BYTES] + bytes([one[0][-1] | 0x80])], 0


def chroma_cases():
    """-> (qtc_u, qtc_v, [(name, records, bad record or None)]): six corpus records."""
    qu, qv = R.corpus()
    qu, qv = qu[40:46], qv[40:46]
    good = H.pack_chroma_records_huff(qu, qv)
    T = H.CHROMA_TABLE_BYTES
    tables = H.parse_tables(good[0], 14)
    over = [list(t) for t in tables]
    over[0][:3] = [1, 1, 1]
    longer = [[x + 1 if x else 0 for x in t] for t in tables]
    lon = H.pack_chroma_records_huff(qu, qv, tables=longer)
    nomatch = list(lon)
    nomatch[4] = bytes([0xFF, 0xFF]) + lon[4][2:]
    return qu, qv, [("canonical", good, None), ("incomplete tables", lon, None),
                    ("kraft above 1", [H.table_bytes(over) + good[0][T:]] + good[1:], 0),
                    ("short tables", [good[0][:T - 1]] + good[1:], 0),
                    ("no code matches", nomatch, 4),
                    ("code past the end", good[:3] + [good[3][:-1]] + good[4:], 3),
                    ("a byte appended", good[:2] + [good[2] + b"\x00"] + good[3:], 2)]


# ---- frames whose histograms bind the 15-bit length limit --------------------------------------------
# 17 symbols with Fibonacci counts make Huffman's tree a chain of depth 16: the smallest histogram
# (4,180 values) whose longest code passes 15, so that the counts are halved and the table rebuilt.
# Twice and four times the counts need 2 and 3 halvings.  The most frequent symbol may be more
# frequent still (it joins the chain last whatever its count), so fill values elsewhere in a frame use
# that symbol.  Every design is checked from the model (limit_rounds) by the tests that use it.
FIB = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597)
COEF_SYMS = (1,) + tuple(range(3, 18)) + (2,)           # rarest first; the most frequent: the value 1
WIDE_SYMS = tuple(range(42, 31, -1)) + (1, 3, 4, 5, 2)    # 16: no halving, the longest code 15 bits; the rarest: the escape classes, 42 first
MV_SYMS = tuple(range(1, 17)) + (0,)


def sym_value(sym: int) -> int:
    """A value whose symbol is sym; an escape class: all its raw bits set (42: -32768)."""
    return H.unzz(sym if sym < 32 else (1 << (sym - 26)) - 1)


def fib_values(scale: int, syms=COEF_SYMS) -> list:
    """scale * FIB[r] times the value of syms[r]."""
    return [sym_value(s) for s, n in zip(syms, FIB) for _ in range(scale * n)]


def _vectors(values, positions, nn: int, seed: int, fill: int = 1) -> np.ndarray:
    """Scan-domain vectors [n, nn]: `values`, shuffled, at `positions` of as many blocks as it takes
    (the last block topped up with the last, most frequent, value), `fill` everywhere else."""
    per = len(positions)
    vals = list(values) + [values[-1]] * (-len(values) % per)
    np.random.default_rng(seed).shuffle(vals)
    out = np.full((len(vals) // per, nn), fill, np.int16)
    out[:, positions] = np.array(vals, np.int16).reshape(-1, per)
    return out


# FIB rank -> run length.  17 ranks: as many zero runs as runs of ones.  16 ranks (no halving, the
# longest code 15 bits): one run of ones more.  The run of 200 ones, the rarest: an escape class with 8
# raw bits.
TOK17 = ({16: 1, 13: 2, 10: 3, 7: 4, 4: 5, 0: 6}, {15: 1, 14: 2, 12: 3, 11: 4, 9: 5, 8: 6, 6: 7, 5: 8, 3: 9, 2: 10, 1: 200})
TOK16 = ({15: 1, 12: 2, 9: 3, 6: 4, 3: 5}, {14: 1, 13: 2, 11: 3, 10: 4, 8: 5, 7: 6, 5: 7, 4: 8, 2: 9, 1: 10, 0: 200})


def _token_vectors(nn: int, seed: int, runs=TOK17) -> np.ndarray:
    """Scan-domain vectors whose tokens at covered counts >= 32 (table tok6) are the symbols of `runs`
    with Fibonacci counts: zero runs Z and runs of ones L laid as Z, L pairs that end exactly at nn (no
    end token) after a head of ones whose token goes to tok0; a run of ones more than zero runs: the
    first vector's head is zeros and that run follows it."""
    zeros, ones = runs
    Z = [n for r, n in zeros.items() for _ in range(FIB[r])]
    L = [n for r, n in ones.items() for _ in range(FIB[r])]
    assert len(L) - len(Z) in (0, 1)
    rng = np.random.default_rng(seed)
    rng.shuffle(Z)
    rng.shuffle(L)
    blocks, room = [[]], nn - 32
    if len(L) > len(Z):
        blocks[0].append((0, L.pop()))
        room -= blocks[0][0][1]
    for pair in zip(Z, L):
        if sum(pair) > room:
            blocks.append([])
            room = nn - 32
        blocks[-1].append(pair)
        room -= sum(pair)
    out = np.ones((len(blocks), nn), np.int16)
    for v, pairs in zip(out, blocks):
        at = nn - sum(z + n for z, n in pairs)
        if pairs[0][0] == 0:
            v[:at] = 0
        for z, n in pairs:
            v[at:at + z] = 0
            at += z + n
    return out


def _luma(bs: int, ftype: int, vecs, split, mv_values=None, mv_fill: int = 0) -> dict:
    """A luma frame from scan-domain vectors and their split flags; the used mv entries take
    mv_values in order, then mv_fill."""
    import packcases
    split = np.asarray(split, np.uint8)
    nb = split.size
    qtc = np.zeros((nb, bs * bs), np.int16)
    for b in range(nb):
        qtc[b, packcases.placement(bs, bool(split[b]))] = vecs[b]
    mv = np.full((nb, 4, 3) if ftype == 1 else (nb, 4), mv_fill, np.int16)
    if mv_values is not None:
        used = np.zeros(mv.shape, bool)
        used[:, 0] = True
        used[split == 1] = True
        assert len(mv_values) <= used.sum()
        flat = np.full(int(used.sum()), mv_fill, np.int16)
        flat[:len(mv_values)] = mv_values
        mv[used] = flat
    return {"kind": "luma", "bs": bs, "ftype": ftype, "split": split, "mv": mv, "qtc": qtc}


SEG5 = [j * 64 + p for j in range(4) for p in range(16, 32)]   # split block: the positions of class 5
SEG4 = [j * 64 + p for j in range(4) for p in range(8, 16)]


def _pad(vecs, nb: int, nn: int) -> np.ndarray:
    return np.concatenate([vecs, np.ones((nb - len(vecs), nn), np.int16)])


LIMIT_NAMES = ("mixed", "three", "mv", "tok", "wide", "coef5", "bs8", "chroma", "equal")


@lru_cache(maxsize=None)
def limit_frames() -> dict:
    """name -> the frames of one call, each {"kind": "luma", bs, ftype, split, mv, qtc} or {"kind":
    "chroma", qu, qv}.  What each is for: check_limit_design."""
    import packcases
    out = {}
    hi = list(range(32, 256))
    # coef6 4 x FIB in 75 unsplit blocks; coef5 2 x FIB and coef4 1 x FIB in 131 split blocks; the other
    # coefficient tables hold the value 1 alone
    a = _vectors(fib_values(4), hi, 256, 1)
    b = _vectors(fib_values(2), SEG5, 256, 2)
    b4 = _vectors(fib_values(1), SEG4, 256, 3)
    b[:, SEG4] = _pad(b4, len(b), 256)[:, SEG4]
    rng = np.random.default_rng(4)
    out["mixed"] = _luma(16, 1, np.concatenate([a, b]), [0] * len(a) + [1] * len(b),
                         rng.integers(-5, 6, 3 * len(a) + 12 * len(b)))
    # one call: 0, 2 and 1 halvings
    two = _vectors(fib_values(2), hi, 256, 5)
    nb = len(two)
    noise = (rng.integers(-40, 41, (nb, 256)) * (rng.random((nb, 256)) < 0.3)).astype(np.int16)
    one = _pad(_vectors(fib_values(1), hi, 256, 6), nb, 256)
    out["three"] = [_luma(16, ft, v, [0] * nb, rng.integers(-9, 10, 3 * nb if ft else nb))
                    for ft, v in ((1, noise), (0, two), (1, one))]
    # the mv table: 349 split inter blocks of zeros
    n = -(-sum(FIB) // 12)
    out["mv"] = _luma(16, 1, np.zeros((n, 256), np.int16), [1] * n, fib_values(1, MV_SYMS))
    # a token table, and the widest codes: coef6 with the escape classes rarest
    tok = _token_vectors(256, 7)
    out["tok"] = _luma(16, 1, tok, [0] * len(tok))
    tok = _token_vectors(256, 8, TOK16)
    wide = _vectors(fib_values(1, WIDE_SYMS), hi, 256, 8)
    out["wide"] = _luma(16, 0, np.concatenate([tok, wide]), [0] * (len(tok) + len(wide)))
    # a coefficient table of class 5, split blocks
    c5 = _vectors(fib_values(1), SEG5, 256, 9)
    out["coef5"] = _luma(16, 0, c5, [1] * len(c5))
    # block size 8
    v8 = _vectors(fib_values(1), list(range(32, 64)), 64, 10)
    out["bs8"] = _luma(8, 1, v8, [0] * len(v8), rng.integers(-3, 4, 3 * len(v8)))
    # chroma: U's and V's class 6 positions share coef6
    vc = _vectors(fib_values(1), list(range(32, 64)), 64, 11)
    vc = _pad(vc, len(vc) + (len(vc) & 1), 64)
    place = packcases.placement(8, False)
    q = np.zeros_like(vc)
    q[:, place] = vc
    out["chroma"] = {"kind": "chroma", "qu": q[0::2].copy(), "qv": q[1::2].copy()}
    # all 43 symbols once in the mv table (lengths 5 and 6) next to a halved coef6
    one43 = _pad(_vectors(fib_values(1), hi, 256, 12), 43, 256)
    out["equal"] = _luma(16, 0, one43, [0] * 43, [sym_value(s) for s in range(43)])
    return {k: v if isinstance(v, list) else [v] for k, v in out.items()}


def frame_records(f):
    """-> (the frame's [[(table, value)]], its number of tables)."""
    if f["kind"] == "chroma":
        return H.chroma_records(f["qu"], f["qv"]), H.CHROMA_TABLES
    return H.luma_records(f["split"], f["mv"], f["qtc"], f["bs"], f["ftype"])[1], H.LUMA_TABLES


def limit_rounds(f) -> list:
    """Per table of the frame: (counts, lengths, halving rounds), from the model."""
    recs, ntab = frame_records(f)
    return [(c,) + H.huffman_rounds(c) for c in H.symbol_counts(recs, ntab)]


def pack_model(f) -> list:
    """The model's bytes of every record of the frame."""
    if f["kind"] == "chroma":
        return H.pack_chroma_records_huff(f["qu"], f["qv"])
    return H.pack_blocks_huff(f["split"], f["mv"], f["qtc"], f["bs"], f["ftype"])


@lru_cache(maxsize=None)
def limit_model(name: str) -> tuple:
    """The model's bytes of every record of every frame of limit_frames()[name], computed once."""
    return tuple(tuple(pack_model(f)) for f in limit_frames()[name])


def _widest(f, tables) -> tuple:
    """The most bits the model writes for one (mv value, token, coefficient) of the frame: code and
    raw bits."""
    recs, ntab = frame_records(f)
    tok0 = H.CHROMA_TOK if f["kind"] == "chroma" else H.LUMA_TOK
    w = [0, 0, 0]
    for rec in recs:
        for t, v in rec:
            sym, raw = H.symbol(v)
            k = 0 if t < tok0 else 1 if t < tok0 + 7 else 2
            w[k] = max(w[k], tables[t][sym] + len(raw))
    return tuple(w)


def check_limit_design(name: str) -> None:
    """Asserts, from the model alone, what the frames of limit_frames()[name] are for -- so that a test
    using them cannot quietly stop exercising the table build's halving loop."""
    frames = limit_frames()[name]
    per = [limit_rounds(f) for f in frames]
    rounds = [[r for _, _, r in tabs] for tabs in per]
    used = [[int((c > 0).sum()) for c, _, _ in tabs] for tabs in per]
    for tabs in per:
        assert all(max(lens) <= H.MAXLEN for _, lens, _ in tabs)
    if name == "mixed":
        # one frame at bs 16: tables of 0, 1, 2 and 3 halvings (lanes leave the loop at different times),
        # a table of one used symbol, an unused one; 0 halvings with several symbols too
        f, r, u = frames[0], rounds[0], used[0]
        assert f["bs"] == 16 and r[12:15] == [1, 2, 3] and r[0] == 0 and u[0] > 2
        assert 1 in u and 0 in u
        # ties after halving: in a halved table a leaf and a merged node of equal weight compete, and
        # the opposite tie order gives other lengths
        for c, lens, k in per[0][12:15]:
            hc = H.halved(c, k)
            straight, _, mixed = H._huffman(hc)
            assert straight == lens and mixed > 0 and H._huffman(hc, reverse_ties=True)[0] != lens
    elif name == "three":
        assert [max(r) for r in rounds] == [0, 2, 1] and len({f["split"].size for f in frames}) == 1
    elif name == "mv":
        assert rounds[0][H.MV] >= 1
    elif name == "tok":
        assert max(rounds[0][H.LUMA_TOK:H.LUMA_TOK + 7]) >= 1
    elif name == "coef5":
        assert rounds[0][H.LUMA_TOK + 7 + 5] >= 1 and frames[0]["split"].all()
    elif name == "bs8":
        assert frames[0]["bs"] == 8 and max(rounds[0]) >= 1
    elif name == "chroma":
        assert frames[0]["kind"] == "chroma" and max(rounds[0]) >= 1
    elif name == "equal":
        c, lens, _ = per[0][H.MV]
        assert (c == c[0]).all() and c[0] > 0 and sorted(lens) == [5] * 21 + [6] * 22
        assert max(rounds[0]) >= 1
    elif name == "wide":
        # the widest a packer writes: a coefficient of 15 + 15 bits (symbol 42, the rarest of a table
        # whose longest code is 15) and a token of 15 + 8 bits.  A token cannot take more: 9 raw bits
        # need zz = 512, a zero run of 256, and a zero run that reaches its list's end is written as 0.
        tables = [lens for _, lens, _ in per[0]]
        c, lens, _ = per[0][H.LUMA_TOK + 7 + 6]
        assert lens[42] == 15 == max(lens) and c[42] == min(x for x in c if x)
        assert _widest(frames[0], tables)[1:] == (23, 30)
    else:
        raise AssertionError(name)


# ---- single records for the decoder's host build and for the GPU unpack --------------------------------
# A case: (kind 0 luma 16 / 1 luma 8 / 2 chroma, frame type, the table bytes record 0 of its frame
# holds -- all of them, or fewer when record 0 is shorter --, the record's bytes -- record 0's: what
# follows the tables --, a name).  host_cases(): valid records, record mutants, table mutants.
SHORT = 24                                       # bytes: the record mutants' base records
NTAB = (H.LUMA_TABLES, H.LUMA_TABLES, H.CHROMA_TABLES)
TBYTES = (H.LUMA_TABLE_BYTES, H.LUMA_TABLE_BYTES, H.CHROMA_TABLE_BYTES)
REASONS = (tuple(r for r in H.RULES if r != "split at 8"), H.RULES,
           tuple(r for r in H.RULES if r not in ("split at 8", "spare nibble")))
FLAT6 = [6] * H.NSYM                             # every symbol has a code: any value can be written


def case_verdict(case):
    """The strict model on one case: ("ok", (split, mv flat, qtc flat)) or ("bad", the rule broken)."""
    kind, ftype, tb, body, _ = case
    try:
        v = H.unpack_record_huff_strict(kind, ftype, tb, body)
    except H.Malformed as e:
        return "bad", e.rule
    return "ok", (int(v["split"]), np.asarray(v["mv"]).reshape(-1), np.asarray(v["qtc"]).reshape(-1))


def _sources():
    """[(kind, frame type, heads, records)]: every packbitcases kind at both frame types, and the chroma
    corpus."""
    import packbitcases
    out = []
    for name in packbitcases.KINDS:
        bs = packbitcases.block_size(name)
        for ft in (0, 1):
            split, mv, qtc = packbitcases.corpus(name, ft)
            heads, recs = H.luma_records(split, mv, qtc, bs, ft)
            out.append((0 if bs == 16 else 1, ft, heads, recs))
    recs = H.chroma_records(*R.corpus())
    out.append((2, 0, [""] * len(recs), recs))
    return out


def _other_tables(tables):
    """Valid tables that are not the canonical ones: every used symbol of a table at one equal length;
    every length one longer (an incomplete code) where none is 15."""
    flat = []
    for t in tables:
        used = sum(1 for n in t if n)
        n = max(1, (used - 1).bit_length())
        flat.append([n if x else 0 for x in t])
    longer = [[x + 1 if x else 0 for x in t] if max(t) < H.MAXLEN else list(t) for t in tables]
    return flat, longer


def _bodies(heads, recs, tables):
    return [x if i else x[len(H.table_bytes(tables)):] for i, x in enumerate(H._encode(recs, heads, tables))]


def _spread(items, n):
    return [items[i] for i in np.linspace(0, len(items) - 1, min(n, len(items))).astype(int)]


def _flips(data: bytes, bits):
    for bit in bits:
        raw = bytearray(data)
        raw[bit >> 3] ^= 0x80 >> (bit & 7)
        yield f"bit {bit}", bytes(raw)


def _damage(data: bytes, lo: int = 0):
    """[(name, bytes)]: truncation to every shorter length down to lo, one and two bytes appended,
    every single-bit flip of the first 8 and last 2 bytes and a stride through the middle, the bytes
    from lo on all ones and all zeros."""
    n = len(data)
    out = [(f"cut to {k}", data[:k]) for k in range(lo, n)]
    out += [(f"+{x.hex()}", data + x) for x in (b"\x00", b"\xff", b"\x00\x00", b"\xff\xff", b"\x00\xff")]
    edge = sorted(set(range(lo * 8, min(n, lo + 8) * 8)) | set(range(max(lo, n - 2) * 8, n * 8)))
    out += list(_flips(data, edge + list(range((lo + 8) * 8 + 3, (n - 2) * 8, 5))))
    out += [("all ones", data[:lo] + b"\xff" * (n - lo)), ("all zeros", data[:lo] + bytes(n - lo))]
    return out


def _forged(kind, head, rec):
    """[(name, head, record)]: every token of the record replaced by one that overruns its (sub-)block
    by 1 and by the most a token can say, as a run of zeros and as a list of values."""
    tok0 = H.CHROMA_TOK if kind == 2 else H.LUMA_TOK
    nn = 64 if kind else (64 if head == "1" else 256)
    out, c, skip = [], 0, 0
    for i, (t, v) in enumerate(rec):
        if t < tok0:
            continue                                             # an mv value
        if skip:
            skip -= 1                                            # a coefficient of a list of values
            continue
        assert tok0 <= t < tok0 + 7 and t == tok0 + H.cls(c)
        for forged in (nn - c + 1, -(nn - c + 1), 32767, -32768):
            out.append((f"token {i} -> {forged}", head, rec[:i] + [(t, forged)] + rec[i + 1:]))
        skip = -v if v < 0 else 0
        c += abs(v)
        if v == 0 or c == nn:
            c = 0                                                # the next list
    return out


def _table_mutants(kind: int, rng) -> list:
    """[(name, table bytes as record 0 holds them, the tables when a record can be written with them or
    None)]."""
    ntab, T = NTAB[kind], TBYTES[kind]

    def same(lens):
        return [list(lens)] * ntab

    out = []
    for i in range(24):
        lo = (0, 3, 5, 7)[i % 4]                                  # from mostly above 1 to mostly below
        tabs = [list(rng.integers(lo, 16, H.NSYM)) for _ in range(ntab)]
        out.append((f"random nibbles {i}", H.table_bytes(tabs), None))
    exact = [5] * 21 + [6] * 22
    over = [5] * 22 + [6] * 20 + [15]
    assert H.kraft(exact) == 1 << 15 and H.kraft(over) == (1 << 15) + 1
    out.append(("kraft exactly 1", H.table_bytes(same(exact)), same(exact)))
    out.append(("kraft 1 + 2^-15", H.table_bytes(same(over)), None))
    for t in range(ntab):                                         # the excess in one table only
        tabs = same(exact)
        tabs[t] = over
        out.append((f"kraft 1 + 2^-15 in table {t}", H.table_bytes(tabs), None))
    out.append(("all lengths 15", H.table_bytes(same([15] * 43)), same([15] * 43)))
    out.append(("all lengths 0", H.table_bytes(same([0] * 43)), None))
    out.append(("one symbol of length 1", H.table_bytes(same([1] + [0] * 42)), same([1] + [0] * 42)))
    out.append(("one symbol of length 15", H.table_bytes(same([15] + [0] * 42)), same([15] + [0] * 42)))
    esc = [4] * 8 + [6] * 24 + [15] * 11
    assert H.kraft(esc) <= 1 << 15
    out.append(("escape classes at length 15", H.table_bytes(same(esc)), same(esc)))
    good = H.table_bytes(same(exact))
    if ntab & 1:
        for nib in (1, 8, 15):
            out.append((f"spare nibble {nib}", good[:-1] + bytes([good[-1] | nib]), None))
    out.append(("one byte short of the tables", good[:T - 1], None))
    out.append(("no table bytes", b"", None))
    return out


@lru_cache(maxsize=None)
def host_cases() -> tuple:
    """Every case, seeded: the valid records (canonical tables; some again with equal-length and
    incomplete tables), the record mutants of a base set of short records per source, record 0's with
    its tables in front, and the table mutants."""
    rng = np.random.default_rng(2024)
    cases = []
    for kind, ft, heads, recs in _sources():
        T = TBYTES[kind]
        canon = H.count_tables(recs, NTAB[kind])
        flat, longer = _other_tables(canon)
        sets = []
        for tname, tables, step in (("canonical", canon, 1), ("equal lengths", flat, 9), ("incomplete", longer, 9)):
            tb, bodies = H.table_bytes(tables), _bodies(heads, recs, tables)
            sets.append((tname, tb, bodies))
            cases += [(kind, ft, tb, bodies[b], f"{tname} {b}") for b in range(0, len(bodies), step)]
        # record mutants: short records spread over the lengths, under the canonical and the
        # incomplete tables (only there can a bit pattern match no code)
        for tname, tb, bodies in (sets[0], sets[2]):
            short = sorted({x for x in bodies if len(x) <= SHORT}, key=lambda x: (len(x), x))
            for body in _spread(short, 20 if tname == "canonical" else 8):
                cases += [(kind, ft, tb, x, f"{tname} {name}") for name, x in _damage(body)]
                if kind == 1:
                    cases.append((kind, ft, tb, bytes([body[0] | 0x80]) + body[1:], f"{tname} split bit set"))
            # record 0 with its tables in front: the damage reaches the tables
            whole = tb + _spread(short, 3)[1]
            for name, x in _damage(whole) + list(_flips(whole, range(64, 8 * T, 97))):
                cases.append((kind, ft, x[:T], x[T:], f"{tname} record 0 {name}"))
        # forged tokens, written with tables in which every symbol has a code
        tb6 = H.table_bytes([FLAT6] * NTAB[kind])
        few = [b for b in range(len(recs)) if len(recs[b]) <= 40]
        for b in _spread(few, 12):
            for name, head, rec in [("as it is", heads[b], recs[b])] + _forged(kind, heads[b], recs[b]):
                cases.append((kind, ft, tb6, _bodies([head], [rec], [FLAT6] * NTAB[kind])[0], f"record {b} {name}"))
    for kind in (0, 1, 2):
        zero = ("0", [(H.MV, 0)] * 3 + [(H.LUMA_TOK, 0)]) if kind < 2 else ("", [(H.CHROMA_TOK, 0)] * 2)
        for name, tb, tables in _table_mutants(kind, rng):
            for i in range(6):
                cases.append((kind, 1, tb, rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes(),
                              f"{name}: random record {i}"))
            if tables is not None:
                cases.append((kind, 1, tb, _bodies([zero[0]], [zero[1]], tables)[0], f"{name}: a zero record"))
    return tuple(cases)


@lru_cache(maxsize=None)
def gpu_frames(kind: int, nsample: int = 300) -> tuple:
    """Frames for the GPU unpack entry points: (name, frame type, the records' bytes -- record 0's
    begin with the table bytes --, whether the model accepts the tables, the model's verdict per
    record as case_verdict gives it).  The table mutants as frames of 7 records (seeded random bytes,
    and a valid record where the tables allow one), record 0 exactly the tables and one byte short of
    them, and a seeded sample of nsample record mutants as frames of one record."""
    rng = np.random.default_rng(77 + kind)
    T = TBYTES[kind]
    zero = ("0", [(H.MV, 0)] * 3 + [(H.LUMA_TOK, 0)]) if kind < 2 else ("", [(H.CHROMA_TOK, 0)] * 2)
    frames = []
    for name, tb, tables in _table_mutants(kind, rng):
        recs = [rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes() for _ in range(7)]
        if tables is not None:
            recs[3] = recs[6] = _bodies([zero[0]], [zero[1]], tables)[0]
        if len(tb) < T or name == "kraft exactly 1":
            frames.append((name + ", no body", 1, [tb] + recs[1:]))
        if len(tb) == T:
            frames.append((name, 1, [tb + recs[0]] + recs[1:]))
    import re
    valid = re.compile(r"(canonical|equal lengths|incomplete) \d+$")
    mutants = [c for c in host_cases() if c[0] == kind and not valid.match(c[4])]
    for i in rng.choice(len(mutants), nsample, replace=False):
        _, ft, tb, body, name = mutants[int(i)]
        frames.append((name, ft, [tb + body]))
    out = []
    for name, ft, recs in frames:
        verdicts = [case_verdict((kind, ft, recs[0][:T], r[T:] if b == 0 else r, name)) for b, r in enumerate(recs)]
        tables_ok = not (verdicts[0][0] == "bad" and verdicts[0][1] in ("short tables", "spare nibble", "kraft"))
        out.append((name, ft, tuple(recs), tables_ok, tuple(verdicts)))
    return tuple(out)
