"""Test helper: hand-made frames for the "huff" coding of the packed stream (the model:
tests/packhuffref.py), numpy only -- a small valid frame, and one damaged copy of it for every rule
that makes a stream malformed, next to valid streams whose tables are not the canonical ones."""
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
