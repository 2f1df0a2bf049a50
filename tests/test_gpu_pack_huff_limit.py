"""huff_tables_kernel where the 15-bit length limit binds: frames whose histograms make Huffman's
tree deeper than 15 (tests/packhuffcases.py limit_frames: Fibonacci counts over 17 symbols, once,
twice and four times, for 1, 2 and 3 halvings of the counts), packed by so_pack_frames_huff /
so_pack_chroma_frames_huff(_after) and compared with the plain-Python model (tests/packhuffref.py)
byte for byte -- every record, offs, the totals, the table bytes at the head of record 0 -- then
unpacked back to the inputs.  A wrong length still gives a decodable prefix code; only equality with
the model shows it.  What each frame is for is asserted from the model (check_limit_design) before
the GPU is looked at, so that no case can quietly stop reaching the halving loop."""
import numpy as np
import pytest

import packhuffcases as C
import packhuffref as H
import test_gpu_pack_huff as L
import test_gpu_pack_huff_chroma as Q

pytestmark = pytest.mark.gpu

LUMA = tuple(n for n in C.LIMIT_NAMES if n != "chroma")


@pytest.mark.parametrize("name", LUMA)
def test_pack_huff_length_limit_bytes_exact(gpu, name):
    """mixed: tables of 0, 1, 2 and 3 halvings, of one symbol and of none in one frame, one lane
    each, with ties between leaves and merged nodes after the halving; three: frames of 0, 2 and 1
    halvings in one call; mv, tok, coef5, bs8: the limit in the mv table, a token table, a
    coefficient table of class 5 and at block size 8; wide: a 30-bit coefficient and a 23-bit token;
    equal: 43 equal counts next to a halved table."""
    C.check_limit_design(name)
    fs = C.limit_frames()[name]
    blocks = C.limit_model(name)
    frames = [(f["ftype"], f["split"], f["mv"], f["qtc"]) for f in fs]
    bs, nb = fs[0]["bs"], fs[0]["split"].size
    T = H.LUMA_TABLE_BYTES
    for f, blk in zip(fs, blocks):
        assert blk[0][:T] == H.table_bytes([lens for _, lens, _ in C.limit_rounds(f)])
    cap = L._cap_for(blocks)
    offs, out, tot = L._pack(gpu, frames, bs, cap)
    for i, blk in enumerate(blocks):                           # the tables first: the clearest message
        assert out[i, :T].tobytes() == blk[0][:T], (name, i, "table bytes")
    L._check_pack(offs, out, tot, blocks, cap)
    own = [out[i, :int(offs[i, nb])].tobytes() for i in range(len(fs))]
    u = L._Unpack(gpu, own, [offs[i, :nb + 1] for i in range(len(fs))], nb, bs)
    u.launch(list(range(len(fs))), [f["ftype"] for f in fs])
    L._check_unpack(u.fetch(), frames)


@pytest.mark.parametrize("after", [False, True])
def test_pack_chroma_huff_length_limit_bytes_exact(gpu, after):
    """The limit in a chroma frame, whose U and V lists share the tables; once through the _after
    placement."""
    C.check_limit_design("chroma")
    f = C.limit_frames()["chroma"][0]
    blk = C.limit_model("chroma")[0]
    nb, T = len(blk), H.CHROMA_TABLE_BYTES
    assert blk[0][:T] == H.table_bytes([lens for _, lens, _ in C.limit_rounds(f)])
    bases = (5,) if after else None
    cap = sum(len(x) for x in blk) + 64
    offs, out, tot = Q._pack(gpu, [(f["qu"], f["qv"])], cap, bases=bases)
    base = 5 if after else 0
    assert out[0, base:base + T].tobytes() == blk[0][:T], "table bytes"
    Q._check_pack(offs, out, tot, [blk], cap, bases=bases)
    own = out[0, base:base + int(offs[0, nb])].tobytes()
    q, err = Q._unpack(gpu, [own], [offs[0, :nb + 1]], nb)
    assert err.tolist() == [0]
    Q._check_unpack(q, [(f["qu"], f["qv"])])
