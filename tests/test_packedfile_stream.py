"""packedfile.open_frames (no GPU): the container read frame by frame.  Files written by write_frames
from synthetic host data, in both layouts and codings, with and without QP maps and chroma, one
frame without payload: the records that come back are the data that went in; every truncation and
one byte too many raise ValueError and nothing else; no read is larger than a frame record."""
import itertools

import numpy as np
import pytest

from streamoptima_amd import packedfile

H, W, BS = 32, 48, 16
NB = (H // BS) * (W // BS)
TYPES = (0, 1, 1, 0)


def _gop(chroma: bool, maps: bool, rc: bool, seed: int = 3):
    """write_frames' input: random bytes of random lengths (the container does not look inside)."""
    rng = np.random.default_rng(seed)
    frames = []
    for i, ft in enumerate(TYPES):
        lens = rng.integers(0, 40, NB).astype(np.uint16)
        if i == 2:
            lens[:] = 0                                   # a frame with zero payload bytes
        f = {"frame_type": ft, "qp_rows": [3 + i, 4 + i] if rc else [], "block_bytes": lens,
             "payload": rng.integers(0, 256, int(lens.sum())).astype(np.uint8).tobytes()}
        if maps:
            f["qp_map"] = None if i == 1 else rng.integers(0, 21, NB).astype(np.int32)
        if chroma:
            clens = rng.integers(1, 30, NB).astype(np.uint16)
            f["chroma_block_bytes"] = clens
            f["chroma_payload"] = rng.integers(0, 256, int(clens.sum())).astype(np.uint8).tobytes()
        frames.append(f)
    return frames


VARIANTS = [(c, m, r, k) for (c, m, r), k in itertools.product(
    [(False, False, False), (False, False, True), (True, False, False), (False, True, True), (True, True, True)],
    ("varint", "bits"))]


@pytest.mark.parametrize("chroma,maps,rc,coding", VARIANTS)
def test_frames_come_back_as_written(tmp_path, chroma, maps, rc, coding):
    frames = _gop(chroma, maps, rc)
    path = str(tmp_path / "gop.sopk")
    packedfile.write_frames(path, H, W, BS, NB, coding, frames, chroma_qp_offset=-2 if chroma else None)
    hdr, it = packedfile.open_frames(path)
    assert hdr == {"h": H, "w": W, "bs": BS, "nb": NB, "coding": coding, "layout": 1 if chroma or maps else 0,
                   "nframes": len(frames), "chroma": chroma, "has_qp_maps": maps,
                   "chroma_qp_offset": -2 if chroma else None}
    n = 0
    for f, g in zip(frames, it):
        n += 1
        assert set(g) == {"frame_type", "qp_rows", "block_bytes", "payload", "qp_map", "chroma_block_bytes",
                          "chroma_payload"}
        assert g["frame_type"] == f["frame_type"] and g["qp_rows"] == f["qp_rows"]
        assert g["block_bytes"].dtype == np.uint16 and np.array_equal(g["block_bytes"], f["block_bytes"])
        assert bytes(g["payload"]) == f["payload"]
        if f.get("qp_map") is None:
            assert g["qp_map"] is None
        else:
            assert g["qp_map"].dtype == np.uint8 and np.array_equal(g["qp_map"], f["qp_map"])
        if chroma:
            assert np.array_equal(g["chroma_block_bytes"], f["chroma_block_bytes"])
            assert bytes(g["chroma_payload"]) == f["chroma_payload"]
        else:
            assert g["chroma_block_bytes"] is None and g["chroma_payload"] is None
    assert n == len(frames)
    assert list(it) == []                                  # exhausted, and the file is closed


def _drain(path):
    hdr, it = packedfile.open_frames(path)
    return sum(1 for _ in it)


@pytest.mark.parametrize("chroma,maps", [(False, False), (True, True)])
def test_every_prefix_and_one_byte_more_raise_value_error(tmp_path, chroma, maps):
    frames = _gop(chroma, maps, rc=True)
    path = tmp_path / "gop.sopk"
    packedfile.write_frames(str(path), H, W, BS, NB, "varint", frames, chroma_qp_offset=1 if chroma else None)
    data = path.read_bytes()
    assert _drain(str(path)) == len(frames)
    cut = tmp_path / "cut.sopk"
    for n in range(len(data)):
        cut.write_bytes(data[:n])
        with pytest.raises(ValueError):
            _drain(str(cut))
    cut.write_bytes(data + b"\0")
    hdr, it = packedfile.open_frames(str(cut))
    for _ in range(len(frames) - 1):                      # visible at the last frame, not before
        next(it)
    with pytest.raises(ValueError, match="after the last frame"):
        next(it)


def test_errors_surface_at_their_frame(tmp_path):
    """A truncation inside frame 2 lets frames 0 and 1 through; lengths that do not add up and a
    bad header are ValueErrors too."""
    frames = _gop(True, True, rc=False)
    path = tmp_path / "gop.sopk"
    packedfile.write_frames(str(path), H, W, BS, NB, "bits", frames, chroma_qp_offset=0)
    data = path.read_bytes()
    sizes = []
    for f in frames:                                      # record sizes, from the format
        s = 3 + len(f["qp_rows"]) + 4 + 2 * NB + len(f["payload"]) + 1 + (NB if f["qp_map"] is not None else 0)
        sizes.append(s + 4 + 2 * NB + len(f["chroma_payload"]))
    assert 36 + sum(sizes) == len(data)
    start2 = 36 + sizes[0] + sizes[1]
    bad = tmp_path / "bad.sopk"
    bad.write_bytes(data[:start2 + 10])
    hdr, it = packedfile.open_frames(str(bad))
    assert next(it)["frame_type"] == 0 and next(it)["frame_type"] == 1
    with pytest.raises(ValueError, match="ends inside a frame"):
        next(it)
    # frame 1's byte count one too high: its lengths no longer add up
    p = 36 + sizes[0] + 3
    (count,) = np.frombuffer(data[p:p + 4], "<u4")
    bad.write_bytes(data[:p] + np.array([count + 1], "<u4").tobytes() + data[p + 4:])
    hdr, it = packedfile.open_frames(str(bad))
    next(it)
    with pytest.raises(ValueError, match="do not add up"):
        next(it)
    for edit, what in ((b"SOPX" + data[4:], "not a packed"), (data[:4] + b"\x07\0\0\0" + data[8:], "version"),
                       (data[:4] + b"\x01\0\x02\0" + data[8:], "version"),
                       (data[:28] + b"\x04\0\0\0" + data[32:], "flags")):
        bad.write_bytes(edit)
        with pytest.raises(ValueError, match=what):
            packedfile.open_frames(str(bad))


class _Counting:
    def __init__(self, f):
        self.f, self.reads = f, []

    def read(self, n=-1):
        self.reads.append(n)
        return self.f.read(n)


def test_no_read_exceeds_a_frame_record(tmp_path):
    frames = _gop(True, True, rc=True)
    path = tmp_path / "gop.sopk"
    packedfile.write_frames(str(path), H, W, BS, NB, "varint", frames, chroma_qp_offset=0)
    largest = max(len(f["payload"]) + len(f["chroma_payload"]) + 5 * NB + 16 for f in frames)
    with open(path, "rb") as fh:
        c = _Counting(fh)
        hdr, it = packedfile.open_frames(c)
        assert sum(1 for _ in it) == len(frames)
        assert not fh.closed                               # a caller's file object stays the caller's
    assert c.reads and min(c.reads) >= 0 and max(c.reads) <= largest
    assert sum(c.reads) <= path.stat().st_size + 1         # every byte once, and the probe behind the last frame
