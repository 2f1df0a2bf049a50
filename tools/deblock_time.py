"""What the deblocking post-filter costs on one MI355X.  From one run, one JSON line:

  kernel   so_deblock_yuv420 on one 4:2:0 frame at 2160 x 3840 and at 1088 x 1920 (1080p in its padded
           planes), split flags random, a QP map of 4..8: every launch between its own device events,
           alternating launch by launch with so_copy_d2d of the same three planes (the floor a
           filter that reads and writes every sample can approach); median, min, the spread of the
           middle 80 %, the ratio of the medians, and the bytes moved (1.5 read + 1.5 written per luma
           sample) over the median.  The frames rotate through a set of --frames different ones, so
           a launch does not find its input in a cache the launch before it filled.  A single launch
           between events includes the host's enqueue; "batch" is the same frames as one launch
           (replayed from a captured graph) against two copies of the whole stacks, per frame: the
           device time.
  stream   hostdecode.HostStreamDecoder.decode_file of a packed 4K 4:2:0 file (--gop frames, VBS on),
           file in, host frames out, host clock between two device synchronisations, deblock off and
           on alternating after two warm-up rounds.  --off-only times the off side alone: run with
           SO_LIB_PATH naming a build of the parent commit, it gives the parent's numbers on the
           same machine; --label names that library in the record.

    python tools/deblock_time.py [--reps 60] [--pairs 7] [--gop 8] [--dir DIR] [--skip-stream] [--off-only]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def spread(ts):
    """(max - min) / median of the middle 80 %"""
    s = sorted(ts)
    k = len(s) // 10
    s = s[k:len(s) - k] if len(s) > 2 * k else s
    return round((s[-1] - s[0]) / statistics.median(s), 4)


def stats(ts, unit=1.0):
    return {"median": round(unit * statistics.median(ts), 3), "min": round(unit * min(ts), 3), "spread": spread(ts)}


def evented(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_case(dev, h, w, nframes, reps, warmup):
    from streamoptima_amd import _lib
    from streamoptima_amd.engine import Engine
    eng = Engine(h, w, 16, device=dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    y = torch.randint(0, 256, (nframes, h, w), dtype=torch.uint8, generator=g).to(dev)
    uv = torch.randint(0, 256, (nframes, 2, h // 2, w // 2), dtype=torch.uint8, generator=g).to(dev)
    split = torch.randint(0, 2, (nframes, eng.nb), dtype=torch.uint8, generator=g).to(dev)
    qmap = torch.randint(4, 9, (nframes, eng.nb), dtype=torch.int32, generator=g).to(dev)
    oy, ouv = torch.empty_like(y), torch.empty_like(uv)
    sh = _lib.stream_handle(dev)
    state = {"i": 0}

    def filt():
        i = state["i"] = (state["i"] + 1) % nframes
        eng.deblock_yuv420(y[i:i + 1], uv[i:i + 1], split=split[i:i + 1], qp_maps=qmap[i:i + 1], out_y=oy[i:i + 1],
                           out_uv=ouv[i:i + 1])

    def copy():
        i = state["i"] = (state["i"] + 1) % nframes
        for dst, src in ((oy[i], y[i]), (ouv[i, 0], uv[i, 0]), (ouv[i, 1], uv[i, 1])):
            _lib.check(eng.lib.so_copy_d2d(dst.data_ptr(), src.data_ptr(), src.numel(), sh), "so_copy_d2d")
    for _ in range(warmup):
        filt()
        copy()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(reps):
        tf.append(evented(filt))
        tc.append(evented(copy))
    # the same frames as ONE launch (a batch is one grid) against two copies of the whole stacks: no
    # host enqueue between frames, so this is the device time; per frame
    def filt_batch():
        eng.deblock_yuv420(y, uv, split=split, qp_maps=qmap, out_y=oy, out_uv=ouv)

    def copy_batch():
        for dst, src in ((oy, y), (ouv, uv)):
            _lib.check(eng.lib.so_copy_d2d(dst.data_ptr(), src.data_ptr(), src.numel(), sh), "so_copy_d2d")
    for _ in range(2):
        filt_batch()
        copy_batch()
    torch.cuda.synchronize()
    # The filter is replayed from a captured graph: the host's work in the call (pointer arrays,
    # checks: more than the kernel's time) is then not in the window.  The copies are two plain calls
    # with next to no host work; replayed from a graph their events gave rates above the HBM peak
    # (copy nodes are not bracketed by the events the way kernels are), so they are not captured.
    gf = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gf):
        filt_batch()
    for _ in range(3):
        gf.replay()
        copy_batch()
    torch.cuda.synchronize()
    bf, bc = [], []
    for _ in range(max(reps // 2, 5)):
        bf.append(evented(gf.replay) / nframes)
        bc.append(evented(copy_batch) / nframes)
    nbytes = 3 * h * w          # 1.5 read, 1.5 written per luma sample
    mf, mc = statistics.median(tf), statistics.median(tc)
    mbf, mbc = statistics.median(bf), statistics.median(bc)
    return {"plane": [h, w], "bytes_moved": nbytes, "filter_us": stats(tf, 1e3), "copy_d2d_us": stats(tc, 1e3),
            "filter_over_copy": round(mf / mc, 3), "batch_frames": nframes,
            "batch_filter_us_per_frame": stats(bf, 1e3), "batch_copy_us_per_frame": stats(bc, 1e3),
            "batch_filter_over_copy": round(mbf / mbc, 3), "batch_filter_bytes_per_s": round(nbytes / (1e-3 * mbf), 0),
            "batch_copy_bytes_per_s": round(nbytes / (1e-3 * mbc), 0)}


def write_file(dev, path, frames):
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.synth import synth_sequence_torch
    from streamoptima_amd.workloads import WORKLOADS
    c = WORKLOADS["4k"]
    h, w = c["h"], c["w"]
    y = synth_sequence_torch(frames, h, w, seed=c["seed"], device=dev).cpu().numpy()
    uv = torch.stack([synth_sequence_torch(frames, h // 2, w // 2, seed=c["seed"] + 1 + p, device=dev) for p in range(2)],
                     dim=1).cpu().numpy()
    cwd = os.getcwd()
    os.chdir(os.path.dirname(path))
    try:
        enc = Y_Video_codec(h, w, frames, 16, 16, c["qp"], frames, 0, 0.015, True, y_only_frame_arr=y, device=dev,
                            chroma=True, chroma_qp_offset=0, uv_frame_arr=uv)
        enc.encode()
        size = enc.transmit_packed420(path)
    finally:
        os.chdir(cwd)
    return {"h": h, "w": w, "frames": frames, "qp": c["qp"], "bytes": size}


def stream_case(dev, path, meta, pairs, off_only, label):
    from streamoptima_amd.decoder import decoder
    from streamoptima_amd.hostdecode import HostStreamDecoder
    sides = {}
    for name, on in (("off", False),) + ((() if off_only else (("on", True),))):
        dec = decoder(0, meta["frames"], 16, meta["frames"], meta["h"], meta["w"], meta["qp"], 1, False, 0.015, True,
                      device=dev, **({"deblock": True} if on else {}))
        sides[name] = HostStreamDecoder(dec, chunk=2, nbuf=2)

    def run(hs):
        n = [0]

        def consume(i, y, u, v):
            n[0] += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hs.decode_file(path, consume)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert n[0] == meta["frames"]
        return 1e3 * dt / meta["frames"]
    for _ in range(2):
        for hs in sides.values():
            run(hs)
    ts = {k: [] for k in sides}
    for _ in range(pairs):
        for k, hs in sides.items():
            ts[k].append(run(hs))
    out = {"unit": "ms per frame, file to host frames", "file": meta, "lib": label}
    out.update({k: dict(stats(v), all=[round(t, 3) for t in v]) for k, v in ts.items()})
    if "on" in ts:
        out["on_over_off"] = round(statistics.median(ts["on"]) / statistics.median(ts["off"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--frames", type=int, default=12, help="different frames the kernel launches rotate through")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--gop", type=int, default=8, help="frames of the 4K file of the stream comparison")
    ap.add_argument("--dir", default=None, help="where the 4K file is kept (written when missing)")
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--label", default=None, help="what the record calls the library under test (default: the file "
                                                  "name SO_LIB_PATH gives, or \"in-tree\")")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deblock_time.py needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    out = {"tool": "deblock_time", "reps": a.reps}
    if not a.skip_kernel:
        out["kernel_4k"] = kernel_case(dev, 2160, 3840, a.frames, a.reps, a.warmup)
        out["kernel_1080p"] = kernel_case(dev, 1088, 1920, a.frames, a.reps, a.warmup)
    if not a.skip_stream:
        d = a.dir or tempfile.mkdtemp(prefix="deblock_time_")
        os.makedirs(d, exist_ok=True)
        path, side = os.path.join(os.path.abspath(d), "gop420_4k.sopk"), os.path.join(os.path.abspath(d), "gop420_4k.json")
        if not (os.path.exists(path) and os.path.exists(side)):
            meta = write_file(dev, path, a.gop)
            json.dump(meta, open(side, "w"))
        meta = json.load(open(side))
        out["stream_4k"] = stream_case(dev, path, meta, a.pairs, a.off_only,
                                       a.label or os.path.basename(os.environ.get("SO_LIB_PATH", "")) or "in-tree")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
