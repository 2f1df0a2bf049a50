"""Time the resampler on one MI355X: 30 frames of 4:2:0, 3840 x 2160 -> 1920 x 1080 and back, for
each filter.  From one run, per case:

  * so_scale_yuv420 on the whole batch (one launch), replayed from a captured graph between events,
    warmed (the device time, without the host's preparation of 180 plane pointers): microseconds per
    frame and the bytes it has to move (the source's picture read once, the destination written
    once) per second; and the same call issued from Python, host cost included ("call").  The 30
    source frames are 373 MB (4K) or 93 MB (1080p), the destinations the other way round: more
    than the 256 MiB Infinity Cache holds;
  * so_copy_d2d of as many bytes read and written in all, in the same run, alternating: the floor;
  * the same planes through torch.nn.functional.interpolate (float32, bicubic, antialias=True, with
    the conversions to float and back to uint8): what a user does without the kernel;
  * the host-to-host region (hoststream.HostStreamEncoder.encode: pinned frames in, packed bytes in
    host memory out) of a 30-frame GOP coded at 1080p from a 4K source (source_size) against the
    same region fed 1080p planes, alternating, and the time the larger upload alone takes.

Prints one JSON line; DESIGN.md "Scaling" quotes it.

    python tools/scale_time.py [--reps 20] [--gop-reps 4] [--warmup 3] [--no-stream]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from streamoptima_amd import _lib  # noqa: E402
from streamoptima_amd.Encoder import Y_Video_codec  # noqa: E402
from streamoptima_amd.engine import Engine  # noqa: E402
from streamoptima_amd.scale import ScalePlan  # noqa: E402
from streamoptima_amd.synth import synth_sequence_torch  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X
FRAMES = 30
SIZES = {"4k_to_1080p": ((2160, 3840), (1080, 1920)), "1080p_to_4k": ((1080, 1920), (2160, 3840))}


def evented_pair(fa, fb, warmup, reps):
    """milliseconds of each of `reps` calls of fa and of fb, alternating, every call between its own events"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for times, fn in ((ta, fa), (tb, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
    return ta, tb


def spread(ts):
    """(max - min) / median of the middle 80 %"""
    s = sorted(ts)
    k = len(s) // 10
    s = s[k:len(s) - k] if len(s) > 2 * k else s
    return round((s[-1] - s[0]) / statistics.median(s), 4)


def torch_resize(y, uv, dst):
    def one(p, hw):
        return F.interpolate(p.to(torch.float32), size=hw, mode="bicubic", antialias=True).round_().clamp_(0, 255).to(torch.uint8)
    return one(y[:, None], dst), one(uv, (dst[0] // 2, dst[1] // 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gop-reps", type=int, default=4)
    ap.add_argument("--no-stream", action="store_true", help="skip the host-to-host region")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scale_time.py needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    eng = Engine(64, 128, 16, 16, device=dev)      # the launches below name their planes: any engine serves
    lib = eng.lib
    out = {"tool": "scale_time", "frames": FRAMES, "reps": a.reps}
    for name, (src, dst) in SIZES.items():
        y = synth_sequence_torch(FRAMES, src[0], src[1], seed=3, device=dev)
        uv = torch.stack([synth_sequence_torch(FRAMES, src[0] // 2, src[1] // 2, seed=4 + c, device=dev) for c in range(2)], dim=1)
        oy = torch.empty((FRAMES, *dst), dtype=torch.uint8, device=dev)
        ouv = torch.empty((FRAMES, 2, dst[0] // 2, dst[1] // 2), dtype=torch.uint8, device=dev)
        nbytes = (src[0] * src[1] + dst[0] * dst[1]) * 3 // 2          # per frame, read + written
        half = FRAMES * nbytes // 2                                    # a copy of this reads and writes as much in all
        ca = torch.empty(half, dtype=torch.uint8, device=dev)
        cb = torch.empty(half, dtype=torch.uint8, device=dev)

        def copy():
            _lib.check(lib.so_copy_d2d(cb.data_ptr(), ca.data_ptr(), half, _lib.stream_handle(dev)), "so_copy_d2d")
        tt, _ = evented_pair(lambda: torch_resize(y, uv, dst), lambda: None, 1, max(3, a.reps // 4))
        case = {"bytes_per_frame": nbytes, "floor_us_per_frame_at_hbm_peak": round(1e6 * nbytes / HBM_PEAK, 2),
                "torch_bicubic_us_per_frame": round(1e3 * statistics.median(tt) / FRAMES, 2),
                "torch_bicubic_us_per_frame_min": round(1e3 * min(tt) / FRAMES, 2)}
        torch.cuda.empty_cache()
        for filt in ("bilinear", "bicubic", "lanczos3"):
            plan = ScalePlan(src, dst, filt, device=dev)

            def kernel():
                eng.scale_yuv420(y, uv, plan, out_y=oy, out_uv=ouv, out_hw=dst)
            tcall, _ = evented_pair(kernel, lambda: None, a.warmup, a.reps)
            graphs = []
            for fn in (kernel, copy):
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    fn()
                graphs.append(gr)
            tk, tc = evented_pair(graphs[0].replay, graphs[1].replay, a.warmup, a.reps)
            k, c = statistics.median(tk) / FRAMES, statistics.median(tc) / FRAMES
            case[filt] = {"call_us_per_frame": round(1e3 * statistics.median(tcall) / FRAMES, 2),
                          "us_per_frame": round(1e3 * k, 2), "us_per_frame_min": round(1e3 * min(tk) / FRAMES, 2),
                          "spread": spread(tk), "bytes_per_s": round(nbytes / (1e-3 * k), 0),
                          "share_of_hbm_peak": round(nbytes / (1e-3 * k) / HBM_PEAK, 4),
                          "copy_us_per_frame": round(1e3 * c, 2), "copy_bytes_per_s": round(nbytes / (1e-3 * c), 0),
                          "taps": [t[2] for t in plan.tables]}
        out[name] = case
        del y, uv, oy, ouv, ca, cb
        torch.cuda.empty_cache()

    if not a.no_stream:
        from streamoptima_amd.hoststream import HostStreamEncoder
        (hs, ws), (h, w) = SIZES["4k_to_1080p"]
        codec = Y_Video_codec(h, w, FRAMES, 16, 16, 4, FRAMES, 0, 0.015, False, device=dev, chroma=True)
        e = codec.engine()
        y4 = synth_sequence_torch(FRAMES, hs, ws, seed=3, device=dev)
        uv4 = torch.stack([synth_sequence_torch(FRAMES, hs // 2, ws // 2, seed=4 + c, device=dev) for c in range(2)], dim=1)
        plan = ScalePlan((hs, ws), (h, w), "lanczos3", device=dev)
        y2, uv2 = e.scale_yuv420(y4, uv4, plan)                        # the 1080p planes the native encoder is fed
        hosts = {"scaled": (y4.cpu().pin_memory(), uv4.cpu().pin_memory()), "native": (y2.cpu().pin_memory(), uv2.cpu().pin_memory())}
        del y4, uv4, y2, uv2
        enc = {"scaled": HostStreamEncoder(codec, FRAMES, source_size=(hs, ws)), "native": HostStreamEncoder(codec, FRAMES)}
        times, nb = {"scaled": [], "native": []}, {}
        for rep in range(a.gop_reps + 2):
            for k in ("native", "scaled"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = enc[k].encode(hosts[k][0], FRAMES, uv_host=hosts[k][1])
                dt = time.perf_counter() - t0
                nb[k] = res["bytes"]
                if rep >= 2:             # two warm-up GOPs each
                    times[k].append(1e3 * dt)
        assert nb["scaled"] == nb["native"], "the two inputs gave different streams"
        for k in times:
            out[f"host_to_host_ms_{k}"] = round(statistics.median(times[k]), 3)
            out[f"host_to_host_ms_{k}_min"] = round(min(times[k]), 3)
            out[f"host_to_host_spread_{k}"] = spread(times[k])
        # the larger source's upload alone: what no schedule can go below
        b = enc["scaled"].bufs[0]
        ups = []
        for _ in range(a.gop_reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.src_y.copy_(hosts["scaled"][0], non_blocking=True)
            b.src_uv.copy_(hosts["scaled"][1], non_blocking=True)
            torch.cuda.synchronize()
            ups.append(1e3 * (time.perf_counter() - t0))
        out["upload_ms_scaled_source"] = round(statistics.median(ups[1:]), 3)
        out["upload_bytes_scaled"] = FRAMES * hs * ws * 3 // 2
        out["upload_bytes_native"] = FRAMES * e.h * e.w * 3 // 2
    print(json.dumps(out))


if __name__ == "__main__":
    main()
