"""Time the colour conversion on one MI355X at 2160 x 3840.  From one run:

  * each direction and layout (so_rgb_to_yuv420 / so_yuv420_to_rgb, hwc and chw), one frame per
    launch: the median of individually evented launches, warmed, and two chains of 30 launches
    replayed from a captured graph, per launch (the device time without the host's enqueue cost)
    -- "chain": the same frame 30 times, 37 MB that stay in the 256 MiB Infinity Cache, so what
    the kernel does when memory is not the limit; "stream": 30 different frames, 1.1 GB per
    replay, so every byte comes from and goes to HBM -- with the bytes moved, computed from the
    shapes (4.5 B per pixel: 3 on the RGB side, 1.5 on the planes'), over that time and over the
    8 TB/s HBM peak; and those 30 frames as one batched launch, evented, per frame;
  * the same arithmetic written as torch ops on the same device (what a user has to do today),
    alternating with the kernel launch by launch, its output checked equal;
  * the host-to-host region (hoststream.HostStreamEncoder.encode: pinned frames in, packed bytes in
    host memory out) of the 4K 30-frame GOP with input="rgb" against input="yuv420", the planes of
    the latter being the conversion of the former's pictures, alternating.

Prints one JSON line; DESIGN.md "Colour conversion" quotes it.

    python tools/colour_time.py [--reps 40] [--gop-reps 6] [--warmup 5] [--no-stream]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from streamoptima_amd.Encoder import Y_Video_codec  # noqa: E402
from streamoptima_amd.colour import Colour  # noqa: E402
from streamoptima_amd.synth import synth_sequence_torch  # noqa: E402
from streamoptima_amd.workloads import WORKLOADS  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X
# BT.709 limited range, the usual tables of 4K material (include/streamoptima.h)
FWD = [[11966, 40254, 4064], [-6596, -22188, 28784], [28784, -26145, -2639]]
INV = [[76309, 0, 117489], [76309, -13975, -34925], [76309, 138438, 0]]
YOFF = 16


def torch_forward(rgb, layout, f):
    """rgb uint8 [1, h, w, 3] or [1, 3, h, w] -> (y [1, h, w], uv [1, 2, h/2, w/2]), as torch ops"""
    p = rgb.to(torch.int32)
    r, g, b = (p[..., 0], p[..., 1], p[..., 2]) if layout == "hwc" else (p[:, 0], p[:, 1], p[:, 2])
    y = ((f[0][0] * r + f[0][1] * g + f[0][2] * b + ((YOFF << 16) + 32768)) >> 16).clamp_(0, 255).to(torch.uint8)

    def cell(c):
        return c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2]
    sr, sg, sb = cell(r), cell(g), cell(b)
    uv = torch.stack([((f[k][0] * sr + f[k][1] * sg + f[k][2] * sb + ((128 << 18) + (1 << 17))) >> 18).clamp_(0, 255)
                      for k in (1, 2)], dim=1).to(torch.uint8)
    return y, uv


def torch_inverse(y, uv, layout, j):
    yy = y.to(torch.int32) - YOFF
    c = uv.to(torch.int32) - 128
    c = c.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    ch = [((j[k][0] * yy + j[k][1] * c[:, 0] + j[k][2] * c[:, 1] + 32768) >> 16).clamp_(0, 255) for k in range(3)]
    return torch.stack(ch, dim=-1 if layout == "hwc" else 1).to(torch.uint8)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--gop-reps", type=int, default=6)
    ap.add_argument("--no-stream", action="store_true", help="skip the host-to-host region")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("colour_time.py needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    cfg = WORKLOADS["4k"]
    h, w, f = cfg["h"], cfg["w"], cfg["frames"]
    col = Colour("bt709", False)
    codec = Y_Video_codec(h, w, f, 16, 16, cfg["qp"], cfg["intra_dur"], 0, 0.015, False, device=dev, chroma=True,
                          colour=col)
    eng = codec.engine()
    assert (eng.h, eng.w) == (h, w)
    rgb_all = torch.stack([synth_sequence_torch(f, h, w, seed=cfg["seed"] + c, device=dev) for c in range(3)], dim=-1)
    nbytes = h * w * 3 + h * w * 3 // 2
    out = {"tool": "colour_time", "height": h, "width": w, "reps": a.reps, "bytes_per_frame": nbytes,
           "floor_us_at_hbm_peak": round(1e6 * nbytes / HBM_PEAK, 2)}
    fwd_t = FWD   # the forward table the torch baseline multiplies by
    for layout in ("hwc", "chw"):
        rgb = rgb_all[:1].contiguous() if layout == "hwc" else rgb_all[:1].permute(0, 3, 1, 2).contiguous()
        y, uv = eng.rgb_to_yuv420(rgb, col, layout)
        back = eng.yuv420_to_rgb(y, uv, h, w, col, layout)
        ty, tuv = torch_forward(rgb, layout, fwd_t)
        assert torch.equal(ty, y) and torch.equal(tuv, uv), "torch forward differs from the kernel"
        assert torch.equal(torch_inverse(y, uv, layout, INV), back), "torch inverse differs from the kernel"
        # 30 different frames, one launch each: nothing is served twice from a cache
        rgb_seq = rgb_all if layout == "hwc" else rgb_all.permute(0, 3, 1, 2).contiguous()
        y_seq, uv_seq = eng.rgb_to_yuv420(rgb_seq, col, layout)
        back_seq = torch.empty_like(rgb_seq)

        def stream_forward():
            for i in range(f):
                eng.rgb_to_yuv420(rgb_seq[i:i + 1], col, layout, out_y=y_seq[i:i + 1], out_uv=uv_seq[i:i + 1])

        def stream_inverse():
            for i in range(f):
                eng.yuv420_to_rgb(y_seq[i:i + 1], uv_seq[i:i + 1], h, w, col, layout, out=back_seq[i:i + 1])
        cases = {
            "forward": (lambda: eng.rgb_to_yuv420(rgb, col, layout, out_y=y, out_uv=uv),
                        lambda: torch_forward(rgb, layout, fwd_t), stream_forward),
            "inverse": (lambda: eng.yuv420_to_rgb(y, uv, h, w, col, layout, out=back),
                        lambda: torch_inverse(y, uv, layout, INV), stream_inverse),
        }
        for name, (kernel, baseline, stream) in cases.items():
            tk, tt = evented_pair(kernel, baseline, a.warmup, a.reps)
            kernel()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(30):
                    kernel()
            stream()
            torch.cuda.synchronize()
            sgraph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(sgraph):
                stream()
            tg, ts = evented_pair(graph.replay, sgraph.replay, a.warmup, a.reps)
            # the same 30 frames as ONE launch (a batch is one grid): no launch between frames
            batch = ((lambda: eng.rgb_to_yuv420(rgb_seq, col, layout, out_y=y_seq, out_uv=uv_seq)) if name == "forward"
                     else (lambda: eng.yuv420_to_rgb(y_seq, uv_seq, h, w, col, layout, out=back_seq)))
            tb, _ = evented_pair(batch, lambda: None, a.warmup, a.reps)
            bat = statistics.median(tb) / f
            med, chain, strm = statistics.median(tk), statistics.median(tg) / 30, statistics.median(ts) / f
            out[f"{name}_{layout}"] = {
                "launch_us": round(1e3 * med, 2), "launch_us_min": round(1e3 * min(tk), 2), "launch_spread": spread(tk),
                "chain_us_per_launch": round(1e3 * chain, 2), "chain_us_per_launch_min": round(1e3 * min(tg) / 30, 2),
                "chain_spread": spread(tg),
                "chain_bytes_per_s": round(nbytes / (1e-3 * chain), 0),
                "chain_share_of_hbm_peak": round(nbytes / (1e-3 * chain) / HBM_PEAK, 4),
                "stream_us_per_launch": round(1e3 * strm, 2), "stream_us_per_launch_min": round(1e3 * min(ts) / f, 2),
                "stream_spread": spread(ts), "stream_bytes_per_s": round(nbytes / (1e-3 * strm), 0),
                "stream_share_of_hbm_peak": round(nbytes / (1e-3 * strm) / HBM_PEAK, 4),
                "batch_us_per_frame": round(1e3 * bat, 2), "batch_us_per_frame_min": round(1e3 * min(tb) / f, 2),
                "batch_spread": spread(tb), "batch_share_of_hbm_peak": round(nbytes / (1e-3 * bat) / HBM_PEAK, 4),
                "torch_us": round(1e3 * statistics.median(tt), 2), "torch_us_min": round(1e3 * min(tt), 2),
            }

    if not a.no_stream:
        from streamoptima_amd.hoststream import HostStreamEncoder
        rgb_host = rgb_all.cpu().pin_memory()
        y, uv = eng.rgb_to_yuv420(rgb_all, col)
        y_host, uv_host = y.cpu().pin_memory(), uv.cpu().pin_memory()
        del rgb_all, rgb_seq, y_seq, uv_seq, back_seq
        enc = {"rgb": HostStreamEncoder(codec, f, input="rgb"), "yuv420": HostStreamEncoder(codec, f)}
        args = {"rgb": (rgb_host,), "yuv420": (y_host,)}
        kw = {"rgb": {}, "yuv420": {"uv_host": uv_host}}
        times, nb = {"rgb": [], "yuv420": []}, {}
        for rep in range(a.gop_reps + 2):
            for k in ("yuv420", "rgb"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = enc[k].encode(*args[k], cfg["intra_dur"], **kw[k])
                dt = time.perf_counter() - t0
                nb[k] = res["bytes"]
                if rep >= 2:             # two warm-up GOPs each
                    times[k].append(1e3 * dt)
        assert nb["rgb"] == nb["yuv420"], "the two inputs gave different streams"
        for k in times:
            out[f"host_to_host_ms_{k}"] = round(statistics.median(times[k]), 3)
            out[f"host_to_host_ms_{k}_min"] = round(min(times[k]), 3)
            out[f"host_to_host_spread_{k}"] = spread(times[k])
        out["upload_bytes_rgb"] = f * h * w * 3
        out["upload_bytes_yuv420"] = f * h * w * 3 // 2
    print(json.dumps(out))


if __name__ == "__main__":
    main()
