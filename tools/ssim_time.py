"""Time so_ssim_u8 on one MI355X: a batch of 2160 x 3840 plane pairs (default thirty), the
median of individually evented calls, next to one so_sse_u8 call over the same planes (the same
bytes read once: the memory-bound yardstick).  Prints one JSON line; DESIGN.md "Device SSIM" quotes it.

    python tools/ssim_time.py [--frames 30] [--height 2160] [--width 3840] [--win 11] [--reps 40]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from streamoptima_amd import _lib  # noqa: E402
from streamoptima_amd.engine import Engine, alloc_planes  # noqa: E402
from streamoptima_amd.synth import synth_sequence_torch  # noqa: E402


def evented(fn, warmup, reps):
    """milliseconds of each of `reps` calls of fn, every one between its own pair of events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--win", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_time.py needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    n, h, w = a.frames, a.height, a.width
    eng = Engine(h, w, 16, 16, False, 0.015, dev)
    src = synth_sequence_torch(n, h, w, seed=3, device=dev)
    x = alloc_planes(n, h, w, dev)
    x.copy_(src)
    # a reconstruction-like second plane: the frame with a small deterministic error
    y = alloc_planes(n, h, w, dev)
    noise = torch.randint(-3, 4, (n, h, w), dtype=torch.int16, device=dev,
                          generator=torch.Generator(device=dev).manual_seed(5))
    y.copy_((src.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8))
    del src, noise
    xs, ys = list(x), list(y)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    acc = torch.zeros(1, dtype=torch.int64, device=dev)

    def ssim():
        eng.ssim(xs, ys, h, w, win=a.win, out=out)

    def sse():   # one call over the batch (the planes lie back to back): device time, not launch rate
        eng.sse_into(x, y, acc)
    t_ssim = evented(ssim, a.warmup, a.reps)
    t_sse = evented(sse, a.warmup, a.reps)
    first = out.cpu()
    ssim()
    assert torch.equal(first, out.cpu()), "so_ssim_u8 is not reproducible"
    med_ssim, med_sse = statistics.median(t_ssim), statistics.median(t_sse)
    bytes_per_frame = 2 * h * w
    print(json.dumps({
        "tool": "ssim_time", "frames": n, "height": h, "width": w, "win": a.win, "reps": a.reps,
        "ssim_us_per_frame": round(1e3 * med_ssim / n, 3), "ssim_us_per_frame_min": round(1e3 * min(t_ssim) / n, 3),
        "sse_us_per_frame": round(1e3 * med_sse / n, 3), "sse_us_per_frame_min": round(1e3 * min(t_sse) / n, 3),
        "ratio_to_sse": round(med_ssim / med_sse, 3),
        "ssim_bytes_per_s": round(bytes_per_frame * n / (1e-3 * med_ssim), 0),
        "sse_bytes_per_s": round(bytes_per_frame * n / (1e-3 * med_sse), 0),
        "ssim_mean": float(first.mean()), "workspace_doubles": int(_lib.load().so_ssim_workspace_elems(n, h, w, a.win)),
    }))


if __name__ == "__main__":
    main()
