"""What chroma costs the host-to-host stream (BASELINE.md section 4's region): the 4K 30-frame
configs[2] GOP through hoststream.HostStreamEncoder with chroma=False and chroma=True,
alternating, in one process.
    python tools/stream_chroma_time.py [--pairs 7] [--out FILE]
Pinned host planes in (hostmem.pinned_empty, as bench.py's region and tools/s4_probe.py's
finding: registered anonymous memory first touched by this process), packed payloads back in
pinned host memory; each call timed from a synchronised device to a synchronised device.  Two
untimed calls of each encoder warm the path.  The H2D link rate is measured in the same session:
the luma GOP's pinned planes up alone (copy engine, no kernel), best of the repeats.
Prints one JSON line: per encoder the times, their median and spread (max - min), the upload
bytes and the upload fraction (upload bytes / median time, against the link rate); then the
expectation -- chroma-on median <= 1.5 x luma-only median + luma-only spread, and an upload
fraction no lower than luma-only's by more than that spread's share of the luma-only median --
and whether it held."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.pairs < 7:
        ap.error("--pairs: at least 7")
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.hostmem import pinned_empty
    from streamoptima_amd.hoststream import HostStreamEncoder
    from streamoptima_amd.synth import synth_sequence_torch
    from streamoptima_amd.workloads import WORKLOADS
    cfg = WORKLOADS["4k"]
    dev = torch.device("cuda:0")
    h, w, f, intra = cfg["h"], cfg["w"], cfg["frames"], cfg["intra_dur"]
    y_host = pinned_empty((f, h, w))
    y_host.copy_(synth_sequence_torch(f, h, w, seed=cfg["seed"], device=dev).cpu())
    uv_host = pinned_empty((f, 2, h // 2, w // 2))
    for p in range(2):
        uv_host[:, p].copy_(synth_sequence_torch(f, h // 2, w // 2, seed=cfg["seed"] + 1 + p, device=dev).cpu())
    enc = {}
    for chroma in (False, True):
        c = Y_Video_codec(h, w, f, 16, 16, cfg["qp"], intra, 0, 0.015, False, chroma=chroma, device=dev)
        enc[chroma] = HostStreamEncoder(c, f, chunk=2)

    def run(chroma):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = enc[chroma].encode(y_host, intra, uv_host=uv_host if chroma else None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, sum(r["bytes"])

    for _ in range(2):
        for chroma in (False, True):
            run(chroma)
    ts, down = {False: [], True: []}, {}
    for _ in range(a.pairs):
        for chroma in (False, True):
            t, down[chroma] = run(chroma)
            ts[chroma].append(t)

    dst = enc[False].frames_dev
    rates = []
    for _ in range(a.pairs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(y_host, non_blocking=True)
        torch.cuda.synchronize()
        rates.append(y_host.numel() / (time.perf_counter() - t0) / 1e9)
    link = max(rates[1:])

    up = {False: y_host.numel(), True: y_host.numel() + uv_host.numel()}
    rec = {}
    for chroma in (False, True):
        med = statistics.median(ts[chroma])
        rec["chroma_on" if chroma else "luma_only"] = {
            "ms": [round(t, 3) for t in ts[chroma]], "median_ms": round(med, 3),
            "spread_ms": round(max(ts[chroma]) - min(ts[chroma]), 3), "upload_bytes": up[chroma],
            "download_bytes": down[chroma], "upload_gbs": round(up[chroma] / med / 1e6, 2),
            "h2d_frac": round(up[chroma] / med / 1e6 / link, 4)}
    lo, on = rec["luma_only"], rec["chroma_on"]
    bound = 1.5 * lo["median_ms"] + lo["spread_ms"]
    frac_floor = lo["h2d_frac"] * (1 - lo["spread_ms"] / lo["median_ms"])
    line = {"workload": cfg["workload"], "pairs": a.pairs, "h2d_link_gbs": round(link, 2),
            "upload_ratio": round(up[True] / up[False], 4), **rec,
            "expectation": {"time_bound_ms": round(bound, 3), "time_ok": on["median_ms"] <= bound,
                            "h2d_frac_floor": round(frac_floor, 4), "frac_ok": on["h2d_frac"] >= frac_floor,
                            "ratio": round(on["median_ms"] / lo["median_ms"], 4)}}
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
