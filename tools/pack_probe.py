"""Time the packed stream's packer (and the D2H of its stream) on a 4K 30-frame GOP's symbols.
    python tools/pack_probe.py [--frames 30] [--reps 5] [--coding {varint,bits} ...]
--coding varint: so_pack_frames_ex (the default); bits: so_pack_frames_bits; "--coding varint bits":
the two on the same symbols in one process, their timed calls interleaved.  One JSON line per coding.
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
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
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--coding", nargs="+", choices=("varint", "bits"), default=["varint"])
    a = ap.parse_args()
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.engine import alloc_planes
    from streamoptima_amd.synth import synth_sequence_torch
    dev = torch.device("cuda:0")
    h, w, f = 2160, 3840, a.frames
    c = Y_Video_codec(h, w, f, 16, 16, 4, f, 0, 0.015, False, device=dev)
    fr = alloc_planes(f, h, w, dev)
    fr.copy_(synth_sequence_torch(f, h, w, seed=0, device=dev))
    syms = c.encode_device(fr, f)["symbols"]
    eng = c.engine()
    bufs = {cd: eng.pack_symbols(syms, coding=cd) for cd in a.coding}     # also the warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {cd: [] for cd in a.coding}
    for _ in range(a.reps):
        for cd in a.coding:                       # every call between its own pair of events
            e0.record()
            eng.pack_symbols(syms, *bufs[cd], coding=cd)
            e1.record()
            torch.cuda.synchronize()
            ts[cd].append(e0.elapsed_time(e1))
    qtc_h = torch.empty((f,) + tuple(syms[0].qtc.shape), dtype=torch.int16).pin_memory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, s in enumerate(syms):
        qtc_h[i].copy_(s.qtc, non_blocking=True)
    torch.cuda.synchronize()
    d2h_dense = time.perf_counter() - t0
    for cd in a.coding:
        offs, out = bufs[cd]
        tot = offs[:, eng.nb].cpu().tolist()
        host = torch.empty((f, max(tot)), dtype=torch.uint8).pin_memory()
        d2hs = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, n in enumerate(tot):
                host[i, :n].copy_(out[i, :n], non_blocking=True)
            torch.cuda.synchronize()
            d2hs.append(time.perf_counter() - t0)
        d2h = statistics.median(d2hs)
        print(json.dumps({"coding": cd, "pack_ms": [round(t, 3) for t in ts[cd]],
                          "pack_ms_median": round(statistics.median(ts[cd]), 3), "packed_bytes": sum(tot),
                          "bytes_per_frame": round(sum(tot) / f), "bytes_i_frame": tot[0],
                          "bytes_per_p_frame": round(sum(tot[1:]) / max(1, f - 1)),
                          "d2h_packed_ms": round(d2h * 1e3, 3), "d2h_packed_gbs": round(sum(tot) / d2h / 1e9, 2),
                          "d2h_qtc_ms": round(d2h_dense * 1e3, 3),
                          "d2h_qtc_gbs": round(qtc_h.numel() * 2 / d2h_dense / 1e9, 2)}))


if __name__ == "__main__":
    main()
