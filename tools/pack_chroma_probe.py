"""Size and time of the packed chroma stream on a 4K 30-frame GOP encoded with chroma on, next to
the luma stream of the same GOP in the same process.
    python tools/pack_chroma_probe.py [--frames 30] [--reps 9]
Every timed call sits between its own pair of device events, the four packers (luma and chroma,
varint and bits) interleaved.  One JSON line per coding: bytes per frame (packed chroma, dense
qtc_u + qtc_v, packed luma), the median call times, and nanoseconds per coefficient -- the luma
packers' figure is the yardstick (chroma has half the coefficients of luma)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.engine import alloc_planes
    from streamoptima_amd.synth import synth_sequence_torch
    dev = torch.device("cuda:0")
    h, w, f = 2160, 3840, a.frames
    c = Y_Video_codec(h, w, f, 16, 16, 4, f, 0, 0.015, False, chroma=True, device=dev)
    fr = alloc_planes(f, h, w, dev)
    fr.copy_(synth_sequence_torch(f, h, w, seed=0, device=dev))
    uv = torch.stack([synth_sequence_torch(f, h // 2, w // 2, seed=1, device=dev),
                      synth_sequence_torch(f, h // 2, w // 2, seed=2, device=dev)], dim=1).contiguous()
    res = c.encode_device(fr, f, uv_dev=uv)
    syms, csyms = res["symbols"], res["chroma_symbols"]
    eng = c.engine()
    codings = ("varint", "bits")
    calls = {}
    for cd in codings:                                        # the first calls are also the warm-up
        lb, cb = eng.pack_symbols(syms, coding=cd), eng.pack_chroma_symbols(csyms, coding=cd)
        calls["luma", cd] = (lambda cd=cd, lb=lb: eng.pack_symbols(syms, *lb, coding=cd), lb)
        calls["chroma", cd] = (lambda cd=cd, cb=cb: eng.pack_chroma_symbols(csyms, *cb, coding=cd), cb)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, (fn, _) in calls.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    nb = eng.nb
    for cd in codings:
        ltot = calls["luma", cd][1][0][:, nb].cpu().tolist()
        ctot = calls["chroma", cd][1][0][:, nb].cpu().tolist()
        lms, cms = statistics.median(ts["luma", cd]), statistics.median(ts["chroma", cd])
        print(json.dumps({
            "coding": cd, "frames": f, "nb": nb,
            "chroma_bytes_per_frame": round(sum(ctot) / f), "chroma_bytes_i_frame": ctot[0],
            "chroma_dense_bytes_per_frame": nb * 128 * 2,
            "luma_bytes_per_frame": round(sum(ltot) / f),
            "chroma_pack_ms": [round(t, 3) for t in ts["chroma", cd]], "chroma_pack_ms_median": round(cms, 3),
            "luma_pack_ms": [round(t, 3) for t in ts["luma", cd]], "luma_pack_ms_median": round(lms, 3),
            "chroma_ns_per_coef": round(cms * 1e6 / (f * nb * 128), 5),
            "luma_ns_per_coef": round(lms * 1e6 / (f * nb * 256), 5)}))


if __name__ == "__main__":
    main()
