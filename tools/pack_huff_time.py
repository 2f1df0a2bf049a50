"""The packed stream's three codings on the bench's 4K 30-frame GOP (configs[2]) and its VBS variant:
bytes per frame, split into I and P, and what the "huff" pack and unpack cost per frame next to the
"bits" ones in the same process.
    python tools/pack_huff_time.py --out JSON [--workloads 4k,4k_vbs] [--reps 15]
Bytes: each frame packed alone in every coding, the length read from offs[nb].  Times: one frame per
call (an I-frame and the GOP's middle P-frame), every buffer preallocated, device events around each
call alone, two warm-up calls, then --reps calls alternating between the codings; median, min, max.
The pack call is the whole path (huff: histogram + tables + size + scan + write)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CODINGS = ("varint", "bits", "huff")


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(name, dev, reps):
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.synth import synth_sequence_torch
    from streamoptima_amd.workloads import WORKLOADS
    c = WORKLOADS[name]
    h, w, f = c["h"], c["w"], c["frames"]
    y = synth_sequence_torch(f, h, w, seed=c["seed"], device=dev).cpu().numpy()
    enc = Y_Video_codec(h, w, f, 16, 16, c["qp"], c["intra_dur"], 0, 0.015, bool(c.get("vbs")), y_only_frame_arr=y,
                        device=dev)
    enc.encode()
    eng, syms = enc.engine(), enc._symbols
    nb = eng.nb
    types = [int(s.frame_type) for s in syms]
    rec = {"workload": c["workload"], "frames": f, "blocks": nb, "frame_types": types}
    offs = torch.empty((1, nb + 1), dtype=torch.int32, device=dev)
    out = torch.empty((1, max(eng.pack_bound(coding=k) for k in CODINGS)), dtype=torch.uint8, device=dev)
    sizes = {k: [] for k in CODINGS}
    for s in syms:
        for k in CODINGS:
            eng.pack_symbols([s], offs, out, coding=k)
            sizes[k].append(int(offs[0, nb].item()))
    rec["bytes_per_frame"] = sizes
    for k in CODINGS:
        i = [b for b, t in zip(sizes[k], types) if t == 0]
        p = [b for b, t in zip(sizes[k], types) if t == 1]
        rec[f"{k}_I_mean"], rec[f"{k}_P_mean"] = round(sum(i) / len(i)), round(sum(p) / max(len(p), 1))
    rec["huff_over_bits_I"] = round(rec["huff_I_mean"] / rec["bits_I_mean"], 4)
    rec["huff_over_bits_P"] = round(rec["huff_P_mean"] / rec["bits_P_mean"], 4)
    rec["frames_where_huff_is_larger_than_bits"] = [i for i in range(f) if sizes["huff"][i] >= sizes["bits"][i]]
    # times: the I-frame and the middle P-frame, one frame a call
    rec["times"] = {}
    for label, i in (("I", 0), ("P", f // 2)):
        s = syms[i]
        packed = {}
        for k in ("bits", "huff"):
            o, b = eng.pack_symbols([s], coding=k)
            packed[k] = (o[0].clone(), b[0, :int(o[0, nb].item())].clone())
        dst = eng.new_symbols(types[i])
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        from streamoptima_amd import _lib
        one = _lib.ptr_array
        sh = _lib.stream_handle(dev)
        ft = _lib.i32_array([types[i]])

        def unpack(k):
            fn = getattr(eng.lib, "so_unpack_frames_" + k)
            rc = fn(1, ft, one([packed[k][1]]), one([packed[k][0]]), nb, eng.bs, one([dst.split]), one([dst.mv]),
                    one([dst.qtc]), err.data_ptr(), sh)
            _lib.check(rc, k)
        sides = {"pack_bits": lambda: eng.pack_symbols([s], offs, out, coding="bits"),
                 "pack_huff": lambda: eng.pack_symbols([s], offs, out, coding="huff"),
                 "unpack_bits": lambda: unpack("bits"), "unpack_huff": lambda: unpack("huff")}
        for _ in range(2):
            for fn in sides.values():
                fn()
        ts = {k: [] for k in sides}
        for _ in range(reps):
            for k, fn in sides.items():
                ts[k].append(_events(fn))
        assert int(err.item()) == 0
        assert torch.equal(dst.qtc, s.qtc) and torch.equal(dst.split, s.split)
        rec["times"][label] = {k: _stats(v) for k, v in ts.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--workloads", default="4k,4k_vbs")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for name in a.workloads.split(","):
        res[name] = measure(name, dev, a.reps)
        print(json.dumps({name: {k: v for k, v in res[name].items() if k != "bytes_per_frame"}}), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main()
