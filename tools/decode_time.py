"""What the fused decoders and the streaming decoder cost against the path they stand beside, on the
bench's 4K 30-frame GOP (configs[2]) with chroma, in both codings of the packed stream.
    python tools/decode_time.py --step write  --dir DIR              # encode once, transmit_packed420 per coding
    python tools/decode_time.py --step device --dir DIR --out JSON   # comparison 1
    python tools/decode_time.py --step region --dir DIR --out JSON   # comparison 2
Three steps so that each runs in a process (and under a time limit) of its own; --out is read,
extended and written back.

1. device: per P-frame (per frame for chroma), device events around the calls alone, everything
   preallocated: so_unpack_frames(_bits) over the run + so_inter_recon_ex per frame against one
   so_decode_p_frames over the run; so_unpack_chroma_frames(_bits) + so_chroma_recon_frame per frame
   against one so_decode_chroma_frames.  The outputs of the two sides are compared once.
2. region: file in, host frames out, host clock from a synchronised device to a synchronised
   device: decoder.decode_packed_file against hostdecode.HostStreamDecoder.decode_file, the latter also
   with fused=False (the same stream on the unpack + reconstruction kernels and one dense set).  The D2H
   link rate is measured in the same process (a 4K 4:2:0 frame's planes to page-locked memory, copy
   engine alone, best of the repeats), and the region is set against the frames' download time at it.
The two sides alternate, --pairs pairs (at least 5) after two warm-up rounds; median, min and max."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CODINGS = ("varint", "bits")


def _cfg():
    from streamoptima_amd.workloads import WORKLOADS
    return WORKLOADS["4k"]


def _path(d, coding):
    return os.path.join(d, f"gop420_{coding}.sopk")


def _stats(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
            "all": [round(t, 4) for t in ts]}


def _update(out, key, value):
    rec = json.load(open(out)) if out and os.path.exists(out) else {}
    rec[key] = value
    print(json.dumps({key: value}), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")


def _decoder(dev):
    from streamoptima_amd.decoder import decoder
    c = _cfg()
    return decoder(0, c["intra_dur"], 16, c["frames"], c["h"], c["w"], c["qp"], 1, False, 0.015, False, device=dev)


def step_write(a, dev):
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.synth import synth_sequence_torch
    c = _cfg()
    h, w, f = c["h"], c["w"], c["frames"]
    y = synth_sequence_torch(f, h, w, seed=c["seed"], device=dev).cpu().numpy()
    uv = torch.stack([synth_sequence_torch(f, h // 2, w // 2, seed=c["seed"] + 1 + p, device=dev) for p in range(2)],
                     dim=1).cpu().numpy()
    os.makedirs(a.dir, exist_ok=True)
    os.chdir(a.dir)
    enc = Y_Video_codec(h, w, f, 16, 16, c["qp"], c["intra_dur"], 0, 0.015, False, y_only_frame_arr=y, device=dev,
                        chroma=True, chroma_qp_offset=0, uv_frame_arr=uv)
    enc.encode()
    sizes = {coding: enc.transmit_packed420(_path(a.dir, coding), coding=coding) for coding in CODINGS}
    _update(a.out, "file", {"workload": c["workload"] + ", 4:2:0", "frames": f, "bytes": sizes,
                            "frame_bytes_420": h * w * 3 // 2})


def _alternate(sides, pairs):
    """sides: {name: callable -> ms}; two warm-up rounds, then `pairs` alternating rounds."""
    for _ in range(2):
        for fn in sides.values():
            fn()
    ts = {k: [] for k in sides}
    for _ in range(pairs):
        for k, fn in sides.items():
            ts[k].append(fn())
    return ts


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def step_device(a, dev):
    from streamoptima_amd import _lib, packedfile
    from streamoptima_amd.engine import FrameSymbols, alloc_planes
    dec = _decoder(dev)
    eng = dec._eng()
    lib, nb = eng.lib, eng.nb
    for coding in CODINGS:
        meta = packedfile.read(_path(a.dir, coding), dev)
        types = meta["frame_types"]
        n = len(types)
        assert types[0] == 0 and all(t == 1 for t in types[1:])
        npf = n - 1
        syms = eng.unpack_symbols(types, meta["packed"], meta["offs"], coding=coding)     # the I-frame's symbols
        ref0 = eng.recon_intra(syms[0].split, syms[0].mv, syms[0].qtc, dec.Qp)
        # ---- luma: the run of P-frames -----------------------------------------------------------
        err = torch.zeros(n, dtype=torch.int32, device=dev)
        p_planes = list(alloc_planes(npf, eng.h, eng.w, dev))
        f_planes = list(alloc_planes(npf, eng.h, eng.w, dev))
        f_split = [torch.empty(nb, dtype=torch.uint8, device=dev) for _ in range(npf)]
        f_mv = [torch.empty((nb, 4, 3), dtype=torch.int16, device=dev) for _ in range(npf)]
        name = "so_unpack_frames_bits" if coding == "bits" else "so_unpack_frames"

        def arr(ts):
            return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        sh = _lib.stream_handle(dev)
        ptypes = (ctypes.c_int32 * npf)(*([1] * npf))
        up = (arr(meta["packed"][1:]), arr(meta["offs"][1:]), arr([s.split for s in syms[1:]]),
              arr([s.mv for s in syms[1:]]), arr([s.qtc for s in syms[1:]]))

        def parent_luma():
            _lib.check(getattr(lib, name)(npf, ptypes, up[0], up[1], nb, eng.bs, up[2], up[3], up[4], err.data_ptr(), sh),
                       name)
            ref = ref0
            for s, out in zip(syms[1:], p_planes):
                eng.recon_inter([ref], s.split, s.mv, s.qtc, dec.Qp, out=out)
                ref = out

        def fused_luma():
            eng.decode_p_frames(meta["packed"][1:], meta["offs"][1:], [ref0], 1, dec.Qp, coding=coding,
                                out_split=f_split, out_mv=f_mv, out_recon=f_planes, err=err)
        ts = _alternate({"unpack_recon": lambda: _events(parent_luma) / npf,
                         "fused": lambda: _events(fused_luma) / npf}, a.pairs)
        assert int(err.abs().sum()) == 0
        same = all(torch.equal(x, y) for x, y in zip(p_planes, f_planes))
        _update(a.out, f"device_luma_{coding}", {"unit": "ms per P-frame", "p_frames": npf, "identical": same,
                                                 **{k: _stats(v) for k, v in ts.items()}})
        # ---- chroma: the whole GOP ---------------------------------------------------------------
        hc, wc = eng.h // 2, eng.w // 2
        q = torch.empty((n, 2, nb, 64), dtype=torch.int16, device=dev)
        pc = alloc_planes(2 * n, hc, wc, dev).view(n, 2, hc, wc)
        fc = alloc_planes(2 * n, hc, wc, dev).view(n, 2, hc, wc)
        cname = "so_unpack_chroma_frames_bits" if coding == "bits" else "so_unpack_chroma_frames"
        cu = (arr(meta["chroma_packed"]), arr(meta["chroma_offs"]), arr([q[i, 0] for i in range(n)]),
              arr([q[i, 1] for i in range(n)]))
        lum = [FrameSymbols(s.frame_type, s.split, s.mv, None, None, None, None, qp_rd=dec.Qp) for s in syms]
        outs = [eng.new_chroma_symbols(encode=False) for _ in range(n)]
        for i, o in enumerate(outs):
            o.recon_u, o.recon_v = pc[i, 0], pc[i, 1]
        off = int(meta["chroma_qp_offset"])

        def parent_chroma():
            _lib.check(getattr(lib, cname)(n, cu[0], cu[1], nb, cu[2], cu[3], err.data_ptr(), sh), cname)
            ru, rv = [], []
            for i, s in enumerate(lum):
                if s.frame_type == 0:
                    ru, rv = [], []
                eng.recon_chroma(s, q[i, 0], q[i, 1], ru, rv, off, out=outs[i])
                ru, rv = [pc[i, 0]], [pc[i, 1]]

        def fused_chroma():
            eng.decode_chroma_frames(types, meta["chroma_packed"], meta["chroma_offs"],
                                     [None] + [s.split for s in syms[1:]], [None] + [s.mv for s in syms[1:]], [], [], 1,
                                     dec.Qp, off, coding=coding, out_u=[fc[i, 0] for i in range(n)],
                                     out_v=[fc[i, 1] for i in range(n)], err=err)
        ts = _alternate({"unpack_recon": lambda: _events(parent_chroma) / n,
                         "fused": lambda: _events(fused_chroma) / n}, a.pairs)
        assert int(err.abs().sum()) == 0
        _update(a.out, f"device_chroma_{coding}", {"unit": "ms per frame (U and V)", "frames": n,
                                                   "identical": bool(torch.equal(pc, fc)),
                                                   **{k: _stats(v) for k, v in ts.items()}})
        del meta, syms, q, pc, fc, p_planes, f_planes
        torch.cuda.empty_cache()


def step_region(a, dev):
    from streamoptima_amd.hostdecode import HostStreamDecoder
    from streamoptima_amd.hostmem import pinned_empty
    c = _cfg()
    dec = _decoder(dev)
    eng = dec._eng()
    hs = HostStreamDecoder(dec, chunk=a.chunk, nbuf=2)
    hs_dense = HostStreamDecoder(dec, chunk=a.chunk, nbuf=2, fused=False)   # the same stream on the unpack + recon kernels
    # the D2H link: one frame's planes (padded luma + chroma) to page-locked memory
    nbytes = eng.h * eng.w * 3 // 2
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = pinned_empty((nbytes,))
    rates = []
    for _ in range(a.pairs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        rates.append(8 * nbytes / (time.perf_counter() - t0) / 1e9)
    link = max(rates[1:])
    _update(a.out, "d2h_link", {"gbs": round(link, 2), "bytes_per_copy": nbytes})
    for coding in CODINGS:
        path = _path(a.dir, coding)
        count = [0]

        def consume(i, y, u, v):
            count[0] += 1

        def parent():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.decode_packed_file(path)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def stream(h=hs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.decode_file(path, consume)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        ts = _alternate({"decode_packed_file": parent, "host_stream_decoder": stream,
                         "host_stream_decoder_unfused": lambda: stream(hs_dense)}, a.pairs)
        assert count[0] == 2 * (a.pairs + 2) * c["frames"]
        down_ms = c["frames"] * nbytes / link / 1e6
        med = statistics.median(ts["host_stream_decoder"])
        _update(a.out, f"region_{coding}", {"unit": "ms per 30-frame GOP, file to host frames", "chunk": a.chunk,
                                            "file_bytes": os.path.getsize(path), "download_ms_at_link": round(down_ms, 3),
                                            "stream_over_download": round(med / down_ms, 3),
                                            **{k: _stats(v) for k, v in ts.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("write", "device", "region"))
    ap.add_argument("--dir", required=True, help="where the step `write` puts the two files")
    ap.add_argument("--out", default=None, help="JSON file to extend")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=2)
    a = ap.parse_args()
    if a.pairs < 5:
        ap.error("--pairs: at least 5")
    a.dir = os.path.abspath(a.dir)
    a.out = os.path.abspath(a.out) if a.out else None
    if not torch.cuda.is_available():
        raise SystemExit("decode_time.py measures on the GPU: no device found")
    {"write": step_write, "device": step_device, "region": step_region}[a.step](a, torch.device("cuda:0"))


if __name__ == "__main__":
    main()
