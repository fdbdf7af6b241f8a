#!/usr/bin/env python3
"""16-bit PCM at the host-stream boundary, measured: the BASELINE configs[3] stream of scripts/stream_c4.py (60 minutes, 4 stems, chunks of
64 tiles, page-locked host buffers) through srtSeparateHostStreamIo in the four I/O combinations (float / int16 in x float / int16 out), in the fp32 and the
fp16-storage mode, and the two conversion kernels alone under device events at one chunk's size.

    python scripts/pcm16_bench.py                         # all cases -> profiles/pcm16_bench.json
    python scripts/pcm16_bench.py --parent-root DIR       # + the float-I/O case alternated with the same case on a built tree of the parent commit

Every case runs in a fresh process (this script started with --case): engine, page-locked buffers and the stream are set up, 2 warm-up calls, then 5 timed
calls; the median, the minimum and the maximum are reported.  The float-I/O case goes through separate_host_stream (the call the parent commit has), so the
same child runs against either tree.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, T, STEMS, HOP, FS = 1024, 256, 4, 1024, 44100.0
PEAK_HBM = 8.0e12                                       # bench.py's PEAK_HBM_TBS: what the other kernels' fractions are quoted against


def child_stream(root, precision, in16, out16, minutes, max_tiles, calls, warmup):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    import stream_c4
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_audio = int(round(minutes * 60 * FS))
    n = 4096 * ((n_audio + 4095) // 4096) + 8192
    rows = (n + HOP - 1) // HOP
    ln = rows * HOP + 3072
    eng = srt.Engine(F=F, T=T, stem_modes=(1,) * STEMS, oob_weights=(0.25, 0.0, 0.25, 0.25), variant=srt.VARIANT_VST, max_tiles=max_tiles, device=dev,
                     precision={"f32": srt.PREC_F32, "f16": srt.PREC_F16}[precision])
    for s in range(STEMS):
        eng.set_coeff(s, synth_weights(s, dev))
    Lp = torch.zeros(n, dtype=torch.float32, pin_memory=True)
    Rp = torch.zeros(n, dtype=torch.float32, pin_memory=True)
    stream_c4.synth_stream(n_audio, 0, n_audio, out=(Lp.numpy()[:n_audio], Rp.numpy()[:n_audio]))
    if in16:
        q = torch.zeros((n, 2), dtype=torch.int16, pin_memory=True)
        qv = q.numpy()
        qv[:, 0] = np.rint(Lp.numpy() * 32768.0)
        qv[:, 1] = np.rint(Rp.numpy() * 32768.0)
        del Lp, Rp
        src = q
    if out16:
        out = torch.empty((STEMS, ln, 2), dtype=torch.int16, pin_memory=True)
    else:
        out = torch.empty((STEMS, 2, ln), dtype=torch.float32, pin_memory=True)
    clipped = None

    def call():
        nonlocal clipped
        if not in16 and not out16:
            eng.separate_host_stream(Lp, Rp, out=out, pinned=True)
        else:
            _, clipped = eng.separate_host_stream_io(src if in16 else (Lp, Rp), out_pcm16=out16, out=out, pinned=True)
    for _ in range(warmup):
        call()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()                                           # synchronous: returns after the last download
        times.append(time.perf_counter() - t0)
    eng.close()
    med = statistics.median(times)
    return {"precision": precision, "in": "int16" if in16 else "float32", "out": "int16" if out16 else "float32", "root": root,
            "seconds_median": med, "seconds_min": min(times), "seconds_max": max(times), "seconds": times, "calls": calls, "warmup": warmup,
            "x_realtime_pcie_inclusive": rows * HOP / FS / med, "rows": rows, "minutes": minutes, "max_tiles_per_chunk": max_tiles,
            "bytes_h2d": n * 4 if in16 else n * 8, "bytes_d2h": STEMS * ln * (4 if out16 else 8),
            "clipped": None if clipped is None else [int(c) for c in clipped]}


def child_kernels(max_tiles, reps):
    """the two kernels alone at one chunk's size: max_tiles * T rows, STEMS stereo pairs for the pack"""
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    import spleeterrt_amd as srt
    lib = srt.load_library()
    torch.cuda.set_device(0)
    count = max_tiles * T * HOP + 3072
    planes = (torch.rand((STEMS, 2, count), device="cuda") - 0.5) * 2.2           # a few percent clip
    out = torch.empty((STEMS, count, 2), dtype=torch.int16, device="cuda")
    clip = torch.zeros(STEMS, dtype=torch.int64, device="cuda")
    pcm = torch.randint(-32768, 32768, (count, 2), dtype=torch.int16, device="cuda")
    lr = torch.empty((2, count), device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())
    cases = {
        "pack_counting": (lambda: lib.srtPcm16Pack(sp, vp(planes), count, STEMS, count, vp(out), count, vp(clip)), STEMS * count * 12),
        "pack": (lambda: lib.srtPcm16Pack(sp, vp(planes), count, STEMS, count, vp(out), count, None), STEMS * count * 12),
        "unpack": (lambda: lib.srtPcm16Unpack(sp, vp(pcm), count, vp(lr[0]), vp(lr[1])), count * 12),
    }
    res = {"frames": count, "pairs": STEMS, "reps": reps, "peak_hbm_bytes_per_s": PEAK_HBM}
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for name, (fn, nbytes) in cases.items():
            for _ in range(3):
                assert fn() == 0, lib.srtLastError()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                assert fn() == 0, lib.srtLastError()
                b.record(s)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            med = statistics.median(ms)
            res[name] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "bytes": nbytes, "gb_per_s": nbytes / (med * 1e-3) / 1e9,
                         "fraction_of_peak_hbm": nbytes / (med * 1e-3) / PEAK_HBM}
    return res


def spawn(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("case %s failed:\n%s\n%s" % (args, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--max-tiles", type=int, default=64)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precisions", default="f32,f16")
    ap.add_argument("--parent-root", default="", help="a built tree of the parent commit: its float-I/O case is alternated with this tree's")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm16_bench.json"))
    ap.add_argument("--case", default="", help="(internal) precision,in16,out16 | kernels")
    ap.add_argument("--root", default=ROOT, help="(internal) the tree whose package the case imports")
    a = ap.parse_args()
    if a.case == "kernels":
        print(json.dumps(child_kernels(a.max_tiles, 20)))
        return
    if a.case:
        prec, i16, o16 = a.case.split(",")
        print(json.dumps(child_stream(a.root, prec, i16 == "1", o16 == "1", a.minutes, a.max_tiles, a.calls, a.warmup)))
        return
    common = ["--minutes", str(a.minutes), "--max-tiles", str(a.max_tiles), "--calls", str(a.calls), "--warmup", str(a.warmup)]
    res = {"config": "BASELINE configs[3] stream (scripts/stream_c4.py): %.1f min, %d stems, %dx%d tiles, chunks of %d, page-locked host buffers; "
                     "median of %d calls after %d warm-up calls, one fresh process per case" % (a.minutes, STEMS, T, F, a.max_tiles, a.calls, a.warmup),
           "kernels": spawn(["--case", "kernels", "--max-tiles", str(a.max_tiles)]), "stream": []}
    print(json.dumps(res["kernels"]), flush=True)
    for prec in a.precisions.split(","):
        for i16, o16 in ((0, 0), (1, 0), (0, 1), (1, 1)):
            r = spawn(common + ["--case", "%s,%d,%d" % (prec, i16, o16)])
            r.pop("root")
            res["stream"].append(r)
            print(json.dumps({k: r[k] for k in ("precision", "in", "out", "seconds_median", "seconds_min", "seconds_max")}), flush=True)
    if a.parent_root:
        ab = {"this": [], "parent": []}
        for _ in range(a.alternations):
            for tag, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
                ab[tag].append(spawn(common + ["--case", "f32,0,0", "--root", root])["seconds_median"])
        res["float_io_vs_parent"] = {"seconds_median_per_process": ab, "this_median": statistics.median(ab["this"]),
                                     "parent_min": min(ab["parent"]), "parent_max": max(ab["parent"]),
                                     "inside_parent_range": min(ab["parent"]) <= statistics.median(ab["this"]) <= max(ab["parent"])}
        print(json.dumps(res["float_io_vs_parent"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
