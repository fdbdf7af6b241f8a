"""Cost and latency of the live mode (srtLive*) at the plugin's shipped geometry, T = 256, F = 1536, 4 stems (VST), fp32 and fp16.

    python scripts/live_bench.py [--out profiles/live_bench.json]      # the measurements below
    python scripts/live_bench.py --trace                                 # a short K = 4 stream for `rocprofv3 --kernel-trace --stats` (run on its own)
    python scripts/live_bench.py --rate [--out profiles/live_rate_bench.json]   # the 44.1 kHz instance against the 48 kHz rate instance
    python scripts/live_bench.py --trace --rate --k K --out DIR/run.json # a short stream on a 48 kHz rate instance, 512-sample calls, under rocprofv3 -d DIR
    python scripts/live_bench.py --rate-trace-summary BENCH.json DIR...  # adds the traces' summaries (converter launches, copies, GPU time) to BENCH.json

Per precision:
  run_ms          GPU time of one run's network: an Engine(max_tiles=1) of the same config in graph mode replays srtForward on one window,
                  device events around each replay (median / min / max of 50 after 10 warm-up); the gather kernel's time comes from the
                  rocprofv3 trace of --trace (srt_live_gather_kernel) and is added in DESIGN.md §11;
  calls[K]        wall time of every srtLiveProcess call of one stream fed 1024-sample calls back to back (Python's perf_counter around the ctypes
                  call, so ~5 us of binding overhead is included), K = 1, 4, 16, 256 with L = 0 (K = 256: the plugin's mode), D + 96 hops each;
                  p50 / p99 / worst over every call after the first D hops;
  gpu_share[K]    run_ms / (K * 23.22 ms): the fraction of one GPU a stream's networks take at that K;
Latency of each (K, L) in the table: srtLiveLatency in samples and ms at 44.1 kHz.
--rate: fp32 only, K = 1, 4, 256 with L = 0; per K the 44.1 kHz instance (1024-sample calls) and the 48 kHz rate instance (1024- and 512-sample calls)
are measured in turn, twice, and the calls of both turns are pooled: p50 / p99 / worst per call after the start-up, and calls_us_per_audio_s = the sum
of the call times per second of audio (the host thread's share).  The GPU's own time per second of audio comes from `rocprofv3 --kernel-trace
--stats --output-format csv -d DIR -o t -- python scripts/live_bench.py --trace --rate --k K --out DIR/run.json`, one run of its own per K,
summarised by --rate-trace-summary: every kernel of the process from the first timed call's start on, per second of the audio those calls carry.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F = 256, 1536
OOB = (0.25, 0.0, 0.25, 0.25)
HOP_MS = 1024 / 44100 * 1e3
TABLE = [(1, 0), (1, 8), (2, 4), (4, 0), (4, 8), (8, 8), (16, 16), (32, 32), (64, 64), (128, 0), (256, 0)]


def run_ms(coeffs, precision, steps=50, warmup=10):
    import torch
    import spleeterrt_amd as srt
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = srt.Engine(F=F, T=T, stem_modes=(1, 1, 1, 1), oob_weights=OOB, variant=srt.VARIANT_VST, max_tiles=1, precision=precision)
        for s, c in enumerate(coeffs):
            eng.set_coeff(s, c)
        eng.set_graph_mode(True)
        mag = torch.rand((1, 2, T, F), device="cuda") * 50
        masks = torch.empty((4, 1, 2, T, F), device="cuda")
        eng.prepare_forward(mag, masks)
        for _ in range(warmup):
            eng.forward(mag, masks)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev:
            a.record(stream)
            eng.forward(mag, masks)
            b.record(stream)
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    eng.close()
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def calls(coeffs, precision, K, Lk=0, extra=96):
    import numpy as np
    import ctypes as C
    import spleeterrt_amd as srt
    live = srt.Live(F, T, (1, 1, 1, 1), OOB, srt.VARIANT_VST, precision, K, Lk, coeffs)
    D = Lk + 2 * K
    hops = D + extra
    rng = np.random.default_rng(K)
    x = rng.uniform(-0.1, 0.1, (2, 1024)).astype(np.float32)
    out = np.zeros((8, 1024), np.float32)
    P = C.c_void_p * 8
    ptrs = P(*[out[j].ctypes.data for j in range(8)])
    us = []
    for h in range(hops):
        t0 = time.perf_counter()
        w = live.L.srtLiveProcess(live.h, C.c_void_p(x[0].ctypes.data), C.c_void_p(x[1].ctypes.data), 1024, ptrs)
        us.append((time.perf_counter() - t0) * 1e6)
        assert w == 1024
    lat = live.latency
    live.close()
    v = sorted(us[D:])
    return {"hops": hops, "timed_calls": len(v), "p50_us": round(v[len(v) // 2], 1), "p99_us": round(v[int(0.99 * (len(v) - 1) + 0.5)], 1),
            "worst_us": round(v[-1], 1), "first_call_us": round(us[0], 1), "latency_samples": lat}


def calls_rate(coeffs, K, fs, call, extra=96):
    """wall time of every srtLiveProcess call of `call` samples: a 44.1 kHz instance (fs None) or a rate instance at fs; the start-up (latency) is not timed"""
    import numpy as np
    import ctypes as C
    import spleeterrt_amd as srt
    live = srt.Live(F, T, (1, 1, 1, 1), OOB, srt.VARIANT_VST, srt.PREC_F32, K, 0, coeffs, sample_rate=fs, max_block=call)
    lat = live.latency
    rate = fs or 44100
    n = (lat + int(extra * 1024 * rate / 44100.0)) // call
    rng = np.random.default_rng(K)
    x = rng.uniform(-0.1, 0.1, (2, call)).astype(np.float32)
    out = np.zeros((8, call), np.float32)
    ptrs = (C.c_void_p * 8)(*[out[j].ctypes.data for j in range(8)])
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        w = live.L.srtLiveProcess(live.h, C.c_void_p(x[0].ctypes.data), C.c_void_p(x[1].ctypes.data), call, ptrs)
        us.append((time.perf_counter() - t0) * 1e6)
        assert w == call
    live.close()
    return us[lat // call + 1:], lat


def rate_table(coeffs, out):
    rec = {"geometry": {"F": F, "T": T, "n_stems": 4, "variant": "VST", "precision": "fp32", "lookahead": 0}, "rows": []}
    for K in (1, 4, 256):
        configs = [("44100_native_1024", None, 1024), ("48000_rate_1024", 48000, 1024), ("48000_rate_512", 48000, 512)]
        pool = {name: [] for name, _, _ in configs}
        lat = {}
        for _turn in range(2):
            for name, fs, call in configs:
                us, lat[name] = calls_rate(coeffs, K, fs, call)
                pool[name] += us
        for name, fs, call in configs:
            v = sorted(pool[name])
            rate = fs or 44100
            row = {"K": K, "instance": name, "sample_rate": rate, "call": call, "timed_calls": len(v), "latency_samples": lat[name],
                   "latency_ms": round(lat[name] / rate * 1e3, 2), "p50_us": round(v[len(v) // 2], 1), "p99_us": round(v[int(0.99 * (len(v) - 1) + 0.5)], 1),
                   "worst_us": round(v[-1], 1), "calls_us_per_audio_s": round(sum(v) / (len(v) * call / rate), 1)}
            rec["rows"].append(row)
            print(json.dumps(row), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)


def trace_summary(bench_json, dirs):
    """per trace directory: the converter launches by side (the input side computes one channel pair, grid y = 1; the output side all 2S = 8 channels,
    grid y = 4), the blit kernels that carry a call's pinned copies, and the GPU time of all kernels per second of audio, create and pre-warm left out"""
    import csv
    rec = json.load(open(bench_json))
    rec["trace"] = []
    for d in dirs:
        run = json.load(open(os.path.join(d, "run.json")))
        rows = list(csv.DictReader(open(os.path.join(d, "t_kernel_trace.csv"))))
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        conv = [i for i, r in enumerate(rows) if "srt_rsstream_kernel" in r["Kernel_Name"]]
        # the two pre-warm launches (input side, then output side, one frame each) come first; the stream's calls follow
        assert len(conv) > 2 and int(rows[conv[0]]["Grid_Size_Y"]) // int(rows[conv[0]]["Workgroup_Size_Y"]) == 1
        first = conv[2]
        while first > 0 and "copyBuffer" in rows[first - 1]["Kernel_Name"]:      # the first call's upload
            first -= 1
        body = rows[first:]
        us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

        def st(v):
            v = sorted(v)
            return {"launches": len(v), "min_us": round(v[0], 2), "median_us": round(v[len(v) // 2], 2), "max_us": round(v[-1], 2)}
        side = lambda r: "srt_rsstream_kernel" in r["Kernel_Name"] and int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"])
        audio = run["calls"] * run["call"] / float(run["sample_rate"])
        total = sum(us(r) for r in body)
        copies = [us(r) for r in body if "copyBuffer" in r["Kernel_Name"]]
        rec["trace"].append({
            "K": run["K"], "sample_rate": run["sample_rate"], "call": run["call"], "calls": run["calls"], "audio_s": round(audio, 3),
            "converter_launches_in_trace": len(conv), "of_which_prewarm": 2,
            "input_side": st([us(r) for r in body if side(r) == 1]), "output_side": st([us(r) for r in body if side(r) == 4]),
            "copy_kernels": dict(st(copies), per_call=round(len(copies) / run["calls"], 2)),
            "gpu_ms_all_kernels": round(total / 1e3, 2), "gpu_ms_per_audio_s": round(total / 1e3 / audio, 2)})
        print(json.dumps(rec["trace"][-1]), flush=True)
    with open(bench_json, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--rate", action="store_true")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rate-trace-summary", nargs="+", default=None, metavar=("BENCH_JSON", "DIR"))
    a = ap.parse_args()
    if a.rate_trace_summary:
        trace_summary(a.rate_trace_summary[0], a.rate_trace_summary[1:])
        return
    import numpy as np
    import spleeterrt_amd as srt
    from oracle import pyoracle as O
    coeffs = [np.ascontiguousarray(O.synth_coeff(k)) for k in range(4)]
    if a.trace and a.rate:
        us, lat = calls_rate(coeffs, a.k, 48000, 512, extra=64)
        run = {"K": a.k, "calls": len(us) + lat // 512 + 1, "call": 512, "sample_rate": 48000, "latency_samples": lat}
        print(json.dumps(run))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)      # rocprofv3 creates its directory only when the program has ended
            with open(a.out, "w") as f:
                json.dump(run, f)
        return
    if a.rate:
        rate_table(coeffs, a.out)
        return
    if a.trace:
        print(json.dumps(calls(coeffs, srt.PREC_F32, 4, 8, extra=64)))
        return
    rec = {"geometry": {"F": F, "T": T, "n_stems": 4, "variant": "VST"}, "hop_ms": round(HOP_MS, 3), "precisions": {}}
    for name, prec in (("fp32", srt.PREC_F32), ("fp16", srt.PREC_F16)):
        r = {"run_ms": run_ms(coeffs, prec), "calls": {}}
        for K in (1, 4, 16, 256):
            r["calls"][str(K)] = calls(coeffs, prec, K)
            print(name, "K=%d" % K, json.dumps(r["calls"][str(K)]), flush=True)
        r["gpu_share"] = {str(K): round(r["run_ms"]["ms_median"] / (K * HOP_MS), 5) for K in (1, 4, 16, 256)}
        rec["precisions"][name] = r
        print(name, "run", json.dumps(r["run_ms"]), flush=True)
    rec["latency"] = [{"K": K, "L": Lk, "D_hops": Lk + 2 * K, "samples": srt.live_latency(K, Lk),
                       "ms": round(srt.live_latency(K, Lk) / 44.1, 2)} for K, Lk in TABLE]
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
