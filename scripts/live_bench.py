"""Cost and latency of the live mode (srtLive*) at the plugin's shipped geometry, T = 256, F = 1536, 4 stems (VST), fp32 and fp16.

    python scripts/live_bench.py [--out profiles/live_bench.json]      # the measurements below
    python scripts/live_bench.py --trace                                 # a short K = 4 stream for `rocprofv3 --kernel-trace --stats` (run on its own)

Per precision:
  run_ms          GPU time of one run's network: an Engine(max_tiles=1) of the same config in graph mode replays srtForward on one window,
                  device events around each replay (median / min / max of 50 after 10 warm-up); the gather kernel's time comes from the
                  rocprofv3 trace of --trace (srt_live_gather_kernel) and is added in DESIGN.md §11;
  calls[K]        wall time of every srtLiveProcess call of one stream fed 1024-sample calls back to back (Python's perf_counter around the ctypes
                  call, so ~5 us of binding overhead is included), K = 1, 4, 16, 256 with L = 0 (K = 256: the plugin's mode), D + 96 hops each;
                  p50 / p99 / worst over every call after the first D hops;
  gpu_share[K]    run_ms / (K * 23.22 ms): the fraction of one GPU a stream's networks take at that K;
Latency of each (K, L) in the table: srtLiveLatency in samples and ms at 44.1 kHz.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import spleeterrt_amd as srt
    from oracle import pyoracle as O
    coeffs = [np.ascontiguousarray(O.synth_coeff(k)) for k in range(4)]
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
