"""What the Wiener filter costs in the live hop path (srtLiveCreateWiener) at the plugin's shipped geometry, T = 256, F = 1536, 4 stems (VST),
fp32, iterations 0..3.  iterations = 0 is srtLiveCreateEx's path - the baseline, measured in the same job.

    python scripts/live_wiener_bench.py [--out profiles/live_wiener_bench.json] [--calls 200]     # the call and run times below
    python scripts/live_wiener_bench.py --trace                                  # a short stream of the four instances at K = 4, L = 8 for
                                                                                 # `rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python ...`
    python scripts/live_wiener_bench.py --trace-summary BENCH.json DIR           # adds the device times of that trace's kernels to BENCH.json

One stream at a time.  Per (K, L) in (1, 0), (4, 8), (16, 8) and per iteration count, one instance is fed 1024-sample calls: first back to back, then paced at
the hop period (1024 / 44100 s); p50 / p99 / worst wall time of a srtLiveProcess call (perf_counter around the ctypes call), the calls up to the stream's latency
not timed.  One run's time on the network stream is taken on the (4, 8) instance: right after a call that launched a run, srtLiveCopyTensor("masks") waits for
both streams and reads the run's masks back; the median of that wait over the runs is recorded, and its difference to iterations = 0 (the same wait and the same
read-back without the statistics launches) is what the filter adds to a run.  The hop inverse's device time comes from the trace, by kernel name."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F = 256, 1536
OOB = (0.25, 0.0, 0.25, 0.25)
SCHEDULES = ((1, 0), (4, 8), (16, 8))
HOP_S = 1024 / 44100.0


def stats(us):
    v = sorted(us)
    return {"timed_calls": len(v), "p50_us": round(v[len(v) // 2], 1), "p99_us": round(v[int(0.99 * (len(v) - 1) + 0.5)], 1), "worst_us": round(v[-1], 1)}


class Stream:
    def __init__(self, coeffs, K, Lk, iters):
        import ctypes as C
        import numpy as np
        import spleeterrt_amd as srt
        self.C, self.K = C, K
        self.live = srt.Live(F, T, (1, 1, 1, 1), OOB, srt.VARIANT_VST, srt.PREC_F32, K, Lk, coeffs, wiener=iters, create_ex=True)
        assert self.live.wiener == iters
        x = np.random.default_rng(4).uniform(-0.1, 0.1, (2, 1024)).astype(np.float32)
        self.x, self.out = x, np.zeros((8, 1024), np.float32)
        self.xl, self.xr = C.c_void_p(x[0].ctypes.data), C.c_void_p(x[1].ctypes.data)
        self.planes = (C.c_void_p * 8)(*[self.out[j].ctypes.data for j in range(8)])
        self.masks = np.zeros(2 * T * F, np.float32)
        self.calls = 0

    def call(self):
        t0 = time.perf_counter()
        w = self.live.L.srtLiveProcess(self.live.h, self.xl, self.xr, 1024, self.planes)
        dt = (time.perf_counter() - t0) * 1e6
        assert w == 1024
        self.calls += 1
        return dt

    def launched_a_run(self):
        return (self.calls - 1) % self.K == self.K - 1

    def join(self):
        """wall time until the run in flight is done and its masks are in host memory"""
        hr = self.C.c_longlong(0)
        t0 = time.perf_counter()
        n = self.live.L.srtLiveCopyTensor(self.live.h, b"masks", 0, 0, self.C.c_void_p(self.masks.ctypes.data), self.masks.size, self.C.byref(hr))
        dt = (time.perf_counter() - t0) * 1e6
        assert n == self.masks.size and hr.value == self.calls - 1
        return dt


def measure(coeffs, K, Lk, iters, calls):
    s = Stream(coeffs, K, Lk, iters)
    skip = s.live.latency // 1024 + 1
    row = {"hops_per_run": K, "lookahead": Lk, "iterations": iters, "latency_samples": s.live.latency}
    b2b = [s.call() for _ in range(skip + calls)][skip:]
    row["back_to_back"] = stats(b2b)
    paced, t0 = [], time.perf_counter()
    for i in range(calls):
        while time.perf_counter() < t0 + i * HOP_S:
            time.sleep(0.0002)
        paced.append(s.call())
    row["paced"] = stats(paced)
    if (K, Lk) == (4, 8):
        joins = []
        while len(joins) < 24:
            s.call()
            if s.launched_a_run():
                joins.append(s.join())
        joins.sort()
        row["run_join_and_masks_readback_us"] = {"runs": len(joins), "min": round(joins[0], 1), "median": round(joins[len(joins) // 2], 1), "max": round(joins[-1], 1)}
    row["output_peak"] = round(float(abs(s.out).max()), 6)
    s.live.close()
    return row


def trace_summary(bench_json, d):
    """device time per launch of the kernels of a rocprofv3 kernel trace of --trace, by kernel name"""
    import csv
    rec = json.load(open(bench_json))
    rows = list(csv.DictReader(open(os.path.join(d, "t_kernel_trace.csv"))))
    out = {}
    for key in ("srt_stream_inverse_kernel", "srt_live_wiener_inverse_kernel<false>", "srt_stream_forward_kernel", "srt_live_gather_kernel",
                "srt_live_spec_gather_kernel", "srt_wiener_stats_kernel", "srt_wiener_finalize_kernel"):
        v = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if key in r["Kernel_Name"])
        if v:
            out[key] = {"launches": len(v), "min_us": round(v[0], 2), "median_us": round(v[len(v) // 2], 2), "max_us": round(v[-1], 2)}
    # --trace runs the instances of iterations 1, 2, 3 one after the other for the same number of hops: the filtering inverse's launches in start order, in thirds
    w = sorted((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows if "srt_live_wiener_inverse_kernel" in r["Kernel_Name"])
    for n in (1, 2, 3):
        v = sorted(d for _, d in w[(n - 1) * len(w) // 3:n * len(w) // 3])
        if v:
            out["srt_live_wiener_inverse_kernel<false> iterations %d" % n] = {"launches": len(v), "min_us": round(v[0], 2), "median_us": round(v[len(v) // 2], 2), "max_us": round(v[-1], 2)}
    rec["trace_device_time"] = out
    print(json.dumps(out))
    with open(bench_json, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-summary", nargs=2, default=None, metavar=("BENCH_JSON", "DIR"))
    a = ap.parse_args()
    if a.trace_summary:
        trace_summary(*a.trace_summary)
        return
    import numpy as np
    from oracle import pyoracle as O
    coeffs = [np.ascontiguousarray(O.synth_coeff(k)) for k in range(4)]
    if a.trace:
        for iters in range(4):
            s = Stream(coeffs, 4, 8, iters)
            for _ in range(s.live.latency // 1024 + 40):
                s.call()
            s.live.close()
        return
    rec = {"geometry": {"F": F, "T": T, "n_stems": 4, "variant": "VST", "precision": "fp32"}, "hop_period_us": round(HOP_S * 1e6, 1), "rows": []}
    for K, Lk in SCHEDULES:
        for iters in range(4):
            row = measure(coeffs, K, Lk, iters, a.calls)
            rec["rows"].append(row)
            print(json.dumps(row), flush=True)
    by = {(r["hops_per_run"], r["iterations"]): r for r in rec["rows"]}
    base = by[(4, 0)]["run_join_and_masks_readback_us"]["median"]
    rec["filter_adds_to_a_run_us"] = {str(n): round(by[(4, n)]["run_join_and_masks_readback_us"]["median"] - base, 1) for n in (1, 2, 3)}
    p = by[(4, 1)]["paced"]
    # tests/test_live.py::test_live_call_latency's bounds for a paced stream: p99 < 2 ms, worst call < the hop period
    rec["k4_l8_n1_paced_inside_the_unfiltered_bounds"] = bool(p["p99_us"] < 2000.0 and p["worst_us"] < HOP_S * 1e6)
    print(json.dumps({"filter_adds_to_a_run_us": rec["filter_adds_to_a_run_us"], "k4_l8_n1_paced_inside_the_unfiltered_bounds": rec["k4_l8_n1_paced_inside_the_unfiltered_bounds"]}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
