"""What the stem remix and the average mask extension cost in the live hop (srtLiveCreateEx) at the plugin's shipped geometry, T = 256,
F = 1536, 4 stems (VST), fp32, K = 4, L = 8: a 44.1 kHz instance fed 1024-sample calls and a 48 kHz rate instance fed 480-sample calls (max_block 480).

    python scripts/live_mix_bench.py [--out profiles/live_mix_bench.json]          # the call times below
    python scripts/live_mix_bench.py --trace --out DIR/run.json                      # a short stream of the same three instances for
                                                                                     # `rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python ...`
    python scripts/live_mix_bench.py --trace-summary BENCH.json DIR                  # adds the hop kernels' device times of that trace to BENCH.json

Three instances live in one process and are called alternately, one call each per round, so that they see the same machine state:
  off       mix off, constant rule: the launches of srtLiveCreate (the baseline; with the plugin's weights its inverse is srt_stream_inverse_kernel)
  karaoke   one output, the row (-1, 0, 0, 0 | 1): srt_live_combine_inverse_kernel<false>, one workgroup
  average   mix off with the average extension: srt_live_combine_inverse_kernel<true>, four workgroups, and one srt_mask_ext_kernel launch per run
Per instance: p50 / p99 / worst wall time of a srtLiveProcess call after the start-up (Python's perf_counter around the ctypes call) and the derived
bytes a call brings back (planes x samples x 4).  The device time of the hop inverse comes from the trace: the launches are told apart by kernel name."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F, K, LK = 256, 1536, 4, 8
OOB = (0.25, 0.0, 0.25, 0.25)
KARAOKE = [[-1.0, 0.0, 0.0, 0.0, 1.0]]
INSTANCES = (("off", {}), ("karaoke", {"mix": KARAOKE}), ("average", {"mask_extension": "average"}))


def stats(us):
    v = sorted(us)
    return {"timed_calls": len(v), "p50_us": round(v[len(v) // 2], 1), "p99_us": round(v[int(0.99 * (len(v) - 1) + 0.5)], 1), "worst_us": round(v[-1], 1)}


def measure(coeffs, fs, call, extra):
    """the three instances called in turn with `call` samples each; the calls up to the stream's latency are not timed"""
    import ctypes as C
    import numpy as np
    import spleeterrt_amd as srt
    lives = [(name, srt.Live(F, T, (1, 1, 1, 1), OOB, srt.VARIANT_VST, srt.PREC_F32, K, LK, coeffs, sample_rate=fs, max_block=call, **kw))
             for name, kw in INSTANCES]
    rate = fs or 44100
    lat = lives[0][1].latency
    assert all(lv.latency == lat for _, lv in lives)
    n = (lat + int(extra * 1024 * rate / 44100.0)) // call
    rng = np.random.default_rng(4)
    x = rng.uniform(-0.1, 0.1, (2, call)).astype(np.float32)
    xl, xr = C.c_void_p(x[0].ctypes.data), C.c_void_p(x[1].ctypes.data)
    bufs, us = {}, {name: [] for name, _ in lives}
    for name, lv in lives:
        out = np.zeros((2 * lv.outputs, call), np.float32)
        bufs[name] = (out, (C.c_void_p * (2 * lv.outputs))(*[out[j].ctypes.data for j in range(2 * lv.outputs)]))
    for _ in range(n):
        for name, lv in lives:
            t0 = time.perf_counter()
            w = lv.L.srtLiveProcess(lv.h, xl, xr, call, bufs[name][1])
            us[name].append((time.perf_counter() - t0) * 1e6)
            assert w == call
    rows = []
    for name, lv in lives:
        row = {"instance": name, "sample_rate": rate, "call": call, "outputs": lv.outputs, "latency_samples": lat,
               "bytes_back_per_call": 2 * lv.outputs * call * 4, "output_peak": round(float(abs(bufs[name][0]).max()), 6)}
        row.update(stats(us[name][lat // call + 1:]))
        rows.append(row)
        lv.close()
    base = rows[0]
    for row in rows:
        row["p50_vs_off_us"] = round(row["p50_us"] - base["p50_us"], 1)
    return rows, n


def trace_summary(bench_json, d):
    """device time per launch of the hop's kernels in a rocprofv3 kernel trace of --trace, by kernel name"""
    import csv
    rec = json.load(open(bench_json))
    rows = list(csv.DictReader(open(os.path.join(d, "t_kernel_trace.csv"))))
    out = {}
    for key in ("srt_stream_inverse_kernel", "srt_live_combine_inverse_kernel<false>", "srt_live_combine_inverse_kernel<true>", "srt_stream_forward_kernel",
                "srt_mask_ext_kernel", "srt_rsstream_kernel"):
        v = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if key in r["Kernel_Name"])
        if v:
            out[key] = {"launches": len(v), "min_us": round(v[0], 2), "median_us": round(v[len(v) // 2], 2), "max_us": round(v[-1], 2)}
    rec["trace_device_time"] = out
    print(json.dumps(out))
    with open(bench_json, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
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
        rows, n = measure(coeffs, None, 1024, 48)
        run = {"rounds": n, "instances": [r["instance"] for r in rows]}
        print(json.dumps(run))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(run, f)
        return
    rec = {"geometry": {"F": F, "T": T, "n_stems": 4, "variant": "VST", "precision": "fp32", "hops_per_run": K, "lookahead": LK}, "rows": []}
    for _turn in range(2):                               # two turns per rate; both are kept, the second one is free of first-use effects
        for fs, call in ((None, 1024), (48000, 480)):
            rows, _ = measure(coeffs, fs, call, 192)
            for row in rows:
                row["turn"] = _turn
                rec["rows"].append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
