"""Time srtSeparate with the multichannel Wiener filter (csrc/srt_wiener.hip) off and at 1 and 2 iterations, with device events, after warm-up.

    python scripts/wiener_bench.py [--steps 20] [--warmup 3] [--out profiles/wiener_bench.json]

Shapes: the bench shape (64 tiles of 256 x 1024, 4 stems, fp32) and BASELINE configs[4] (the same batch, 5 stems, fp16 conv).  Per (shape, iterations):
ms per srtSeparate call (median, min, max of `steps` event-timed calls), then one more call with per-launch timing (srtGetTiming) summed per launch
name, and the statistics pass's algorithmic bytes (in-band spectrum 16 B per row-bin + S masks x 2 channels x 4 B; the first pass also reads the
out-of-band spectrum for max |x|) over its time, as a fraction of the 8 TB/s HBM peak.  Prints one JSON line per case and writes them all to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM = 8.0e12


def stats_bytes(rows, F, S, first):
    b = rows * F * 16 + S * 2 * rows * F * 4
    return b + (rows * (2049 - F) * 16 if first else 0)


def run(case, stems, precision, iters_list, steps, warmup):
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    T, F, tiles = 256, 1024, 64
    dev = torch.device("cuda", 0)
    eng = srt.Engine(F=F, T=T, stem_modes=(1, 0, 1, 1, 0)[:stems], oob_weights=(0.25, 0.0, 0.25, 0.25, 0.25)[:stems], variant=srt.VARIANT_VST,
                     max_tiles=tiles, device=dev, precision=precision)
    for s in range(stems):
        eng.set_coeff(s, synth_weights(s, dev))
    n = tiles * T * 1024
    g = torch.Generator(device=dev).manual_seed(777)
    L = (torch.rand(n, device=dev, generator=g) - 0.5) * 0.2
    R = 0.5 * L + (torch.rand(n, device=dev, generator=g) - 0.5) * 0.1
    rows = eng.L.srtStftRows(n)
    out = torch.empty((stems, 2, eng.L.srtIstftLength(rows)), device=dev)
    res = []
    for it in iters_list:
        eng.set_wiener(it)
        for _ in range(warmup):
            eng.separate(L, R, out)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev:
            a.record()
            eng.separate(L, R, out)
            b.record()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
        eng.set_timing(True)
        eng.separate(L, R, out)
        tim = eng.get_timing()
        eng.set_timing(False)
        per = {}
        for name, t in tim:
            per[name] = per.get(name, 0.0) + t
        stats_ms = [t for name, t in tim if name == "wiener_stats"]
        r = {"case": case, "stems": stems, "precision": {0: "f32", 1: "f16"}[precision], "tiles": tiles, "T": T, "F": F, "rows": rows,
             "wiener_iterations": it, "steps": steps, "warmup": warmup,
             "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
             "per_launch_ms": {k: round(v, 4) for k, v in per.items()}}
        if stats_ms:
            r["stats_pass_ms"] = [round(t, 4) for t in stats_ms]
            r["stats_pass_hbm_fraction"] = [round(stats_bytes(rows, F, stems, i == 0) / (t * 1e-3) / PEAK_HBM, 3) for i, t in enumerate(stats_ms)]
        print(json.dumps(r), flush=True)
        res.append(r)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wiener_bench.json"))
    a = ap.parse_args()
    res = run("bench shape (BASELINE configs[2])", 4, 0, (0, 1, 2), a.steps, a.warmup)
    res += run("BASELINE configs[4]", 5, 1, (0, 1, 2), a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
