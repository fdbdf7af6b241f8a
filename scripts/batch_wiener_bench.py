"""Time srtSeparateBatchWiener (the multichannel Wiener filter per track of a packed batch) against the calls it replaces, with device events, after warm-up.

    python scripts/batch_wiener_bench.py [--steps 20] [--warmup 3] [--out profiles/batch_wiener_bench.json]
    python scripts/batch_wiener_bench.py --filter-off-only [--package-root OTHER_CHECKOUT] --out FILE

Bench shape: F = 1024, T = 256, max_tiles = 64, 4 stems fp32 and 5 stems fp16, iterations = 1, 32 clips of 10 s (431 rows, 2 tiles each = 64 packed tiles,
13 792 real rows).  Cases, per precision:
  (a) one srtSeparateBatchWiener against the same clips as 32 srtSeparate calls with srtSetWiener(1), and against one srtSeparate of a single 64-tile signal
      (16 384 rows) with the filter on; the three are timed alternately (one call of each per step) in the same process;
  (b) the filter off: srtSeparateBatch of the clips and srtSeparate of the 64-tile signal, alternately.  --filter-off-only runs just this case, and
      --package-root imports spleeterrt_amd from another checkout (built there), so that the same script times the parent commit's library for an A/B;
  (c) per-launch ms (srtGetTiming) of the four batch kernels next to their single-signal relatives on one signal of the same 13 792 rows, and of the whole
      batch call and the 64-tile call (which launch carries a difference between them).
Every time is the median (with min and max) of `steps` event-timed calls after `warmup` calls; one JSON line per case, all of them written to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F, TILES, ITERS = 256, 1024, 64, 1


def timed_alternately(fns, steps, warmup):
    """fns: {name: callable}; one call of each per step, in order; -> {name: {ms_median, ms_min, ms_max}}"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] for k in fns}
    for i in range(steps):
        for k, fn in fns.items():
            a, b = ev[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    out = {}
    for k in fns:
        ms = [a.elapsed_time(b) for a, b in ev[k]]
        out[k] = {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    return out


def per_launch(eng, fn, steps):
    """median ms per launch name over `steps` calls (per-launch events; a name launched several times in one call is summed per call)"""
    fn()
    eng.set_timing(True)
    for _ in range(steps):
        fn()
    tim = eng.get_timing()
    eng.set_timing(False)
    per_call = len(tim) // steps
    sums = []
    for i in range(steps):
        d = {}
        for name, t in tim[i * per_call:(i + 1) * per_call]:
            d[name] = d.get(name, 0.0) + t
        sums.append(d)
    return {k: round(statistics.median(d[k] for d in sums), 4) for k in sums[0]}


def clips(counts, seed, dev):
    """seeded stereo noise clips of the given sample counts"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for m in counts:
        L = (torch.rand(m, device=dev, generator=g) - 0.5) * 0.2
        R = 0.5 * L + (torch.rand(m, device=dev, generator=g) - 0.5) * 0.1
        out.append((L, R))
    return out


def run(precision, S, steps, warmup, filter_off_only, label):
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    dev = torch.device("cuda", 0)
    prec = {srt.PREC_F32: "f32", srt.PREC_F16: "f16"}[precision]
    eng = srt.Engine(F=F, T=T, stem_modes=(1, 0, 1, 1, 0)[:S], oob_weights=(0.25, 0.0, 0.25, 0.25, 0.25)[:S], variant=srt.VARIANT_VST, max_tiles=TILES,
                     device=dev, precision=precision)
    for s in range(S):
        eng.set_coeff(s, synth_weights(s, dev))
    base = {"precision": prec, "T": T, "F": F, "stems": S, "max_tiles": TILES, "iterations": ITERS, "steps": steps, "warmup": warmup, "library": label}
    res = []

    def emit(r):
        r = dict(base, **r)
        print(json.dumps(r), flush=True)
        res.append(r)

    tr = clips([441000] * 32, 7, dev)
    ns = [L.numel() for L, _ in tr]
    rows = [eng.L.srtStftRows(n) for n in ns]
    outs = [torch.empty((S, 2, eng.L.srtIstftLength(r)), device=dev) for r in rows]
    n64 = TILES * T * 1024
    big = clips([n64], 8, dev)[0]
    out64 = torch.empty((S, 2, eng.L.srtIstftLength(eng.L.srtStftRows(n64))), device=dev)

    # (b) the filter off (also what the parent commit's library can run)
    off = timed_alternately({"srtSeparateBatch": lambda: eng.separate_batch(tr, outs),
                             "srtSeparate_64_tiles": lambda: eng.separate(big[0], big[1], out64)}, steps, warmup)
    emit(dict({"case": "(b) filter off"}, **off))
    if filter_off_only:
        eng.close()
        return res

    # (a) the batch call, the loop of 32 filtered srtSeparate calls and one filtered 64-tile srtSeparate, alternately
    eng.set_wiener(ITERS)
    on = timed_alternately({"srtSeparateBatchWiener": lambda: eng.separate_batch(tr, outs, wiener=ITERS),
                            "loop_32_srtSeparate_wiener": lambda: [eng.separate(L, R, o) for (L, R), o in zip(tr, outs)],
                            "srtSeparate_wiener_64_tiles": lambda: eng.separate(big[0], big[1], out64)}, steps, warmup)
    b, lp, sg = (on[k]["ms_median"] for k in ("srtSeparateBatchWiener", "loop_32_srtSeparate_wiener", "srtSeparate_wiener_64_tiles"))
    emit(dict({"case": "(a) 32 clips x 10 s, filter on", "tracks": 32, "rows_per_track": rows[0], "real_rows": sum(rows), "packed_tiles": TILES,
               "speedup_batch_over_loop": round(lp / b, 3), "batch_over_single_64_tiles": round(b / sg, 4)}, **on))

    # (c) per launch: the batch kernels next to the single-signal ones at equal rows, and the two whole calls
    tot_rows = sum(rows)
    eq = clips([tot_rows * 1024], 9, dev)[0]
    assert eng.L.srtStftRows(eq[0].numel()) == tot_rows
    outeq = torch.empty((S, 2, eng.L.srtIstftLength(tot_rows)), device=dev)
    pb = per_launch(eng, lambda: eng.separate_batch(tr, outs, wiener=ITERS), steps)
    ps = per_launch(eng, lambda: eng.separate(eq[0], eq[1], outeq), steps)
    p64 = per_launch(eng, lambda: eng.separate(big[0], big[1], out64), steps)
    pairs = (("wiener_stats_batch", "wiener_stats"), ("wiener_cov_batch", "wiener_cov"), ("wiener_filter_batch", "wiener_filter"), ("istft_batch", "istft"))
    emit({"case": "(c) per launch", "rows": tot_rows, "packed_rows_incl_tile_padding": TILES * T,
          "batch_vs_single_at_equal_rows_ms": {bn: {"batch": pb.get(bn), "single": ps.get(sn)} for bn, sn in pairs},
          "batch_call_per_launch_ms": pb, "single_64_tile_call_per_launch_ms": p64})
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--filter-off-only", action="store_true")
    ap.add_argument("--package-root", default=None, help="import spleeterrt_amd from this checkout instead (A/B against another commit's library)")
    ap.add_argument("--label", default=None, help="recorded as \"library\" in every line (default: \"this tree\", or the --package-root path)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_wiener_bench.json"))
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    import spleeterrt_amd as srt
    label = a.label or (a.package_root or "this tree")
    res = run(srt.PREC_F32, 4, a.steps, a.warmup, a.filter_off_only, label)
    res += run(srt.PREC_F16, 5, a.steps, a.warmup, a.filter_off_only, label)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
