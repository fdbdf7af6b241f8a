"""Measure the average mask extension (srtSetMaskExtension): the bench-shape step with the mode off and on, in one process.

    python scripts/mask_ext_bench.py [--steps 20] [--warmup 3] [--out profiles/mask_ext_bench.json]

Bench shape: F = 1024, T = 256, max_tiles = 64, srtSeparate of a 64-tile signal (16 384 rows); 4 stems fp32 and the 5-stem fp16 mode (half masks).  Device
events, the median (with min and max) of `steps` calls after `warmup` calls, as the other bench scripts do.  Per precision:
  off       the mode at SRT_MASK_EXT_CONSTANT: the baseline - the path and the kernels of the parent commit (tests/test_mask_extension.py holds it to them
            bit for bit and launch for launch);
  on        SRT_MASK_EXT_AVERAGE on the same engine, the same buffers;
  launches  median ms of the "mask_ext" launch and of "istft" in both modes (per-launch events), the kernels that ran, and the bytes the reduction reads
            (every mask once more) with the HBM rate that gives.
The two modes are timed alternately (off, on, off, on) so that a drift of the device shows in both.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F, TILES = 256, 1024, 64
CONFIGS = {"f32": (4, (1, 0, 1, 1), (0.25, 0.0, 0.25, 0.25)), "f16": (5, (1, 0, 1, 1, 1), (0.25, 0.0, 0.25, 0.25, 0.25))}


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def per_launch(eng, fn, steps):
    """median ms per launch name over `steps` calls (per-launch events; a name launched several times in one call is summed per call)"""
    fn()
    eng.set_timing(True)
    for _ in range(steps):
        fn()
    tim = eng.get_timing()
    kn = eng.get_timing_kernels()
    eng.set_timing(False)
    per_call = len(tim) // steps
    sums = []
    for i in range(steps):
        d = {}
        for name, t in tim[i * per_call:(i + 1) * per_call]:
            d[name] = d.get(name, 0.0) + t
        sums.append(d)
    return {k: round(statistics.median(d[k] for d in sums), 4) for k in sums[0]}, dict(kn[:per_call])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_ext_bench.json"))
    a = ap.parse_args()
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    dev = torch.device("cuda", 0)
    res = []
    for prec in ("f32", "f16"):
        S, modes, oob = CONFIGS[prec]
        eng = srt.Engine(F=F, T=T, stem_modes=modes, oob_weights=oob, variant=srt.VARIANT_VST, max_tiles=TILES, device=dev,
                         precision={"f32": srt.PREC_F32, "f16": srt.PREC_F16}[prec])
        for s in range(S):
            eng.set_coeff(s, synth_weights(s, dev))
        rows = TILES * T
        g = torch.Generator(device=dev).manual_seed(8)
        L = (torch.rand(rows * 1024, device=dev, generator=g) - 0.5) * 0.2
        R = 0.5 * L + (torch.rand(rows * 1024, device=dev, generator=g) - 0.5) * 0.1
        out = torch.empty((S, 2, eng.L.srtIstftLength(rows)), device=dev)

        def sep(mode):
            eng.set_mask_extension(mode)
            return lambda: eng.separate(L, R, out)
        runs = [(mode, timed(sep(mode), a.steps, a.warmup)) for mode in ("constant", "average") * 2]
        pl_off, kn_off = per_launch(eng, sep("constant"), a.steps)
        pl_on, kn_on = per_launch(eng, sep("average"), a.steps)
        half = kn_on["mask_ext"].startswith("srt_mask_ext_kernel<true")
        nbytes = S * TILES * 2 * T * F * (2 if half else 4)
        off = statistics.median(r["ms_median"] for m, r in runs if m == "constant")
        on = statistics.median(r["ms_median"] for m, r in runs if m == "average")
        rec = {"precision": prec, "stems": S, "rows": rows, "tiles": TILES, "runs": [{"mode": m, **r} for m, r in runs],
               "off_ms": round(off, 4), "on_ms": round(on, 4), "on_minus_off_ms": round(on - off, 4), "on_over_off": round(on / off, 4),
               "mask_ext_ms": pl_on["mask_ext"], "istft_ms": {"off": pl_off["istft"], "on": pl_on["istft"]},
               "kernels": {"mask_ext": kn_on["mask_ext"], "istft_on": kn_on["istft"], "istft_off": kn_off["istft"]},
               "mask_bytes_read": nbytes, "mask_ext_GB_per_s": round(nbytes / (pl_on["mask_ext"] * 1e-3) / 1e9, 1)}
        print(json.dumps(rec), flush=True)
        res.append(rec)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
