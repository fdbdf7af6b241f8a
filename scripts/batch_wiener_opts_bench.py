"""Time srtSeparateBatchWienerEx (the Wiener filter per track of a packed batch with per-call options) against the calls it replaces, with
device events, after warm-up.

    python scripts/batch_wiener_opts_bench.py [--steps 20] [--warmup 3] [--parent-root PARENT_CHECKOUT] [--out profiles/batch_wiener_opts_bench.json]

Bench shape: F = 1024, T = 256, max_tiles = 64, 4 stems fp32 and 5 stems fp16, iterations = 1, clips of 10 s (431 rows: 2 tiles each back to back and at
O = 64, so 32 clips fill the 64 packed tiles either way).  Cases, per precision; the compared calls are timed alternately (one call of each per step) in one process:
  (i)   every option off against srtSeparateBatchWiener (the launch lists are equal);
  (ii)  O = 64 against the same clips as a loop of 32 srtSeparateWiener calls at O = 64;
  (iii) (ii) with the average mask extension;
  (iv)  (ii) with one karaoke output per track;
  (v)   the filter off: srtSeparateBatch of the clips and srtSeparate of one 64-tile signal.  With --parent-root the same case is run in child processes that
        import spleeterrt_amd from that checkout (built there) and from this tree, alternately, twice each: nothing on those paths changes, so this tree's
        medians must lie inside the parent's min..max.
Per-launch ms (srtGetTiming) of the option call are recorded with (iii) and (iv).  Every time is the median (with min and max) of `steps` event-timed calls
after `warmup` calls; one JSON line per case, all of them written to --out.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

T, F, TILES, ITERS, OV = 256, 1024, 64, 1, 64


def filter_off(precision, S, steps, warmup, label):
    """case (v) alone: what the parent commit's library can run as well"""
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    from batch_wiener_bench import clips, timed_alternately
    dev = torch.device("cuda", 0)
    eng = srt.Engine(F=F, T=T, stem_modes=(1, 0, 1, 1, 0)[:S], oob_weights=(0.25, 0.0, 0.25, 0.25, 0.25)[:S], variant=srt.VARIANT_VST, max_tiles=TILES,
                     device=dev, precision=precision)
    for s in range(S):
        eng.set_coeff(s, synth_weights(s, dev))
    tr = clips([441000] * 32, 7, dev)
    outs = [torch.empty((S, 2, eng.L.srtIstftLength(eng.L.srtStftRows(L.numel()))), device=dev) for L, _ in tr]
    n64 = TILES * T * 1024
    big = clips([n64], 8, dev)[0]
    out64 = torch.empty((S, 2, eng.L.srtIstftLength(eng.L.srtStftRows(n64))), device=dev)
    off = timed_alternately({"srtSeparateBatch": lambda: eng.separate_batch(tr, outs),
                             "srtSeparate_64_tiles": lambda: eng.separate(big[0], big[1], out64)}, steps, warmup)
    eng.close()
    r = dict({"precision": {srt.PREC_F32: "f32", srt.PREC_F16: "f16"}[precision], "T": T, "F": F, "stems": S, "max_tiles": TILES, "steps": steps, "warmup": warmup,
              "library": label, "case": "(v) filter off"}, **off)
    print(json.dumps(r), flush=True)
    return [r]


def run(precision, S, steps, warmup):
    import numpy as np
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    from batch_wiener_bench import clips, per_launch, timed_alternately
    dev = torch.device("cuda", 0)
    prec = {srt.PREC_F32: "f32", srt.PREC_F16: "f16"}[precision]
    eng = srt.Engine(F=F, T=T, stem_modes=(1, 0, 1, 1, 0)[:S], oob_weights=(0.25, 0.0, 0.25, 0.25, 0.25)[:S], variant=srt.VARIANT_VST, max_tiles=TILES,
                     device=dev, precision=precision)
    for s in range(S):
        eng.set_coeff(s, synth_weights(s, dev))
    base = {"precision": prec, "T": T, "F": F, "stems": S, "max_tiles": TILES, "iterations": ITERS, "steps": steps, "warmup": warmup, "library": "this tree"}
    res = []

    def emit(r):
        r = dict(base, **r)
        print(json.dumps(r), flush=True)
        res.append(r)

    tr = clips([441000] * 32, 7, dev)
    rows = [eng.L.srtStftRows(L.numel()) for L, _ in tr]
    assert sum(eng.L.srtOverlapTiles(r, T, OV) for r in rows) == TILES
    outs = [torch.empty((S, 2, eng.L.srtIstftLength(r)), device=dev) for r in rows]
    karaoke = np.zeros((1, S + 1), np.float32)
    karaoke[0, 0], karaoke[0, S] = -1.0, 1.0
    shape = {"tracks": len(tr), "rows_per_track": rows[0], "real_rows": sum(rows), "packed_tiles": TILES}

    one = timed_alternately({"srtSeparateBatchWienerEx_options_off": lambda: eng.separate_batch_wiener(tr, outs, iterations=ITERS),
                             "srtSeparateBatchWiener": lambda: eng.separate_batch(tr, outs, wiener=ITERS)}, steps, warmup)
    emit(dict({"case": "(i) options off against srtSeparateBatchWiener"}, **shape, **one))
    cases = (("(ii) O = 64", dict(overlap=OV)),
             ("(iii) O = 64, average extension", dict(overlap=OV, mask_extension="average")),
             ("(iv) O = 64, one karaoke output per track", dict(overlap=OV, mix=karaoke)))
    for name, kw in cases:
        both = timed_alternately({"srtSeparateBatchWienerEx": lambda: eng.separate_batch_wiener(tr, outs, iterations=ITERS, **kw),
                                  "loop_32_srtSeparateWiener": lambda: [eng.separate_wiener(L, R, ITERS, out=o, **kw) for (L, R), o in zip(tr, outs)]}, steps, warmup)
        r = dict({"case": name, "overlap": OV, "speedup_batch_over_loop": round(both["loop_32_srtSeparateWiener"]["ms_median"] / both["srtSeparateBatchWienerEx"]["ms_median"], 3)},
                 **shape, **both)
        if name != cases[0][0]:
            r["batch_call_per_launch_ms"] = per_launch(eng, lambda: eng.separate_batch_wiener(tr, outs, iterations=ITERS, **kw), steps)
        emit(r)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: case (v) is then also run on its library, in child processes alternating with this tree's")
    ap.add_argument("--filter-off-only", action="store_true", help="case (v) alone in this process (what the child processes run)")
    ap.add_argument("--package-root", default=None, help="with --filter-off-only: import spleeterrt_amd from this checkout instead")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_wiener_opts_bench.json"))
    a = ap.parse_args()
    res = []
    if a.filter_off_only:
        if a.package_root:
            sys.path.insert(0, os.path.abspath(a.package_root))
        import spleeterrt_amd as srt
        label = a.label or (a.package_root or "this tree")
        res = filter_off(srt.PREC_F32, 4, a.steps, a.warmup, label) + filter_off(srt.PREC_F16, 5, a.steps, a.warmup, label)
    else:
        if a.parent_root:                                            # fresh child processes, before this one opens the device
            for i in (1, 2):
                for label, root in (("parent commit", a.parent_root), ("this tree", None)):
                    tmp = a.out + ".%s_%d.tmp" % (label.split()[0], i)
                    cmd = [sys.executable, os.path.abspath(__file__), "--filter-off-only", "--steps", str(a.steps), "--warmup", str(a.warmup), "--label", label, "--out", tmp]
                    subprocess.check_call(cmd + (["--package-root", root] if root else []), timeout=300)
                    for r in json.load(open(tmp)):
                        res.append(dict(r, process="%s_%d" % (label.split()[0], i)))
                    os.remove(tmp)
        import spleeterrt_amd as srt
        if not a.parent_root:
            res += filter_off(srt.PREC_F32, 4, a.steps, a.warmup, "this tree") + filter_off(srt.PREC_F16, 5, a.steps, a.warmup, "this tree")
        res += run(srt.PREC_F32, 4, a.steps, a.warmup)
        res += run(srt.PREC_F16, 5, a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
