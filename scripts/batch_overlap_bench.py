"""Measure srtSeparateBatchOverlap (overlapped tiles inside every track of a packed batch).

    python scripts/batch_overlap_bench.py [--parent-root DIR] [--steps 20] [--warmup 3] [--out profiles/batch_overlap_bench.json]

Bench shape: F = 1024, T = 256, max_tiles = 64; 4 stems fp32 and the 5-stem fp16 mode.  Device events, the median (with min and max) of `steps` calls after
`warmup` calls, as scripts/overlap_bench.py does.  The clips are the 32 x 10 s of scripts/batch_bench.py (441 000 samples: 431 rows; two tiles each
back to back, and two overlapped tiles each at O = 64: 64 packed tiles either way).  Sections:
  (a) default   srtSeparateBatch on the clips, on this tree and - with --parent-root, a checkout of the parent commit whose library is built - on the parent,
                in fresh child processes run alternately (parent, this, parent, this).  The change leaves that path alone when this tree's medians lie
                inside the parent's own min..max spread.
  (b) gain      the clips at O = 64 as ONE srtSeparateBatchOverlap call against 32 srtSeparate calls after srtSetOverlap(64).
  (c) cost      that batch call against srtSeparateBatch on a list that takes the same number of packed tiles (the same clips at O = 0), with the two
                transforms per launch (stft_batch / istft_batch of either form).
No ratio is fixed for (b) or (c) in advance; they are recorded.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a child of section (a) imports the package of the tree it measures (BATCH_OVERLAP_BENCH_ROOT) and bench.synth_weights from this one
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get("BATCH_OVERLAP_BENCH_ROOT", ROOT))

T, F, TILES, O_BENCH = 256, 1024, 64, 64
CLIPS, CLIP_SAMPLES = 32, 441000
CONFIGS = {"f32": (4, (1, 0, 1, 1), (0.25, 0.0, 0.25, 0.25)), "f16": (5, (1, 0, 1, 1, 1), (0.25, 0.0, 0.25, 0.25, 0.25))}
TAG = "BATCH_OVERLAP_BENCH_CHILD "


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
    eng.set_timing(False)
    per_call = len(tim) // steps
    sums = []
    for i in range(steps):
        d = {}
        for name, t in tim[i * per_call:(i + 1) * per_call]:
            d[name] = d.get(name, 0.0) + t
        sums.append(d)
    return {k: round(statistics.median(d[k] for d in sums), 4) for k in sums[0]}


def engine(prec, dev):
    import spleeterrt_amd as srt
    from bench import synth_weights
    S, modes, oob = CONFIGS[prec]
    eng = srt.Engine(F=F, T=T, stem_modes=modes, oob_weights=oob, variant=srt.VARIANT_VST, max_tiles=TILES, device=dev,
                     precision={"f32": srt.PREC_F32, "f16": srt.PREC_F16}[prec])
    for s in range(S):
        eng.set_coeff(s, synth_weights(s, dev))
    return eng, S


def clips(dev):
    """the seeded stereo noise clips of scripts/batch_bench.py, case (a)"""
    import torch
    g = torch.Generator(device=dev).manual_seed(7)
    out = []
    for _ in range(CLIPS):
        L = (torch.rand(CLIP_SAMPLES, device=dev, generator=g) - 0.5) * 0.2
        R = 0.5 * L + (torch.rand(CLIP_SAMPLES, device=dev, generator=g) - 0.5) * 0.1
        out.append((L, R))
    return out


def outputs(eng, S, tr, dev):
    import torch
    return [torch.empty((S, 2, eng.L.srtIstftLength(eng.L.srtStftRows(L.numel()))), device=dev) for L, _ in tr]


def child_default(steps, warmup):
    """srtSeparateBatch on the clips in both modes, with the API the parent commit already has; one JSON line"""
    import torch
    dev = torch.device("cuda", 0)
    res = {}
    for prec in ("f32", "f16"):
        eng, S = engine(prec, dev)
        tr = clips(dev)
        outs = outputs(eng, S, tr, dev)
        res[prec] = timed(lambda: eng.separate_batch(tr, outs), steps, warmup)
        eng.close()
    print(TAG + json.dumps(res), flush=True)


def section_default(parent_root, steps, warmup):
    def child(root):
        env = dict(os.environ, BATCH_OVERLAP_BENCH_ROOT=root)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-default", "--steps", str(steps), "--warmup", str(warmup)],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit("batch_overlap_bench: child on %s failed (%d):\n%s" % (root, r.returncode, r.stderr[-2000:]))
        return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith(TAG))[len(TAG):])
    order = (["parent", "this"] * 2) if parent_root else ["this"] * 2
    runs = [(who, child(parent_root if who == "parent" else ROOT)) for who in order]
    out = {"section": "(a) default path: srtSeparateBatch, 32 clips x 10 s, 64 packed tiles", "runs": [{"tree": w, **r} for w, r in runs]}
    if parent_root:
        for prec in ("f32", "f16"):
            lo = min(r[prec]["ms_min"] for w, r in runs if w == "parent")
            hi = max(r[prec]["ms_max"] for w, r in runs if w == "parent")
            med = [r[prec]["ms_median"] for w, r in runs if w == "this"]
            out[prec] = {"parent_min": lo, "parent_max": hi, "parent_medians": [r[prec]["ms_median"] for w, r in runs if w == "parent"], "this_medians": med,
                         "inside_parent_spread": all(lo <= m <= hi for m in med)}
    return out


def section_overlap(steps, warmup):
    import torch
    from spleeterrt_amd import stream
    dev = torch.device("cuda", 0)
    res = []
    for prec in ("f32", "f16"):
        eng, S = engine(prec, dev)
        tr = clips(dev)
        outs = outputs(eng, S, tr, dev)
        ns = [L.numel() for L, _ in tr]
        g_ov, g_0 = stream.pack_tracks(ns, T, TILES, overlap=O_BENCH), stream.pack_tracks(ns, T, TILES)
        assert len(g_ov) == 1 and len(g_0) == 1 and g_ov[0].ntiles == TILES and g_0[0].ntiles == TILES

        def loop():
            for (L, R), o in zip(tr, outs):
                eng.separate(L, R, o)
        batch_ov = timed(lambda: eng.separate_batch(tr, outs, overlap=O_BENCH), steps, warmup)
        eng.set_overlap(O_BENCH)
        loop_ov = timed(loop, steps, warmup)
        eng.set_overlap(0)
        batch_0 = timed(lambda: eng.separate_batch(tr, outs, overlap=0), steps, warmup)
        batch_ov2 = timed(lambda: eng.separate_batch(tr, outs, overlap=O_BENCH), steps, warmup)      # (once more after the O = 0 calls: the order of the two)
        pl_ov = per_launch(eng, lambda: eng.separate_batch(tr, outs, overlap=O_BENCH), steps)
        pl_0 = per_launch(eng, lambda: eng.separate_batch(tr, outs, overlap=0), steps)
        eng.set_timing(True)
        eng.separate_batch(tr, outs, overlap=O_BENCH)
        kn = eng.get_timing_kernels()
        eng.set_timing(False)
        rec = {"section": "(b) gain over the loop, (c) cost over srtSeparateBatch at equal packed tiles", "precision": prec, "stems": S, "T": T, "F": F,
               "max_tiles": TILES, "overlap": O_BENCH, "tracks": CLIPS, "rows_per_track": stream.stft_rows(CLIP_SAMPLES), "packed_tiles": TILES,
               "steps": steps, "warmup": warmup,
               "batch_overlap_call": batch_ov, "batch_overlap_call_again": batch_ov2, "loop_32_srtSeparate_overlap": loop_ov, "srtSeparateBatch_O0": batch_0,
               "b_speedup_batch_over_loop": round(loop_ov["ms_median"] / batch_ov["ms_median"], 3),
               "c_overlap_batch_over_plain_batch": round(batch_ov["ms_median"] / batch_0["ms_median"], 4),
               "kernels_overlap": {"stft_batch": kn[0][1], "istft_batch": kn[-1][1]},
               "stft_batch_ms": {"overlap": pl_ov["stft_batch"], "O0": pl_0["stft_batch"]},
               "istft_batch_ms": {"overlap": pl_ov["istft_batch"], "O0": pl_0["istft_batch"]}}
        print(json.dumps(rec), flush=True)
        res.append(rec)
        eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built (spleeterrt_amd/libspleeterrt_amd.so)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_overlap_bench.json"))
    ap.add_argument("--child-default", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_default:
        return child_default(a.steps, a.warmup)
    res = [section_default(a.parent_root and os.path.abspath(a.parent_root), a.steps, a.warmup)]
    print(json.dumps(res[0]), flush=True)
    res += section_overlap(a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
