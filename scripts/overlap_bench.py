"""Measure overlapped network tiles (srtSetOverlap): what the default path costs after the change, what an overlap costs, what it buys.

    python scripts/overlap_bench.py [--parent-root DIR] [--steps 20] [--warmup 3] [--out profiles/overlap_bench.json]

Bench shape: F = 1024, T = 256, max_tiles = 64; 4 stems fp32 and the 5-stem fp16 mode.  Device events, the median (with min and max) of `steps` calls after
`warmup` calls, as the other bench scripts do.  Sections:
  default   srtSeparate of a 64-tile signal (16 384 rows) at O = 0, on this tree and - with --parent-root, a checkout of the parent commit whose library is
            built - on the parent, in fresh child processes run alternately (parent, this, parent, this) in one session.  The change leaves the default
            path alone when this tree's median lies inside the parent's own min..max spread.
  cost      a signal of 12 352 rows at O = 64 = exactly 64 overlapped tiles (63 * 192 + 256): the same 64-tile forward as `default`, transforms over fewer
            rows.  The whole call against the 64-tile srtSeparate (+ 3 % allowed); stft / istft per row against the O = 0 kernels at EQUAL rows with the
            HBM bytes each form moves (algorithmic: PCM, spectrum, magnitudes, masks, stems); ms per second of audio at O = 0, 32, 64, 128 on one
            8 320-row signal (64 tiles at O = 128) against the derived T / (T - O).
  buys      on the oracle's synthetic clip with tones: mean |m(r) - m(r-1)| of the per-row masks over the rows r that are multiples of T (the back-to-back
            seams) and over all other rows, at O = 0, 32, 64.  Recorded, not asserted: the weights are synthetic, so this shows the continuity of the masks
            across tile boundaries, not separation quality.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a child of the `default` section imports the package of the tree it measures (OVERLAP_BENCH_ROOT) and bench.synth_weights from this one
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get("OVERLAP_BENCH_ROOT", ROOT))

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


def noise(rows, seed, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    L = (torch.rand(rows * 1024, device=dev, generator=g) - 0.5) * 0.2
    R = 0.5 * L + (torch.rand(rows * 1024, device=dev, generator=g) - 0.5) * 0.1
    return L, R


def child_default(steps, warmup):
    """srtSeparate of the 64-tile signal at O = 0 in both modes, with the API the parent commit already has; one JSON line"""
    import torch
    dev = torch.device("cuda", 0)
    res = {}
    for prec in ("f32", "f16"):
        eng, S = engine(prec, dev)
        L, R = noise(TILES * T, 8, dev)
        out = torch.empty((S, 2, eng.L.srtIstftLength(TILES * T)), device=dev)
        res[prec] = timed(lambda: eng.separate(L, R, out), steps, warmup)
        eng.close()
    print("OVERLAP_BENCH_CHILD " + json.dumps(res), flush=True)


def section_default(parent_root, steps, warmup):
    def child(root):
        env = dict(os.environ, OVERLAP_BENCH_ROOT=root)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-default", "--steps", str(steps), "--warmup", str(warmup)],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit("overlap_bench: child on %s failed (%d):\n%s" % (root, r.returncode, r.stderr[-2000:]))
        return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("OVERLAP_BENCH_CHILD "))[len("OVERLAP_BENCH_CHILD "):])
    order = (["parent", "this"] * 2) if parent_root else ["this"] * 2
    runs = [(who, child(parent_root if who == "parent" else ROOT)) for who in order]
    out = {"section": "default path, O = 0, 64 tiles", "rows": TILES * T, "runs": [{"tree": w, **r} for w, r in runs]}
    if parent_root:
        for prec in ("f32", "f16"):
            lo = min(r[prec]["ms_min"] for w, r in runs if w == "parent")
            hi = max(r[prec]["ms_max"] for w, r in runs if w == "parent")
            med = [r[prec]["ms_median"] for w, r in runs if w == "this"]
            out[prec] = {"parent_min": lo, "parent_max": hi, "parent_medians": [r[prec]["ms_median"] for w, r in runs if w == "parent"], "this_medians": med,
                         "inside_parent_spread": all(lo <= m <= hi for m in med)}
    return out


def hbm_bytes(rows, O, S, len_out, mask_bytes=4):
    """algorithmic HBM bytes of the two transforms on `rows` rows: PCM in, spectrum + magnitudes out / spectrum (once: the stems of a run share it in
    L2) + masks in, stems out.  With an overlap O of every T - O rows are written (STFT) and read (inverse) twice."""
    import spleeterrt_amd.stream as st
    nt = st.overlap_tiles(rows, T, O)
    dup = sum(1 for r in range(rows) if O and min(r // (T - O), nt - 1) > 0 and r - min(r // (T - O), nt - 1) * (T - O) < O)
    spec = 2 * rows * 2052 * 8
    pad = ((nt - 1) * (T - O) + T - rows) * 2 * F * 4
    return {"stft": 2 * rows * 1024 * 4 + spec + 2 * (rows + dup) * F * 4 + pad, "istft": spec + S * 2 * (rows + dup) * F * mask_bytes + S * 2 * len_out * 4, "rows_in_two_tiles": dup}


def section_cost(steps, warmup):
    import torch
    from spleeterrt_amd import stream
    dev = torch.device("cuda", 0)
    res = []
    for prec in ("f32", "f16"):
        eng, S = engine(prec, dev)
        rows64 = 63 * (T - 64) + T
        assert stream.overlap_tiles(rows64, T, 64) == TILES and rows64 == 12352
        sig = {rows: noise(rows, 9 + rows % 7, dev) for rows in (TILES * T, rows64, 8320)}
        outs = {rows: torch.empty((S, 2, eng.L.srtIstftLength(rows)), device=dev) for rows in sig}

        def sep(rows, O):
            eng.set_overlap(O)
            return lambda: eng.separate(sig[rows][0], sig[rows][1], outs[rows])
        base = timed(sep(TILES * T, 0), steps, warmup)
        ov = timed(sep(rows64, 64), steps, warmup)
        eq = timed(sep(rows64, 0), steps, warmup)
        pl_ov = per_launch(eng, sep(rows64, 64), steps)
        pl_eq = per_launch(eng, sep(rows64, 0), steps)
        pl_base = per_launch(eng, sep(TILES * T, 0), steps)
        eng.set_overlap(64)
        eng.set_timing(True)
        eng.separate(sig[rows64][0], sig[rows64][1], outs[rows64])
        kn = eng.get_timing_kernels()
        eng.set_timing(False)
        ln = eng.L.srtIstftLength(rows64)
        mb = 2 if "true>" in kn[-1][1] and prec == "f16" else 4     # the fp16 mode's own masks are halves where the half-mask inverse form ran
        rec = {"section": "cost of overlap", "precision": prec, "stems": S,
               "separate_64_tiles_O0": dict(base, rows=TILES * T), "separate_64_overlapped_tiles_O64": dict(ov, rows=rows64),
               "separate_equal_rows_O0": dict(eq, rows=rows64, tiles=stream.overlap_tiles(rows64, T, 0)),
               "overlap_over_64_tile_call": round(ov["ms_median"] / base["ms_median"], 4), "within_3_percent": ov["ms_median"] <= 1.03 * base["ms_median"],
               "kernels_O64": {"stft": kn[0][1], "istft": kn[-1][1]},
               "stft_ms": {"O64": pl_ov["stft"], "O0_equal_rows": pl_eq["stft"], "O0_64_tiles": pl_base["stft"]},
               "istft_ms": {"O64": pl_ov["istft"], "O0_equal_rows": pl_eq["istft"], "O0_64_tiles": pl_base["istft"]},
               "stft_us_per_row": {"O64": round(1e3 * pl_ov["stft"] / rows64, 5), "O0": round(1e3 * pl_eq["stft"] / rows64, 5)},
               "istft_us_per_row": {"O64": round(1e3 * pl_ov["istft"] / rows64, 5), "O0": round(1e3 * pl_eq["istft"] / rows64, 5)},
               "hbm_bytes": {"O64": hbm_bytes(rows64, 64, S, ln, mb), "O0": hbm_bytes(rows64, 0, S, ln, mb)}}
        sweep = []
        secs = 8320 * 1024 / 44100.0
        for O in (0, 32, 64, 128):
            t = timed(sep(8320, O), steps, warmup)
            sweep.append({"O": O, "tiles": stream.overlap_tiles(8320, T, O), **t, "ms_per_second_of_audio": round(t["ms_median"] / secs, 5),
                          "T_over_T_minus_O": round(T / (T - O), 4)})
        for s in sweep:
            s["over_O0"] = round(s["ms_median"] / sweep[0]["ms_median"], 4)
        rec["sweep_8320_rows"] = sweep
        print(json.dumps(rec), flush=True)
        res.append(rec)
        eng.close()
    return res


def blend_rows(masks, rows, O):
    """per-row masks [S][2][rows][F] from masks [S][tiles][2][T][F] in the overlapped layout (the rule of include/spleeterrt_amd.h, on the device with torch)"""
    import torch
    nt, st = masks.shape[1], T - O
    mm = masks.permute(1, 3, 0, 2, 4)                       # [tiles][T][S][2][F]
    r = torch.arange(rows, device=masks.device)
    j1 = torch.clamp(r // st, max=nt - 1)
    k = r - j1 * st
    b = mm[j1, k]                                           # [rows][S][2][F]
    if O:
        two = (j1 > 0) & (k < O)
        a = mm[torch.clamp(j1 - 1, min=0), torch.clamp(k + st, max=T - 1)]
        w = ((k.float() + 0.5) / O)[:, None, None, None]
        b = torch.where(two[:, None, None, None], a + w * (b - a), b)
    return b.permute(1, 2, 0, 3)


def section_buys():
    import torch
    from oracle import pyoracle as orc
    from spleeterrt_amd import stream
    dev = torch.device("cuda", 0)
    eng, S = engine("f32", dev)
    rows = 8 * T + 100
    Lh, Rh = orc.synth_audio(rows * 1024 - 300, 4711, True)
    L, R = torch.from_numpy(Lh).to(dev), torch.from_numpy(Rh).to(dev)
    out = []
    for O in (0, 32, 64):
        eng.set_overlap(O)
        spec, mag = eng.stft(L, R)
        m = blend_rows(eng.forward(mag), rows, O)           # [S][2][rows][F]
        d = (m[:, :, 1:] - m[:, :, :-1]).abs().mean(dim=(0, 1, 3)).cpu().numpy()    # d[i]: rows i + 1 against i
        r = 1 + torch.arange(rows - 1).numpy()
        seam = (r % T) == 0
        own = (r % (T - O)) == 0
        out.append({"O": O, "tiles": stream.overlap_tiles(rows, T, O), "mean_abs_step_rows_multiple_of_T": float(d[seam].mean()), "mean_abs_step_other_rows": float(d[~seam].mean()),
                    "mean_abs_step_first_rows_of_tiles": float(d[own].mean()), "max_abs_step": float(d.max())})
    eng.close()
    rec = {"section": "what it buys: continuity of the masks (synthetic weights: not separation quality)", "clip": "oracle synth_audio with tones, %d rows" % rows, "steps": out}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built (spleeterrt_amd/libspleeterrt_amd.so)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_bench.json"))
    ap.add_argument("--child-default", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_default:
        return child_default(a.steps, a.warmup)
    res = [section_default(a.parent_root and os.path.abspath(a.parent_root), a.steps, a.warmup)]
    print(json.dumps(res[0]), flush=True)
    res += section_cost(a.steps, a.warmup)
    res.append(section_buys())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
