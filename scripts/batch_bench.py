"""Time srtSeparateBatch (many independent tracks in one packed batch) against separating the tracks one call at a time, with device events, after warm-up.

    python scripts/batch_bench.py [--steps 10] [--warmup 3] [--out profiles/batch_bench.json]

Bench shape: F = 1024, T = 256, 4 stems, max_tiles = 64, fp32 (and the (a) case once more in the fp16 mode).  Cases:
  (a) 32 clips of 10 s (441 000 samples: 431 rows, 2 tiles each, 64 packed tiles): one srtSeparateBatch call, 32 srtSeparate calls on the same engine, and
      one srtSeparate of a single 64-tile signal (the headline step);
  (b) 64 clips of 5..40 s (seeded lengths) through Engine.separate_batch, which cuts them into calls of <= 64 tiles;
  (c) the batched transforms against the single-signal ones at equal rows: stft_batch / istft_batch of (a) against stft / istft of one signal of the same
      total row count (per-launch events, srtGetTiming, median over the timed calls).
Every time is the median (with min and max) of `steps` event-timed calls; one JSON line per case, all of them written to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F, S, TILES = 256, 1024, 4, 64


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


def run(precision, steps, warmup, full):
    import random
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    dev = torch.device("cuda", 0)
    prec = {srt.PREC_F32: "f32", srt.PREC_F16: "f16"}[precision]
    eng = srt.Engine(F=F, T=T, stem_modes=(1, 0, 1, 1), oob_weights=(0.25, 0.0, 0.25, 0.25), variant=srt.VARIANT_VST, max_tiles=TILES, device=dev,
                     precision=precision)
    for s in range(S):
        eng.set_coeff(s, synth_weights(s, dev))
    base = {"precision": prec, "T": T, "F": F, "stems": S, "max_tiles": TILES, "steps": steps, "warmup": warmup}
    res = []

    def emit(r):
        r = dict(base, **r)
        print(json.dumps(r), flush=True)
        res.append(r)

    # (a) 32 clips of 10 s
    tr = clips([441000] * 32, 7, dev)
    ns = [L.numel() for L, _ in tr]
    rows = [eng.L.srtStftRows(n) for n in ns]
    outs = [torch.empty((S, 2, eng.L.srtIstftLength(r)), device=dev) for r in rows]
    ntiles = sum((r + T - 1) // T for r in rows)
    batch = timed(lambda: eng.separate_batch(tr, outs), steps, warmup)
    loop = timed(lambda: [eng.separate(L, R, o) for (L, R), o in zip(tr, outs)], steps, warmup)
    n64 = TILES * T * 1024
    big = clips([n64], 8, dev)[0]
    out64 = torch.empty((S, 2, eng.L.srtIstftLength(eng.L.srtStftRows(n64))), device=dev)
    single = timed(lambda: eng.separate(big[0], big[1], out64), steps, warmup)
    emit({"case": "(a) 32 clips x 10 s", "tracks": 32, "samples_per_track": ns[0], "rows_per_track": rows[0], "packed_tiles": ntiles,
          "batch_call": batch, "loop_32_srtSeparate": loop, "single_64_tile_signal": single,
          "speedup_batch_over_loop": round(loop["ms_median"] / batch["ms_median"], 3),
          "batch_over_single_64_tiles": round(batch["ms_median"] / single["ms_median"], 4)})

    # (c) batched transforms against the single-signal ones at the same total rows
    tot_rows = sum(rows)
    eq = clips([tot_rows * 1024], 9, dev)[0]
    assert eng.L.srtStftRows(eq[0].numel()) == tot_rows
    outeq = torch.empty((S, 2, eng.L.srtIstftLength(tot_rows)), device=dev)
    pb = per_launch(eng, lambda: eng.separate_batch(tr, outs), steps)
    ps = per_launch(eng, lambda: eng.separate(eq[0], eq[1], outeq), steps)
    p64 = per_launch(eng, lambda: eng.separate(big[0], big[1], out64), steps)
    emit({"case": "(c) transforms at equal rows", "rows": tot_rows, "packed_rows_incl_tile_padding": ntiles * T,
          "stft_batch_ms": pb.get("stft_batch"), "stft_ms": ps.get("stft"), "istft_batch_ms": pb.get("istft_batch"), "istft_ms": ps.get("istft"),
          "stft_batch_over_stft": round(pb["stft_batch"] / ps["stft"], 4), "istft_batch_over_istft": round(pb["istft_batch"] / ps["istft"], 4),
          "single_64_tile_signal": {"rows": TILES * T, "stft_ms": p64.get("stft"), "istft_ms": p64.get("istft")},
          "batch_per_launch_ms": pb})

    if full:
        # (b) 64 clips of 5..40 s through separate_batch (several calls of <= 64 tiles)
        rnd = random.Random(11)
        secs = [rnd.uniform(5.0, 40.0) for _ in range(64)]
        trb = clips([int(x * 44100) for x in secs], 10, dev)
        from spleeterrt_amd import stream
        nsb = [L.numel() for L, _ in trb]
        groups = stream.pack_tracks(nsb, T, TILES)
        outsb = [torch.empty((S, 2, eng.L.srtIstftLength(eng.L.srtStftRows(n))), device=dev) for n in nsb]
        mixed = timed(lambda: eng.separate_batch(trb, outsb), steps, warmup)
        loopb = timed(lambda: [eng.separate(L, R, o) for (L, R), o in zip(trb, outsb)], max(2, steps // 2), 1)
        tiles_b = sum(g.ntiles for g in groups)
        emit({"case": "(b) 64 clips of 5..40 s", "tracks": 64, "seconds_total": round(sum(secs), 1), "calls": len(groups), "packed_tiles": tiles_b,
              "separate_batch": mixed, "loop_64_srtSeparate": loopb, "speedup_batch_over_loop": round(loopb["ms_median"] / mixed["ms_median"], 3),
              "ms_per_packed_tile": round(mixed["ms_median"] / tiles_b, 4)})
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.json"))
    a = ap.parse_args()
    import spleeterrt_amd as srt
    res = run(srt.PREC_F32, a.steps, a.warmup, True)
    res += run(srt.PREC_F16, a.steps, a.warmup, False)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
