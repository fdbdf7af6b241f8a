"""Measure the stem remix (srtSetMix) against the mix-off path, in one process.

    python scripts/mix_bench.py [--steps 20] [--warmup 3] [--minutes 10] [--out profiles/mix_bench.json]

Bench shape: F = 1024, T = 256, max_tiles = 64, srtSeparate of a 64-tile signal (16 384 rows); 4 stems fp32 and the 5-stem fp16 mode.  Device events, the
median (with min and max) of `steps` calls after `warmup` calls, as the other bench scripts do.  Per precision:
  off       the mix off: the baseline - the path and the kernels of the parent commit (tests/test_mix.py holds set_mix(None) to them bit for bit and launch
            for launch); the fp16 mode then runs its half masks;
  mix1      one output, karaoke: the input minus stem 1;
  mix2      two outputs: stem 1 and the input minus stem 1;
  launches  median ms of "istft" in the three settings (per-launch events) and the kernels that ran.
The settings are timed alternately (off, mix1, mix2, off, mix1, mix2) so that a drift of the device shows in all of them.
Host stream: separate_host_stream_io of a `minutes`-minute 44.1 kHz stream from pinned memory on the 4-stem fp32 engine - mix off (4 pairs of floats come
down), one output (1 pair), one output with SRT_HOST_OUT_PCM16 (1 pair of 16-bit samples) - wall-clock per call (the call is synchronous), median of three
calls after one, with the bytes each setting downloads.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F, TILES = 256, 1024, 64
CONFIGS = {"f32": (4, (1, 0, 1, 1), (0.25, 0.0, 0.25, 0.25)), "f16": (5, (1, 0, 1, 1, 1), (0.25, 0.0, 0.25, 0.25, 0.25))}


def matrices(S):
    import numpy as np
    karaoke = np.zeros((1, S + 1), np.float32)
    karaoke[0, 1], karaoke[0, S] = -1.0, 1.0
    vocal = np.zeros((1, S + 1), np.float32)
    vocal[0, 1] = 1.0
    return {"off": None, "mix1": karaoke, "mix2": np.concatenate([vocal, karaoke])}


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


def host_stream(eng, S, minutes):
    import torch
    n = int(minutes * 60 * 44100)
    g = torch.Generator().manual_seed(9)
    L = ((torch.rand(n, generator=g) - 0.5) * 0.2).pin_memory()
    R = (0.5 * L + (torch.rand(n, generator=g) - 0.5) * 0.1).pin_memory()
    ln = eng.L.srtIstftLength(eng.L.srtStftRows(n))
    mats = matrices(S)
    res = []
    for name, mat, pcm16 in (("off", mats["off"], False), ("mix1", mats["mix1"], False), ("mix1_pcm16", mats["mix1"], True)):
        eng.set_mix(mat)
        pairs = eng.outputs
        out = torch.empty((pairs, ln, 2), dtype=torch.int16).pin_memory() if pcm16 else torch.empty((pairs, 2, ln), dtype=torch.float32).pin_memory()
        secs = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.separate_host_stream_io((L, R), out_pcm16=pcm16, out=out, pinned=True)
            secs.append(time.perf_counter() - t0)
        secs = secs[1:]
        nbytes = pairs * 2 * ln * (2 if pcm16 else 4)
        res.append({"setting": name, "pairs": pairs, "pcm16": pcm16, "samples": n, "bytes_down": nbytes, "s_median": round(statistics.median(secs), 4),
                    "s_min": round(min(secs), 4), "s_max": round(max(secs), 4)})
        print(json.dumps(res[-1]), flush=True)
        del out
    eng.set_mix(None)
    eng.release_staging()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_bench.json"))
    a = ap.parse_args()
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    dev = torch.device("cuda", 0)
    res = {"step": [], "host_stream": []}
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
        mats = matrices(S)

        def sep(name):
            eng.set_mix(mats[name])
            return lambda: eng.separate(L, R, out)
        order = ("off", "mix1", "mix2")
        runs = [(name, timed(sep(name), a.steps, a.warmup)) for name in order * 2]
        launches = {name: per_launch(eng, sep(name), a.steps) for name in order}
        med = {name: statistics.median(r["ms_median"] for m, r in runs if m == name) for name in order}
        rec = {"precision": prec, "stems": S, "rows": rows, "tiles": TILES, "runs": [{"setting": m, **r} for m, r in runs],
               "step_ms": {k: round(v, 4) for k, v in med.items()},
               "minus_off_ms": {k: round(med[k] - med["off"], 4) for k in order[1:]}, "over_off": {k: round(med[k] / med["off"], 4) for k in order[1:]},
               "istft_ms": {k: launches[k][0]["istft"] for k in order}, "istft_kernel": {k: launches[k][1]["istft"] for k in order}}
        print(json.dumps(rec), flush=True)
        res["step"].append(rec)
        if prec == "f32":
            del L, R, out
            res["host_stream"] = host_stream(eng, S, a.minutes)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
