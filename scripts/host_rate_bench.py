#!/usr/bin/env python3
"""Host streams at the caller's sample rate (srtSeparateHostStreamRate), measured at the bench shape (4 stems, 256 x 1024 tiles, pieces of 64 tiles,
fp32, wall clock, median of 3 after 1 warm-up round, the routes measured alternately in one process per stream):

  new_float / new_pcm16        separate_host_rate(rate -> rate), page-locked buffers, float and 16-bit output
  three_call                   what a caller did before: Resampler.resample_host to 44.1 kHz, separate_host_stream_io, resample_host per stem (floats; the route
                               has no 16-bit output).  It exists at the parent commit: the baseline.
  stream44_float / _pcm16      separate_host_stream_io on 44.1 kHz input of the same duration, page-locked: what the converters add when nothing else changes
  rate_in / rate_out           the converters' device time inside one new_float call (srtGetTiming events)
  rate_out_shared / _per_pair  the output converter's kernel on one full piece (64 tiles of 44.1 kHz samples, 4 pairs): one launch whose workgroups compute every
                               pair from each weight load, against one launch per pair (device events, median of 5)

    python scripts/host_rate_bench.py [--minutes 10,60] [--rates 48000,96000]        # -> profiles/host_rate_bench.json

The signal is noise (the timing does not depend on the samples)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, T, STEMS, HOP = 1024, 256, 4, 1024


def _noise(t, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    a = t.numpy()
    for i in range(0, a.size, 1 << 22):
        a[i:i + (1 << 22)] = rng.standard_normal(min(1 << 22, a.size - i), dtype=np.float32) * np.float32(0.1)


def child(minutes, rate, max_tiles, calls, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import spleeterrt_amd as srt
    from spleeterrt_amd import stream
    from bench import synth_weights
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    eng = srt.Engine(F=F, T=T, stem_modes=(1,) * STEMS, oob_weights=(0.25, 0.0, 0.25, 0.25), variant=srt.VARIANT_VST, max_tiles=max_tiles, device=dev)
    for s in range(STEMS):
        eng.set_coeff(s, synth_weights(s, dev))
    n = int(round(minutes * 60 * rate))
    n44 = stream.resample_length(n, rate, 44100)
    len_out, len44 = eng.host_rate_length(n, rate, rate), stream.stft_rows(n44) * HOP + 3072
    pin = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
    Lp, Rp, L44, R44 = pin(n, torch.float32), pin(n, torch.float32), pin(n44, torch.float32), pin(n44, torch.float32)
    for k, t in enumerate((Lp, Rp, L44, R44)):
        _noise(t, k)
    out, out16 = pin((STEMS, 2, len_out), torch.float32), pin((STEMS, len_out, 2), torch.int16)
    out44, out44_16 = pin((STEMS, 2, len44), torch.float32), pin((STEMS, len44, 2), torch.int16)
    r_in, r_out = srt.Resampler(rate, 44100), srt.Resampler(44100, rate)

    def three_call():
        x44 = r_in.resample_host(Lp.numpy(), Rp.numpy())
        y44, _ = eng.separate_host_stream_io(x44)
        return [r_out.resample_host(y44[s, 0], y44[s, 1]) for s in range(STEMS)]
    routes = {"new_float": lambda: eng.separate_host_rate((Lp, Rp), rate, out=out, pinned=True),
              "new_pcm16": lambda: eng.separate_host_rate((Lp, Rp), rate, out_pcm16=True, out=out16, pinned=True),
              "three_call": three_call,
              "stream44_float": lambda: eng.separate_host_stream_io((L44, R44), out=out44, pinned=True),
              "stream44_pcm16": lambda: eng.separate_host_stream_io((L44, R44), out_pcm16=True, out=out44_16, pinned=True)}
    times = dict((k, []) for k in routes)
    for rep in range(warmup + calls):                       # alternately: one round runs every route once
        for name, call in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if rep >= warmup:
                times[name].append(time.perf_counter() - t0)
    res = {"minutes": minutes, "rate": rate, "frames": n, "frames_44k1": n44, "frames_out": len_out, "max_tiles_per_piece": max_tiles, "calls": calls, "warmup": warmup,
           "pieces": len(stream.host_rate_pieces(n, rate, rate, T, 0, max_tiles))}
    for name, ts in times.items():
        res[name] = {"seconds_median": statistics.median(ts), "seconds_min": min(ts), "seconds_max": max(ts)}
    res["new_float_over_three_call"] = res["new_float"]["seconds_median"] / res["three_call"]["seconds_median"]
    res["new_float_over_stream44_float"] = res["new_float"]["seconds_median"] / res["stream44_float"]["seconds_median"]
    res["new_pcm16_over_stream44_pcm16"] = res["new_pcm16"]["seconds_median"] / res["stream44_pcm16"]["seconds_median"]
    eng.set_timing(True)
    eng.separate_host_rate((Lp, Rp), rate, out=out, pinned=True)
    tim = eng.get_timing()
    eng.set_timing(False)
    for name in ("rate_in", "rate_out"):
        ms = [v for k, v in tim if k == name]
        res[name] = {"launches": len(ms), "ms_total": sum(ms), "ms_max": max(ms)}
    res["ms_all_launches_of_the_call"] = sum(v for _, v in tim)
    eng.close()
    # the output converter alone on one full piece: every pair in one launch against one launch per pair
    fin = max_tiles * T * HOP
    g = stream.rs_geometry(44100, rate)
    j1 = stream.rs_computable(g, fin)
    y = torch.randn((2 * STEMS, fin), device=dev)
    o = torch.empty((2 * STEMS, j1), device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def device_ms(call):
        call()
        ms = []
        for _ in range(5):
            a, b = ev(), ev()
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)
    res["rate_out_shared_ms"] = device_ms(lambda: r_out.resample_spans(y, 0, None, fin, 0, j1, out=o))
    res["rate_out_per_pair_ms"] = device_ms(lambda: [r_out.resample_spans(y[2 * p:2 * p + 2], 0, None, fin, 0, j1, out=o[2 * p:2 * p + 2]) for p in range(STEMS)])
    res["rate_out_shared_over_per_pair"] = res["rate_out_shared_ms"] / res["rate_out_per_pair_ms"]
    res["rate_out_piece"] = {"pairs": STEMS, "frames_in": fin, "frames_out": j1}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", default="10,60")
    ap.add_argument("--rates", default="48000,96000")
    ap.add_argument("--max-tiles", type=int, default=64)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_rate_bench.json"))
    ap.add_argument("--case", default="", help="(internal) <minutes>,<rate>")
    a = ap.parse_args()
    if a.case:
        minutes, rate = a.case.split(",")
        print(json.dumps(child(float(minutes), int(rate), a.max_tiles, a.calls, a.warmup)))
        return
    res = {"config": "%d stems, %dx%d tiles, pieces of %d tiles, fp32, noise; wall clock, median of %d timed rounds after %d warm-up, every route once per round, one "
                     "process per stream; page-locked buffers except the three-call route (pageable, as its calls allocate them)" % (STEMS, T, F, a.max_tiles, a.calls, a.warmup),
           "streams": []}
    if os.path.exists(a.out):                               # a run of some streams keeps the others' entries
        old = json.load(open(a.out))
        res["streams"] = [s for s in old.get("streams", []) if "%g,%d" % (s["minutes"], s["rate"]) not in ["%g,%d" % (float(m), int(r)) for m in a.minutes.split(",") for r in a.rates.split(",")]]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for m in a.minutes.split(","):
        for rate in a.rates.split(","):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", "%s,%s" % (m, rate), "--max-tiles", str(a.max_tiles), "--calls", str(a.calls),
                                "--warmup", str(a.warmup)], cwd=ROOT, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit("case %s,%s failed:\n%s\n%s" % (m, rate, r.stdout[-2000:], r.stderr[-4000:]))
            entry = json.loads(r.stdout.strip().splitlines()[-1])
            res["streams"].append(entry)
            print(json.dumps(entry), flush=True)
            open(a.out, "w").write(json.dumps(res, indent=1) + "\n")            # (kept as far as it got)


if __name__ == "__main__":
    main()
