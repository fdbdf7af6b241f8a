#!/usr/bin/env python3
"""24-bit PCM and dithered 16-bit output on the host stream, measured at the bench shape (4 stems, 256 x 1024 tiles, chunks of 64 tiles, fp32,
page-locked buffers, wall clock, median of 3 after 1 warm-up round, the routes measured alternately in one process per stream) through separate_host_stream_io:

  float32            (L, R) float32 in, float32 out: the call without any flag
  pcm24_out          float32 in, packed 24-bit out                  (3/4 of the download)
  pcm16_out          float32 in, 16-bit out                         (1/2 of the download)
  pcm16_dither_out   float32 in, 16-bit out with TPDF dither        (the same bytes; the hash is the only difference)
  pcm24_in_out       packed 24-bit in and out

and, from one timed call per route (srtSetTiming events; the kernel names from srtGetTimingKernels), the device time of every pack and unpack launch.  The float
route's download rate (bytes of the output over its wall clock: the call is download-bound) prices one chunk's download, which the dithered pack's time per chunk is
held against.

    python scripts/pcm24_bench.py [--minutes 10,60] [--parent-root DIR]        # -> profiles/pcm24_bench.json

--parent-root: a built checkout of the parent commit.  Its separate_host_stream and this tree's float32 route are then measured in fresh processes, alternately,
three each; this tree's median must not lie above the parent's slowest process ("float_route_vs_parent").

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
    a = t.numpy().reshape(-1)
    for i in range(0, a.size, 1 << 22):
        m = min(1 << 22, a.size - i)
        a[i:i + m] = rng.integers(0, 256, m, dtype=np.uint8) if a.dtype == np.uint8 else rng.standard_normal(m, dtype=np.float32) * np.float32(0.1)


def _engine(root, max_tiles):
    sys.path.insert(0, root)
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    eng = srt.Engine(F=F, T=T, stem_modes=(1,) * STEMS, oob_weights=(0.25, 0.0, 0.25, 0.25), variant=srt.VARIANT_VST, max_tiles=max_tiles, device=dev)
    for s in range(STEMS):
        eng.set_coeff(s, synth_weights(s, dev))
    return torch, srt, eng


def _timed(torch, routes, calls, warmup):
    times = dict((k, []) for k in routes)
    for rep in range(warmup + calls):                       # alternately: one round runs every route once
        for name, call in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if rep >= warmup:
                times[name].append(time.perf_counter() - t0)
    return dict((k, {"seconds_median": statistics.median(v), "seconds_min": min(v), "seconds_max": max(v)}) for k, v in times.items())


def child_float(root, minutes, max_tiles, calls, warmup):
    """separate_host_stream alone (the call the parent commit has), or this tree's float32 route of separate_host_stream_io, from the package under `root`"""
    torch, srt, eng = _engine(root, max_tiles)
    n = int(round(minutes * 60 * 44100))
    pin = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
    Lp, Rp = pin(n, torch.float32), pin(n, torch.float32)
    _noise(Lp, 0)
    _noise(Rp, 1)
    out = pin((STEMS, 2, eng.L.srtStftRows(n) * HOP + 3072), torch.float32)
    if os.path.abspath(root) == ROOT:
        call = lambda: eng.separate_host_stream_io((Lp, Rp), out=out, pinned=True)
    else:
        call = lambda: eng.separate_host_stream(Lp, Rp, out=out, pinned=True)
    res = _timed(torch, {"float": call}, calls, warmup)["float"]
    eng.close()
    return res


def child(minutes, max_tiles, calls, warmup):
    torch, srt, eng = _engine(ROOT, max_tiles)
    n = int(round(minutes * 60 * 44100))
    ln = eng.L.srtStftRows(n) * HOP + 3072
    pin = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
    Lp, Rp, in24 = pin(n, torch.float32), pin(n, torch.float32), pin((n, 2, 3), torch.uint8)
    for k, t in enumerate((Lp, Rp, in24)):
        _noise(t, k)
    out, out24, out16 = pin((STEMS, 2, ln), torch.float32), pin((STEMS, ln, 2, 3), torch.uint8), pin((STEMS, ln, 2), torch.int16)
    routes = {"float32": lambda: eng.separate_host_stream_io((Lp, Rp), out=out, pinned=True),
              "pcm24_out": lambda: eng.separate_host_stream_io((Lp, Rp), out_bits=24, out=out24, pinned=True),
              "pcm16_out": lambda: eng.separate_host_stream_io((Lp, Rp), out_bits=16, out=out16, pinned=True),
              "pcm16_dither_out": lambda: eng.separate_host_stream_io((Lp, Rp), out_bits=16, dither=True, out=out16, pinned=True),
              "pcm24_in_out": lambda: eng.separate_host_stream_io(in24, out_bits=24, out=out24, pinned=True)}
    chunk = max_tiles * T * HOP
    res = {"minutes": minutes, "frames": n, "frames_out": ln, "max_tiles_per_chunk": max_tiles, "chunks": -(-eng.L.srtStftRows(n) // (max_tiles * T)), "calls": calls, "warmup": warmup,
           "bytes_up": {"float32": n * 8, "pcm24": n * 6}, "bytes_down": {"float32": STEMS * ln * 8, "pcm24": STEMS * ln * 6, "pcm16": STEMS * ln * 4}}
    res.update(_timed(torch, routes, calls, warmup))
    for name in routes:
        if name != "float32":
            res[name]["over_float32"] = res[name]["seconds_median"] / res["float32"]["seconds_median"]
    # the conversion kernels' device time, one timed call per route
    res["kernels"] = {}
    for name, call in routes.items():
        eng.set_timing(True)
        call()
        tim, kern = eng.get_timing(), dict(eng.get_timing_kernels())
        eng.set_timing(False)
        for key in sorted(set(k for k, _ in tim if k.startswith("pcm"))):
            ms = [v for k, v in tim if k == key]
            res["kernels"]["%s/%s" % (name, key)] = {"kernel": kern.get(key, ""), "launches": len(ms), "ms_total": sum(ms), "ms_median_per_launch": statistics.median(ms), "ms_max": max(ms)}
    # what makes the dither free end to end: its pack of a full chunk against the download of that chunk's 16-bit frames at the float route's measured rate
    rate = res["bytes_down"]["float32"] / res["float32"]["seconds_median"]
    take = min(chunk, ln)
    pack = res["kernels"]["pcm16_dither_out/pcm16_pack_dither"]
    res["dither_pack_vs_download"] = {"download_bytes_per_second_float_route": rate, "chunk_frames": take, "chunk_download_ms_16bit": 1e3 * STEMS * take * 4 / rate,
                                      "dither_pack_ms_per_chunk_max": pack["ms_max"], "plain_pack_ms_per_chunk_max": res["kernels"]["pcm16_out/pcm16_pack"]["ms_max"],
                                      "pack_below_download": pack["ms_max"] < 1e3 * STEMS * take * 4 / rate}
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", default="10,60")
    ap.add_argument("--max-tiles", type=int, default=64)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: its separate_host_stream is alternated with this tree's float32 route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm24_bench.json"))
    ap.add_argument("--case", default="", help="(internal) <minutes>")
    ap.add_argument("--float-case", default="", help="(internal) <minutes>,<package root>")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(child(float(a.case), a.max_tiles, a.calls, a.warmup)))
        return
    if a.float_case:
        minutes, root = a.float_case.split(",", 1)
        print(json.dumps(child_float(root, float(minutes), a.max_tiles, a.calls, a.warmup)))
        return

    def run(args):
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args + ["--max-tiles", str(a.max_tiles), "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("%s failed:\n%s\n%s" % (args, r.stdout[-2000:], r.stderr[-4000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])
    res = {"config": "%d stems, %dx%d tiles, chunks of %d tiles, fp32, noise, page-locked buffers; wall clock, median of %d timed rounds after %d warm-up, every route once "
                     "per round, one process per stream; kernel times: device events of one timed call" % (STEMS, T, F, a.max_tiles, a.calls, a.warmup),
           "streams": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for m in a.minutes.split(","):
        entry = run(["--case", m])
        if a.parent_root:
            ab = {"this": [], "parent": []}
            for rep in range(3):                                # fresh processes, alternately
                for tag, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
                    ab[tag].append(run(["--float-case", "%s,%s" % (m, root)])["seconds_median"])
            entry["float_route_vs_parent"] = {"seconds_median_per_process": ab, "this_median": statistics.median(ab["this"]), "parent_median": statistics.median(ab["parent"]),
                                              "parent_min": min(ab["parent"]), "parent_max": max(ab["parent"]),
                                              "not_slower_than_parent_max": statistics.median(ab["this"]) <= max(ab["parent"])}
        res["streams"].append(entry)
        print(json.dumps(entry), flush=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")            # (kept as far as it got)


if __name__ == "__main__":
    main()
