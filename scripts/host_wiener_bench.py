#!/usr/bin/env python3
"""The Wiener filter over a host stream (srtSeparateHostWiener), measured at the bench shape (4 stems, 256 x 1024 tiles, pieces of 64 tiles,
page-locked host buffers, fp32):

  stream   a 10-minute and a 60-minute stream (the BASELINE configs[3] signal of scripts/stream_c4.py): separate_host_wiener at 1 and 2 iterations beside
           separate_host_stream of the same stream without the filter;
  fits     a 64-tile signal (one piece): separate_host_wiener beside separate_wiener on device-resident PCM (no PCIe, no store).

    python scripts/host_wiener_bench.py                   # all cases -> profiles/host_wiener_bench.json

Every case runs in a fresh process (this script started with --case): engine, page-locked buffers and the stream are set up once, then each call gets its warm-up
calls and its timed calls; the median, the minimum and the maximum are reported.  No threshold: the file records what was measured.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, T, STEMS, HOP, FS = 1024, 256, 4, 1024, 44100.0


def _engine(dev, max_tiles):
    import spleeterrt_amd as srt
    from bench import synth_weights
    eng = srt.Engine(F=F, T=T, stem_modes=(1,) * STEMS, oob_weights=(0.25, 0.0, 0.25, 0.25), variant=srt.VARIANT_VST, max_tiles=max_tiles, device=dev)
    for s in range(STEMS):
        eng.set_coeff(s, synth_weights(s, dev))
    return eng


def _timed(call, calls, warmup):
    import torch
    for _ in range(warmup):
        call()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"seconds_median": statistics.median(times), "seconds_min": min(times), "seconds_max": max(times), "seconds": times}


def child_stream(minutes, max_tiles, calls, warmup):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    sys.path.insert(0, ROOT)
    import torch
    import stream_c4
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_audio = int(round(minutes * 60 * FS))
    n = 4096 * ((n_audio + 4095) // 4096) + 8192
    rows = (n + HOP - 1) // HOP
    eng = _engine(dev, max_tiles)
    Lp = torch.zeros(n, dtype=torch.float32, pin_memory=True)
    Rp = torch.zeros(n, dtype=torch.float32, pin_memory=True)
    stream_c4.synth_stream(n_audio, 0, n_audio, out=(Lp.numpy()[:n_audio], Rp.numpy()[:n_audio]))
    out = torch.empty((STEMS, 2, rows * HOP + 3072), dtype=torch.float32, pin_memory=True)
    res = {"minutes": minutes, "rows": rows, "pieces": (rows + max_tiles * T - 1) // (max_tiles * T), "max_tiles_per_piece": max_tiles, "calls": calls, "warmup": warmup,
           "store_bytes": eng.host_wiener_bytes(n), "bytes_h2d": n * 8, "bytes_d2h": STEMS * 2 * (rows * HOP + 3072) * 4}
    cases = (("host_stream_no_filter", lambda: eng.separate_host_stream(Lp, Rp, out=out, pinned=True)),
             ("host_wiener_1", lambda: eng.separate_host_wiener((Lp, Rp), 1, out=out, pinned=True)),
             ("host_wiener_2", lambda: eng.separate_host_wiener((Lp, Rp), 2, out=out, pinned=True)))
    for name, call in cases:
        r = _timed(call, calls, warmup)
        r["x_realtime_pcie_inclusive"] = rows * HOP / FS / r["seconds_median"]
        res[name] = r
    for it in (1, 2):
        res["host_wiener_%d" % it]["over_no_filter"] = res["host_wiener_%d" % it]["seconds_median"] / res["host_stream_no_filter"]["seconds_median"]
    eng.close()
    return res


def child_fits(max_tiles, calls, warmup):
    """one piece: the host call (PCIe and the store included) beside separate_wiener on PCM that is already on the device"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    sys.path.insert(0, ROOT)
    import torch
    import stream_c4
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = max_tiles * T
    n = rows * HOP
    eng = _engine(dev, max_tiles)
    Lp = torch.zeros(n, dtype=torch.float32, pin_memory=True)
    Rp = torch.zeros(n, dtype=torch.float32, pin_memory=True)
    stream_c4.synth_stream(n, 0, n, out=(Lp.numpy(), Rp.numpy()))
    Ld, Rd = Lp.to(dev), Rp.to(dev)
    out_h = torch.empty((STEMS, 2, rows * HOP + 3072), dtype=torch.float32, pin_memory=True)
    out_d = torch.empty((STEMS, 2, rows * HOP + 3072), dtype=torch.float32, device=dev)
    res = {"rows": rows, "tiles": max_tiles, "calls": calls, "warmup": warmup, "store_bytes": eng.host_wiener_bytes(n)}
    for it in (1, 2):
        res["separate_wiener_device_%d" % it] = _timed(lambda: eng.separate_wiener(Ld, Rd, it, out=out_d), calls, warmup)
        res["host_wiener_%d" % it] = _timed(lambda: eng.separate_host_wiener((Lp, Rp), it, out=out_h, pinned=True), calls, warmup)
        res["host_wiener_%d" % it]["over_device_resident"] = res["host_wiener_%d" % it]["seconds_median"] / res["separate_wiener_device_%d" % it]["seconds_median"]
    eng.close()
    return res


def spawn(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("case %s failed:\n%s\n%s" % (args, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", default="10,60")
    ap.add_argument("--max-tiles", type=int, default=64)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_wiener_bench.json"))
    ap.add_argument("--case", default="", help="(internal) stream,<minutes> | fits")
    a = ap.parse_args()
    if a.case == "fits":
        print(json.dumps(child_fits(a.max_tiles, max(a.calls, 5), a.warmup)))
        return
    if a.case:
        print(json.dumps(child_stream(float(a.case.split(",")[1]), a.max_tiles, a.calls, a.warmup)))
        return
    common = ["--max-tiles", str(a.max_tiles), "--calls", str(a.calls), "--warmup", str(a.warmup)]
    res = {"config": "%d stems, %dx%d tiles, pieces of %d tiles, fp32, page-locked host buffers, the stream of scripts/stream_c4.py; median of the timed calls after "
                     "the warm-up calls, one fresh process per case" % (STEMS, T, F, a.max_tiles), "stream": []}
    res["fits"] = spawn(common + ["--case", "fits"])
    print(json.dumps(res["fits"]), flush=True)
    for m in a.minutes.split(","):
        r = spawn(common + ["--case", "stream,%s" % m])
        res["stream"].append(r)
        print(json.dumps(r), flush=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")            # (kept as far as it got)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
