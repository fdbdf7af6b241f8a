#!/usr/bin/env python3
"""The Wiener filter on overlapped tiles over a host stream (srtSeparateHostWienerOverlap), measured by the method of scripts/host_wiener_bench.py at
the bench shape (4 stems, 256 x 1024 tiles, pieces of 64 tiles, page-locked host buffers, fp32, the stream of scripts/stream_c4.py):

  a 10-minute and a 60-minute stream: separate_host_wiener_overlap at O = 0 and O = 64 with 1 and 2 iterations, beside separate_host_wiener of the same stream (its
  code is unchanged; O = 0 issues the same launches) and beside separate_host_stream / separate_host_overlap(O = 64) without the filter.

    python scripts/host_wiener_overlap_bench.py           # all cases -> profiles/host_wiener_overlap_bench.json

Every stream runs in a fresh process (this script started with --case): engine, page-locked buffers and the stream are set up once, then each call gets its warm-up
calls and its timed calls (wall clock); the median, the minimum and the maximum are reported.  No threshold: the file records what was measured.  The derived
expectation beside each overlapped figure: the network's share grows by T / (T - O) (that many more tiles), and O / (max_tiles * (T - O)) of the analysis - upload,
unpack, transform - is done twice.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
from host_wiener_bench import F, FS, HOP, STEMS, T, _engine, _timed      # noqa: E402


def child_stream(minutes, max_tiles, overlap, calls, warmup):
    import torch
    import stream_c4
    from spleeterrt_amd import stream
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
    S = T - overlap
    res = {"minutes": minutes, "rows": rows, "overlap": overlap, "max_tiles_per_piece": max_tiles, "calls": calls, "warmup": warmup,
           "tiles": {"O0": stream.overlap_tiles(rows, T, 0), "O%d" % overlap: stream.overlap_tiles(rows, T, overlap)},
           "pieces": {"O0": len(stream.host_overlap_pieces(rows, T, 0, max_tiles)), "O%d" % overlap: len(stream.host_overlap_pieces(rows, T, overlap, max_tiles))},
           "store_bytes": {"O0": eng.host_wiener_overlap_bytes(n, 0), "O%d" % overlap: eng.host_wiener_overlap_bytes(n, overlap)},
           "expected": {"network_share_factor": T / S, "analysis_done_twice": overlap / (max_tiles * S)},
           "bytes_h2d": n * 8, "bytes_d2h": STEMS * 2 * (rows * HOP + 3072) * 4}
    ov = "O%d" % overlap
    cases = [("host_stream_no_filter", lambda: eng.separate_host_stream(Lp, Rp, out=out, pinned=True)),
             ("host_overlap_%s_no_filter" % ov, lambda: eng.separate_host_overlap((Lp, Rp), overlap, out=out, pinned=True))]
    for it in (1, 2):
        cases += [("host_wiener_%d" % it, lambda it=it: eng.separate_host_wiener((Lp, Rp), it, out=out, pinned=True)),
                  ("host_wiener_overlap_O0_%d" % it, lambda it=it: eng.separate_host_wiener_overlap((Lp, Rp), 0, it, out=out, pinned=True)),
                  ("host_wiener_overlap_%s_%d" % (ov, it), lambda it=it: eng.separate_host_wiener_overlap((Lp, Rp), overlap, it, out=out, pinned=True))]
    for name, call in cases:
        r = _timed(call, calls, warmup)
        r["x_realtime_pcie_inclusive"] = rows * HOP / FS / r["seconds_median"]
        res[name] = r
    med = lambda k: res[k]["seconds_median"]                                 # noqa: E731
    res["host_overlap_%s_no_filter" % ov]["over_O0"] = med("host_overlap_%s_no_filter" % ov) / med("host_stream_no_filter")
    for it in (1, 2):
        res["host_wiener_overlap_O0_%d" % it]["over_host_wiener"] = med("host_wiener_overlap_O0_%d" % it) / med("host_wiener_%d" % it)
        r = res["host_wiener_overlap_%s_%d" % (ov, it)]
        r["over_host_wiener"] = r["seconds_median"] / med("host_wiener_%d" % it)
        r["over_overlap_no_filter"] = r["seconds_median"] / med("host_overlap_%s_no_filter" % ov)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", default="10,60")
    ap.add_argument("--max-tiles", type=int, default=64)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_wiener_overlap_bench.json"))
    ap.add_argument("--case", default="", help="(internal) stream,<minutes>")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(child_stream(float(a.case.split(",")[1]), a.max_tiles, a.overlap, a.calls, a.warmup)))
        return
    common = ["--max-tiles", str(a.max_tiles), "--overlap", str(a.overlap), "--calls", str(a.calls), "--warmup", str(a.warmup)]
    res = {"config": "%d stems, %dx%d tiles, pieces of %d tiles, O = 0 and O = %d, fp32, page-locked host buffers, the stream of scripts/stream_c4.py; wall clock, median "
                     "of the timed calls after the warm-up calls, one fresh process per stream" % (STEMS, T, F, a.max_tiles, a.overlap), "stream": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for m in a.minutes.split(","):
        r = spawn(common + ["--case", "stream,%s" % m])
        res["stream"].append(r)
        print(json.dumps(r), flush=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")            # (kept as far as it got)


def spawn(args):
    """host_wiener_bench.spawn starts its own file: this one's child is this file"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("case %s failed:\n%s\n%s" % (args, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    main()
