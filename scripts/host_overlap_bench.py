#!/usr/bin/env python3
"""Overlapped tiles over a host stream (srtSeparateHostStreamOverlap), measured at the bench shape (4 stems, 256 x 1024 tiles, pieces of 64 tiles,
page-locked host buffers, fp32, wall clock) on a 10-minute and a 60-minute stream (the BASELINE configs[3] signal of scripts/stream_c4.py):

  (a) default path   separate_host_overlap at overlap 0 on this tree against separate_host_stream on the parent commit (--parent-root: a built checkout of it),
                     alternately in fresh processes; this tree's median must lie inside the parent's min..max (the launches are the same) - recorded as
                     "inside_parent_range", with both trees' numbers;
  (b) cost           overlap 32 / 64 / 128 beside overlap 0 in one process.  Expected from the code: the network's T / (T - O); recorded without a bound;
  (c) the carry      the srt_mask_seam_save_kernel launches of one overlap-64 call (srtGetTiming device events): count, total and largest.

    python scripts/host_overlap_bench.py --parent-root ../parent        # -> profiles/host_overlap_bench.json

Every case runs in a fresh process (this script started with --case): engine, page-locked buffers and the stream are set up once, then each call gets its warm-up
calls and its timed calls (median of 3 after 1 by default).  Without --parent-root part (a) records this tree alone and says so.
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
OVERLAPS = (32, 64, 128)


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


def child(root, what, minutes, max_tiles, calls, warmup):
    """what = "default": the O = 0 call of the tree at `root` (separate_host_overlap where the tree has it, else separate_host_stream); "cost": (b) and (c)"""
    sys.path.insert(0, os.path.join(root, "scripts"))
    sys.path.insert(0, root)
    import torch
    import spleeterrt_amd as srt
    import stream_c4
    from bench import synth_weights
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_audio = int(round(minutes * 60 * FS))
    n = 4096 * ((n_audio + 4095) // 4096) + 8192
    rows = (n + HOP - 1) // HOP
    eng = srt.Engine(F=F, T=T, stem_modes=(1,) * STEMS, oob_weights=(0.25, 0.0, 0.25, 0.25), variant=srt.VARIANT_VST, max_tiles=max_tiles, device=dev)
    for s in range(STEMS):
        eng.set_coeff(s, synth_weights(s, dev))
    Lp = torch.zeros(n, dtype=torch.float32, pin_memory=True)
    Rp = torch.zeros(n, dtype=torch.float32, pin_memory=True)
    stream_c4.synth_stream(n_audio, 0, n_audio, out=(Lp.numpy()[:n_audio], Rp.numpy()[:n_audio]))
    out = torch.empty((STEMS, 2, rows * HOP + 3072), dtype=torch.float32, pin_memory=True)
    has = hasattr(eng, "separate_host_overlap")
    res = {"tree": "this tree" if os.path.abspath(root) == ROOT else "parent", "minutes": minutes, "rows": rows, "max_tiles_per_piece": max_tiles, "calls": calls, "warmup": warmup}
    if what == "default":
        res["call"] = "separate_host_overlap(overlap=0)" if has else "separate_host_stream"
        call = (lambda: eng.separate_host_overlap((Lp, Rp), 0, out=out, pinned=True)) if has else (lambda: eng.separate_host_stream(Lp, Rp, out=out, pinned=True))
        res.update(_timed(call, calls, warmup))
    else:
        from spleeterrt_amd import stream
        for O in (0,) + OVERLAPS:
            r = _timed(lambda: eng.separate_host_overlap((Lp, Rp), O, out=out, pinned=True), calls, warmup)
            r["pieces"] = len(stream.host_overlap_pieces(rows, T, O, max_tiles))
            r["tiles"] = stream.overlap_tiles(rows, T, O)
            r["network_growth_expected"] = T / (T - O)
            r["x_realtime_pcie_inclusive"] = rows * HOP / FS / r["seconds_median"]
            res["overlap_%d" % O] = r
        for O in OVERLAPS:
            res["overlap_%d" % O]["over_overlap_0"] = res["overlap_%d" % O]["seconds_median"] / res["overlap_0"]["seconds_median"]
        eng.set_timing(True)
        eng.separate_host_overlap((Lp, Rp), 64, out=out, pinned=True)
        tim = eng.get_timing()
        eng.set_timing(False)
        saves = [ms for name, ms in tim if name == "mask_seam"]
        res["mask_seam_save_overlap_64"] = {"launches": len(saves), "ms_total": sum(saves), "ms_max": max(saves) if saves else 0.0,
                                            "ms_all_launches_of_the_call": sum(ms for _, ms in tim), "bytes_per_launch": STEMS * 2 * 64 * F * 4 * 2}
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
    ap.add_argument("--rounds", type=int, default=3, help="fresh processes per tree in part (a)")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_overlap_bench.json"))
    ap.add_argument("--case", default="", help="(internal) <root>,<default|cost>,<minutes>")
    a = ap.parse_args()
    if a.case:
        root, what, minutes = a.case.rsplit(",", 2)
        print(json.dumps(child(root, what, float(minutes), a.max_tiles, a.calls, a.warmup)))
        return
    common = ["--max-tiles", str(a.max_tiles), "--calls", str(a.calls), "--warmup", str(a.warmup)]
    res = {"config": "%d stems, %dx%d tiles, pieces of %d tiles, fp32, page-locked host buffers, the stream of scripts/stream_c4.py; wall clock, median of the timed "
                     "calls after the warm-up calls, one fresh process per case" % (STEMS, T, F, a.max_tiles), "streams": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for m in a.minutes.split(","):
        entry = {"minutes": float(m), "default_path": {"this_tree": [], "parent": []}}
        for _ in range(a.rounds):
            if a.parent_root:
                entry["default_path"]["parent"].append(spawn(common + ["--case", "%s,default,%s" % (os.path.abspath(a.parent_root), m)]))
            entry["default_path"]["this_tree"].append(spawn(common + ["--case", "%s,default,%s" % (ROOT, m)]))
        d = entry["default_path"]
        d["this_tree_median"] = statistics.median(r["seconds_median"] for r in d["this_tree"])
        if d["parent"]:
            d["parent_min"] = min(r["seconds_min"] for r in d["parent"])
            d["parent_max"] = max(r["seconds_max"] for r in d["parent"])
            d["inside_parent_range"] = d["parent_min"] <= d["this_tree_median"] <= d["parent_max"]
        else:
            d["note"] = "no --parent-root: the parent commit was not measured"
        entry["cost"] = spawn(common + ["--case", "%s,cost,%s" % (ROOT, m)])
        res["streams"].append(entry)
        print(json.dumps(entry), flush=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")            # (kept as far as it got)


if __name__ == "__main__":
    main()
