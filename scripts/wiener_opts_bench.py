"""Time the Wiener filter's per-call options (srtSeparateWiener) with device events, after warm-up.

    python scripts/wiener_opts_bench.py [--steps 20] [--warmup 3] [--parent-root DIR] [--out profiles/wiener_opts_bench.json]

Shapes: the bench shape (64 tiles of 256 x 1024, 4 stems, fp32) and BASELINE configs[4] (the same batch, 5 stems, fp16 conv), one iteration.  Every case runs
in a fresh process (--worker) and reports ms per call (median, min, max of `steps` event-timed calls) and the per-launch ms of one more, timed call:
  (i)   separate under set_wiener(1), on this tree and - with --parent-root, a built checkout of the parent commit - on the parent, alternating;
  (ii)  separate_wiener with every option off (the same launches as (i));
  (iii) overlap 64 on the 12 352-row signal (exactly 64 overlapped tiles) against overlap 0 on the same signal;
  (iv)  the average mask extension on;
  (v)   one karaoke output (n_out = 1) against every stem (ii).
Prints one JSON line per run and writes them all to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, F, TILES = 256, 1024, 64
CASES = {          # name: (rows, keyword arguments of separate_wiener; None: separate under set_wiener)
    "i_separate_set_wiener": (TILES * T, None),
    "ii_defaults": (TILES * T, {}),
    "iii_overlap0_12352": (12352, {}),
    "iii_overlap64_12352": (12352, {"overlap": 64}),
    "iv_average": (TILES * T, {"mask_extension": "average"}),
    "v_karaoke": (TILES * T, {"mix": "karaoke"}),
}


def worker(a):
    sys.path.insert(0, a.root)
    import torch
    import spleeterrt_amd as srt
    from bench import synth_weights
    stems, rows, kw = a.stems, CASES[a.case][0], CASES[a.case][1]
    dev = torch.device("cuda", 0)
    eng = srt.Engine(F=F, T=T, stem_modes=(1, 0, 1, 1, 0)[:stems], oob_weights=(0.25, 0.0, 0.25, 0.25, 0.25)[:stems], variant=srt.VARIANT_VST,
                     max_tiles=TILES, device=dev, precision=a.precision)
    for s in range(stems):
        eng.set_coeff(s, synth_weights(s, dev))
    n = rows * 1024
    g = torch.Generator(device=dev).manual_seed(777)
    L = (torch.rand(n, device=dev, generator=g) - 0.5) * 0.2
    R = 0.5 * L + (torch.rand(n, device=dev, generator=g) - 0.5) * 0.1
    if kw is None:
        eng.set_wiener(1)
        planes, call = stems, lambda: eng.separate(L, R, out)
    else:
        kw = dict(kw)
        if kw.get("mix") == "karaoke":
            kw["mix"] = [[0.0, -1.0] + [0.0] * (stems - 2) + [1.0]]           # everything minus stem 1 (the vocals)
        planes, call = (1 if "mix" in kw else stems), lambda: eng.separate_wiener(L, R, 1, out=out, **kw)
    out = torch.empty((planes, 2, eng.L.srtIstftLength(rows)), device=dev)
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    for x, y in ev:
        x.record()
        call()
        y.record()
    torch.cuda.synchronize()
    ms = [x.elapsed_time(y) for x, y in ev]
    eng.set_timing(True)
    call()
    tim = eng.get_timing()
    eng.set_timing(False)
    per = {}
    for name, t in tim:
        per[name] = per.get(name, 0.0) + t
    print(json.dumps({"case": a.case, "tree": a.tree, "stems": stems, "precision": {0: "f32", 1: "f16"}[a.precision], "rows": rows, "outputs": planes,
                      "steps": a.steps, "warmup": a.warmup, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                      "launches": len(tim), "per_launch_ms": {k: round(v, 4) for k, v in per.items()}}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: case (i) also runs there, alternating with this tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wiener_opts_bench.json"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--case")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--tree", default="this")
    ap.add_argument("--stems", type=int, default=4)
    ap.add_argument("--precision", type=int, default=0)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = []

    def run(case, stems, precision, root=ROOT, tree="this"):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--case", case, "--root", root, "--tree", tree, "--stems", str(stems), "--precision", str(precision),
               "--steps", str(a.steps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if p.returncode:                         # a failed worker ends the run: nothing more is started on the device
            sys.exit("worker %s failed (%d):\n%s" % (case, p.returncode, p.stderr[-2000:]))
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        res.append(json.loads(line))

    for stems, precision in ((4, 0), (5, 1)):
        for _ in range(2):
            if a.parent_root:
                run("i_separate_set_wiener", stems, precision, os.path.abspath(a.parent_root), "parent")
            run("i_separate_set_wiener", stems, precision)
        for case in ("ii_defaults", "iii_overlap0_12352", "iii_overlap64_12352", "iv_average", "v_karaoke"):
            run(case, stems, precision)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
