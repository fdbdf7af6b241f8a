"""Time srtResample (csrc/srt_resample.hip) on 60 minutes of stereo fp32 resident in HBM, with device events, after warm-up.

    python scripts/resample_bench.py [--minutes 60] [--steps 10] [--warmup 3] [--out profiles/resample_bench.json]

Per rate pair: ms per call (median and min of `steps` event-timed calls), algorithmic bytes (input read once + output written once)
over time in GB/s, that rate as a fraction of the 8 TB/s HBM peak (and of the 6.29 TB/s a float4 copy reaches), and taps x frames
(the FMA count / 2 channels).  Prints one JSON line per pair and writes them all to --out.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM = 8.0e12
COPY_HBM = 6.29e12
PAIRS = [(48000, 44100), (96000, 44100), (44100, 48000)]


def taps_per_frame(fs_in, fs_out, table_len=22438, index_inc=491):
    """window length of the kernel (src_sinc.c taps of both halves, padded to a multiple of 4)"""
    r = fs_out / float(fs_in)
    inc = int(round(index_inc * min(r, 1.0) * 4096))
    t = 2 * (((table_len - 2) << 12) // inc) + 2
    return (t + 3) // 4 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    import torch
    import spleeterrt_amd as srt
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: no GPU (the converter has no CPU path)")
    rows = []
    for fs_in, fs_out in PAIRS:
        n = int(a.minutes * 60 * fs_in)
        g = torch.Generator(device="cuda").manual_seed(fs_in)
        x = torch.randn((2, n), device="cuda", generator=g) * 0.25
        rs = srt.Resampler(fs_in, fs_out)
        m = rs.length(n)
        Lo = torch.empty(m, device="cuda")
        Ro = torch.empty(m, device="cuda")
        for _ in range(a.warmup):
            rs.resample(x[0], x[1], Lo=Lo, Ro=Ro)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rs.resample(x[0], x[1], Lo=Lo, Ro=Ro)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        med = ms[len(ms) // 2]
        nbytes = 8 * n + 8 * m
        taps = taps_per_frame(fs_in, fs_out)
        row = {"fs_in": fs_in, "fs_out": fs_out, "minutes": a.minutes, "frames_in": n, "frames_out": m, "ms_median": round(med, 4),
               "ms_min": round(ms[0], 4), "gb_per_s": round(nbytes / (med * 1e-3) / 1e9, 1), "hbm_peak_frac": round(nbytes / (med * 1e-3) / PEAK_HBM, 4),
               "hbm_copy_frac": round(nbytes / (med * 1e-3) / COPY_HBM, 4), "algorithmic_bytes": nbytes, "taps_per_frame": taps,
               "taps_x_frames": taps * m, "fma_per_s": round(2 * taps * m / (med * 1e-3), 1), "steps": a.steps, "warmup": a.warmup}
        print(json.dumps(row), flush=True)
        rows.append(row)
        rs.close()
        del x, Lo, Ro
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": rows}, f, indent=1)


if __name__ == "__main__":
    main()
