"""Measure srtSeparateBatchMix (the stem remix per track of a packed batch).

    python scripts/batch_mix_bench.py [--steps 20] [--warmup 3] [--out profiles/batch_mix_bench.json]

Bench shape and clips of scripts/batch_overlap_bench.py: F = 1024, T = 256, max_tiles = 64; 4 stems fp32 and the 5-stem fp16 mode; 32 clips x 10 s, 64 packed
tiles at O = 0 and at O = 64.  Device events, the median (with min and max) of `steps` calls after `warmup` calls.  Per mode and overlap, in one process:
  mix1 / mix2   ONE srtSeparateBatchMix call writing one karaoke output (input minus stem 0) / two outputs (stem 0 and the karaoke bus) per track
  loop          the path a caller had before: 32 srtSeparate calls after srtSetMix (and srtSetOverlap), same matrices
  all_stems     the other one: srtSeparateBatch[Overlap] writing every stem at the same packed tiles (the sum is still to be formed by the caller)
and the istft_batch launch of each batch call on its own.  Nothing is asserted; the expectation of §16 (one output's inverse launch no slower than the
all-stem launch at equal rows; two may be) is recorded as a flag.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import batch_overlap_bench as OB  # noqa: E402

T, F, TILES, CLIPS = OB.T, OB.F, OB.TILES, OB.CLIPS


def matrices(S):
    import numpy as np
    kar = np.zeros((1, S + 1), np.float32)
    kar[0, 0], kar[0, S] = -1.0, 1.0
    voc = np.zeros((1, S + 1), np.float32)
    voc[0, 0] = 1.0
    return kar, np.concatenate([voc, kar])


def section(prec, steps, warmup):
    import torch
    from spleeterrt_amd import stream
    dev = torch.device("cuda", 0)
    eng, S = OB.engine(prec, dev)
    tr = OB.clips(dev)
    ns = [L.numel() for L, _ in tr]
    stems = OB.outputs(eng, S, tr, dev)
    g1, g2 = matrices(S)
    res = []
    for O in (0, OB.O_BENCH):
        g = stream.pack_tracks(ns, T, TILES, overlap=O)
        assert len(g) == 1 and g[0].ntiles == TILES
        rec = {"precision": prec, "stems": S, "T": T, "F": F, "max_tiles": TILES, "overlap": O, "tracks": CLIPS, "rows_per_track": stream.stft_rows(OB.CLIP_SAMPLES),
               "packed_tiles": TILES, "steps": steps, "warmup": warmup}
        rec["all_stems_batch"] = OB.timed(lambda: eng.separate_batch(tr, stems, overlap=O), steps, warmup)
        rec["all_stems_istft_batch_ms"] = OB.per_launch(eng, lambda: eng.separate_batch(tr, stems, overlap=O), steps)["istft_batch"]
        for tag, G in (("mix1", g1), ("mix2", g2)):
            outs = OB.outputs(eng, G.shape[0], tr, dev)
            call = lambda: eng.separate_batch(tr, outs, overlap=O, mix=G)      # noqa: E731
            rec[tag + "_batch"] = OB.timed(call, steps, warmup)
            rec[tag + "_istft_batch_ms"] = OB.per_launch(eng, call, steps)["istft_batch"]
            eng.set_timing(True)
            call()
            rec[tag + "_kernel"] = eng.get_timing_kernels()[-1][1]
            eng.set_timing(False)

            def loop():
                for (L, R), o in zip(tr, outs):
                    eng.separate(L, R, o)
            eng.set_overlap(O)
            eng.set_mix(G)
            rec[tag + "_loop_32_srtSeparate_srtSetMix"] = OB.timed(loop, steps, warmup)
            eng.set_mix(None)
            eng.set_overlap(0)
            rec[tag + "_speedup_over_loop"] = round(rec[tag + "_loop_32_srtSeparate_srtSetMix"]["ms_median"] / rec[tag + "_batch"]["ms_median"], 3)
            rec[tag + "_over_all_stems_batch"] = round(rec[tag + "_batch"]["ms_median"] / rec["all_stems_batch"]["ms_median"], 4)
        rec["expectation_mix1_istft_no_slower_than_all_stems"] = rec["mix1_istft_batch_ms"] <= rec["all_stems_istft_batch_ms"]
        print(json.dumps(rec), flush=True)
        res.append(rec)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_mix_bench.json"))
    a = ap.parse_args()
    res = section("f32", a.steps, a.warmup) + section("f16", a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
