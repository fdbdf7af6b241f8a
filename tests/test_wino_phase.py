"""Barrier phase offset of the fp32 Winograd decoder kernels (csrc/srt_nn4.hip, PH of srt_dec_wino32 and srt_dec_wino; switch SPLEETERRT_WINO_PH).

With the offset, waves 4-7 of a workgroup meet the K step's barrier in front of a later quad instead of the first, over rings of five; which MFMAs feed an
accumulator, and in which order, does not change.  So the layer outputs must be BIT-IDENTICAL to the arrangement without the offset (SPLEETERRT_WINO_PH=0):
any difference is a slab or a patch read before it landed, or overwritten while a wave still read it.

5 tiles x 4 stems (20 instances: above the 16-instance switch to the Winograd form), T = 256 so that up1 runs its two-instance form with a half-empty last pair,
F = 1024 and F = 1536 (up2 8 x 48: a half-empty last tile column).  srtSeparate on seeded noise (every tile distinct) with the seeded weights of the oracle;
up1..up5 of every instance (srtCopyTensor) and the whole output are compared through SHA-256 digests of their bytes.

Each arrangement runs in a process of its own under its own time limit, one after the other: a fault or a hang of the first ends the job, the second is not started.

What this test can and cannot see: a slab or patch read too early, or overwritten too early, shows here only if the race fires at these 20 instances.  The guard of the
ring and vmcnt arithmetic itself are the kernels' static_asserts (UR >= D + 2, the early-piece counts tied to the piece maps); this test holds that the arrangement the
switch selects really is another instantiation of each layer's kernel and that, as run, it computes the same bits.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, TILES, STEMS = 256, 5, 4
FS = (1024, 1536)
LAYERS = ("up1", "up2", "up3", "up4", "up5")
RUN_LIMIT_S = 150           # per process: interpreter + torch start-up, two engines, two srtSeparate calls (seconds each), 200 tensor copies


def _worker(out_path):
    """both geometries under the SPLEETERRT_WINO_PH of the environment -> JSON {F: {"kernels": {layer: symbol}, "digests": {name: sha256}}}"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import spleeterrt_amd as srt
    from oracle import pyoracle
    res = {}
    for F in FS:
        eng = srt.Engine(F=F, T=T, stem_modes=(1, 0, 1, 0), variant=srt.VARIANT_VST, max_tiles=TILES, impl=srt.IMPL_MFMA)
        for s in range(STEMS):
            eng.set_coeff(s, pyoracle.synth_coeff(s))
        n = (TILES * T - 40) * 1024                                      # 5 tiles, the last one partly past the end of the signal
        L, R = pyoracle.synth_audio(n, seed=1000 + F)
        Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        assert eng.tiles(eng.L.srtStftRows(n)) == TILES
        out = eng.separate(Ld, Rd).cpu().numpy()
        assert np.isfinite(out).all()
        dig = {"out": hashlib.sha256(out.tobytes()).hexdigest()}
        for name in LAYERS:
            for s in range(STEMS):
                for t in range(TILES):
                    dig["%s/%d/%d" % (name, s, t)] = hashlib.sha256(eng.tensor(name, s, t).tobytes()).hexdigest()
        _, mag = eng.stft(Ld, Rd)
        eng.set_timing(True)
        eng.forward(mag)
        ks = dict(eng.get_timing_kernels())
        eng.set_timing(False)
        res[str(F)] = {"kernels": {k: ks[k] for k in LAYERS}, "digests": dig}
        eng.close()
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{switch value: the worker's record}: "0" first, then "-1" (every layer group phased), each under its own time limit"""
    d = tmp_path_factory.mktemp("wino_phase")
    got = {}
    for val in ("0", "-1"):
        path = str(d / ("ph_%s.json" % val.replace("-", "m")))
        env = dict(os.environ, SPLEETERRT_WINO_PH=val)
        p = subprocess.run(["timeout", "-k", "10", str(RUN_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker", path],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:                                            # chained: nothing more is started on the GPU after a fault or a time limit
            pytest.fail("SPLEETERRT_WINO_PH=%s: exit status %d\n%s" % (val, p.returncode, p.stdout[-4000:]), pytrace=False)
        got[val] = json.load(open(path))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("F", FS)
def test_phase_offset_is_bit_identical(runs, F):
    off, on = runs["0"][str(F)], runs["-1"][str(F)]
    for name in ("up1", "up2", "up3", "up4"):                           # the switch must select another instantiation of the same kernel
        assert off["kernels"][name].startswith("srt_dec_wino32<") and on["kernels"][name].startswith("srt_dec_wino32<"), (off["kernels"], on["kernels"])
        assert off["kernels"][name] != on["kernels"][name], (name, on["kernels"][name])
    assert off["kernels"]["up5"].startswith("srt_dec_wino<") and on["kernels"]["up5"].startswith("srt_dec_wino<"), (off["kernels"], on["kernels"])
    assert off["kernels"]["up5"] != on["kernels"]["up5"], on["kernels"]["up5"]
    assert set(off["digests"]) == set(on["digests"]) and len(on["digests"]) == 1 + len(LAYERS) * STEMS * TILES
    bad = sorted(k for k in on["digests"] if on["digests"][k] != off["digests"][k])
    print("F = %d: %d digests, %d differ" % (F, len(on["digests"]), len(bad)))
    assert not bad, "F = %d: not bit-identical with the phase offset: %s" % (F, bad[:12])


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    _worker(sys.argv[2])
