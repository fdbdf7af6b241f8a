"""All-class form of the fp32 Winograd decoder kernel (csrc/srt_nn4.hip, AC of srt_dec_wino32; switch SPLEETERRT_WINO_AC).

With the switch's bit 1 set, up2..up4 run workgroups of four waves in which ONE wave owns all four parity classes of its 16 blocks and both M blocks (98
accumulator tiles, one wave per SIMD) and computes the 16 distinct transform values of a block once, where the class-split form computes 49 in four waves.
Which MFMAs feed an accumulator, and in which channel order, does not change, and the output transform and epilogue are the same functions: the layer outputs
must be BIT-IDENTICAL to the class-split form (SPLEETERRT_WINO_AC=0).  Any difference is a slab or a patch read before it landed or overwritten while a wave
still read it, a wrong place in the slab, or - the MFMAs of this form are issued from inline assembly - a result read before the matrix pipeline delivered it.

GPU part: 5 tiles x 4 stems (20 instances: above the 16-instance switch to the Winograd form), T = 256, F = 1024 and F = 1536 (up2 8 x 48: a half-empty last
tile column), the last tile partly past the end of the signal; seeded weights of the oracle, stem modes (1, 0, 1, 0).  up1..up5 of every instance
(srtCopyTensor) and the whole output go through SHA-256.  One process per setting (0, then -1), each under its own time limit, chained: nothing is started on
the GPU after a non-zero exit.  The layer groups this form is built for are listed in BUILT; up1 and up5 keep their kernels under either setting.

CPU part: the compiler's resource report of the new instantiation (scripts/kernel_resources.py) must show occupancy 1 and no scratch: 392 accumulator
registers leave about 120 for everything else, and a kernel that spills is not this kernel.
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, TILES, STEMS = 256, 5, 4
FS = (1024, 1536)
LAYERS = ("up1", "up2", "up3", "up4", "up5")
BUILT = ("up2", "up3", "up4")          # the layer groups the all-class form exists for (bit 1 of the switch)
RUN_LIMIT_S = 150                     # per process: interpreter + torch start-up, two engines, two srtSeparate calls (seconds each), 200 tensor copies
# what the class-split tree reports for these launches (SPLEETERRT_WINO_PH at its default): SPLEETERRT_WINO_AC=0 must launch exactly these
HEAD_KERNELS = {
    "up1": "srt_dec_wino32<2, 8, 0, 5, 3, 1, 1, 0, 1, 1, 2, 0, 1, 1",
    "up2": "srt_dec_wino32<2, 16, 0, 5, 3, 1, 1, 0, 1, 1, 1, 0, 1, 1",
    "up3": "srt_dec_wino32<2, 16, 0, 5, 3, 1, 1, 0, 1, 1, 1, 0, 1, 1",
    "up4": "srt_dec_wino32<2, 16, 0, 5, 3, 1, 1, 0, 1, 1, 1, 0, 1, 1",
    "up5": "srt_dec_wino<4, 16, 1, 0, 5, 0, 0, 1, 3, 2>",
}


def _worker(out_path):
    """both geometries under the SPLEETERRT_WINO_AC of the environment -> JSON {F: {"kernels": {layer: symbol}, "digests": {name: sha256}}}"""
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
    """{switch value: the worker's record}: "0" first, then "-1" (every layer group the form is built for), each under its own time limit"""
    d = tmp_path_factory.mktemp("wino_allclass")
    got = {}
    for val in ("0", "-1"):
        path = str(d / ("ac_%s.json" % val.replace("-", "m")))
        env = dict(os.environ, SPLEETERRT_WINO_AC=val)
        env.pop("SPLEETERRT_WINO_PH", None)                              # the form is taken only where the group's phase bit is set: its default
        p = subprocess.run(["timeout", "-k", "10", str(RUN_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker", path],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:                                            # chained: nothing more is started on the GPU after a fault or a time limit
            pytest.fail("SPLEETERRT_WINO_AC=%s: exit status %d\n%s" % (val, p.returncode, p.stdout[-4000:]), pytrace=False)
        got[val] = json.load(open(path))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("F", FS)
def test_all_class_form_is_bit_identical(runs, F):
    off, on = runs["0"][str(F)], runs["-1"][str(F)]
    print("F = %d kernels, switch 0: %s" % (F, off["kernels"]))
    print("F = %d kernels, switch -1: %s" % (F, on["kernels"]))
    for name in LAYERS:                                                  # switch 0: exactly the class-split launches
        k = off["kernels"][name]
        assert k == HEAD_KERNELS[name] or k.startswith(HEAD_KERNELS[name] + ","), (name, k)
    for name in BUILT:                                                   # the switch selects another instantiation of the same kernel
        assert on["kernels"][name].startswith("srt_dec_wino32<4, 16, "), (name, on["kernels"][name])
        assert on["kernels"][name] != off["kernels"][name], (name, on["kernels"][name])
    for name in set(LAYERS) - set(BUILT):
        assert on["kernels"][name] == off["kernels"][name], (name, on["kernels"][name])
    assert set(off["digests"]) == set(on["digests"]) and len(on["digests"]) == 1 + len(LAYERS) * STEMS * TILES
    bad = sorted(k for k in on["digests"] if on["digests"][k] != off["digests"][k])
    print("F = %d: %d digests, %d differ" % (F, len(on["digests"]), len(bad)))
    assert not bad, "F = %d: not bit-identical in the all-class form: %s" % (F, bad[:12])


def test_all_class_kernel_resources():
    """occupancy 1, no scratch, no spilled vector register, and the LDS of four rings"""
    src = os.path.join(ROOT, "spleeterrt_amd", "csrc", "srt_nn4.hip")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), src, "-fno-slp-vectorize"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [l for l in p.stdout.splitlines() if re.match(r"srt_dec_wino32<4, 16, .*, 1>\s", l)]
    print("\n".join(rows))
    assert len(rows) == 1, p.stdout[-4000:]
    m = re.search(r"scratch\s+(\d+) occ (\d+) lds\s+(\d+) spill v(\d+)", rows[0])
    assert m, rows[0]
    scratch, occ, lds, vspill = (int(x) for x in m.groups())
    assert (scratch, occ, vspill) == (0, 1, 0), rows[0]
    assert lds <= 160 * 1024, rows[0]
    committed = open(os.path.join(ROOT, "profiles", "wino_allclass_kernel_resources.txt")).read().splitlines()
    assert rows[0].split("vgpr")[0].strip() in [l.split("vgpr")[0].strip() for l in committed], "profiles/wino_allclass_kernel_resources.txt does not list " + rows[0]


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    _worker(sys.argv[2])
