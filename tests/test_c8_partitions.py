"""The fp16 mode's C8 layers (csrc/srt_nn5.hip: srt_enc_c8 / srt_dec_c8) at every way a launch can be cut into workgroups, and under graph replay.

A C8 launch is a grid of workgroups, each walking a run of `tpw` consecutive units of one (stem, M block); the count of workgroups is a table value, the
SPLEETERRT_C8_WGS override, or what c8_tuned measured on the layer shape's first launch.  The partition must change nothing in the results, so every check
here is BIT FOR BIT (torch.equal / np.array_equal), never a tolerance:
  - part 0 (no GPU): a host restatement of the launchers' unit / run / grid arithmetic, and the SPLEETERRT_C8_WGS values that put every C8 layer of a
    geometry at its edges (one run per (stem, M block), one unit per run, a last run of one unit, a grid that is not a multiple of 8);
  - part 1: every split (the tuner's candidates, those edge values, the NRW = 2 and resident-weight forms switched off) against the table split, with a
    forward on ANOTHER input in between, so a unit no workgroup writes shows that input's values;
  - part 2: the tuner in a fresh process (empty cache): its first, measuring call, a cached call, the table split and each reported winner;
  - part 3: hipGraph replay of forward / separate against eager runs, one of them under a forced split;
  - part 4: the layout a replayed graph leaves for srtCopyTensor, and the layout switches as part of the graph key.
"""
import contextlib
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENC_CH = ((2, 16), (16, 32), (32, 64), (64, 128), (128, 256), (256, 512))       # csrc/srt_engine.h ENC_CH / DEC_CH
DEC_CH = ((512, 256), (512, 128), (256, 64), (128, 32), (64, 16), (32, 1))
TUNE_CANDIDATES = (512, 768, 1024, 1280, 1536, 2048)                            # c8_tuned's cands[]
EDGES = ("whole", "single", "last1", "grid_odd")
C8_TAPS = ["conv%d" % i for i in range(2, 7)] + ["up%d" % i for i in range(1, 6)]

# part 1 geometries: (T, F, ntiles, stem modes)
GEOMETRIES = {
    "configs4": (256, 1024, 64, (1,) * 5),      # BASELINE configs[4] as bench.py --stems 5 --precision f16 runs it
    "bench4": (256, 1024, 64, (1,) * 4),        # the 4-stem fp16 bench shape
    "f256": (64, 256, 17, (0,)),                # from test_fp16_c8_layers: one-pixel-high deep layers, every tile partial
    "f768": (192, 768, 6, (1, 1, 0)),           # ... tile counts that are not powers of two
}


# ------------------------------------------------------------------ part 0: host restatement of the C8 launch arithmetic
def _cdiv(a, b):
    return (a + b - 1) // b


def down1_c8(T, F, ntiles):
    """srt_down1_c8_ok at its defaults: down1 writes C8 outputs and down2 runs on srt_enc_c8 (the size limits are far above these shapes)"""
    Ho, Wo = T // 2, F // 2
    return F % 4 == 0 and Wo % 64 == 0 and Ho % 8 == 0 and (Wo // 64) * ntiles >= 384


def c8_layers(T, F, ntiles, nstems, nr2=1):
    """every launch of srt_enc_c8 / srt_dec_c8 in one fp16 forward (enc_c8_launch / dec_c8_launch, csrc/srt_nn5.hip): name, kernel, form, units per
    (stem, M block), (stem, M block) pairs, table workgroup count, and whether c8_tuned measures it"""
    out = []
    for i in range(1 if down1_c8(T, F, ntiles) else 2, 6):
        cin, cout = ENC_CH[i]
        Ho, Wo = (T >> i) // 2, (F >> i) // 2
        if Wo > 16:
            form, TH, TW, NI, table = "enc 8x32x1", 8, 32, 1, 768 if cin <= 64 else 1536
        else:
            form, TH, TW, NI, table = "enc 4x16x4", 4, 16, 4, 1536
        out.append(dict(name="down%d" % (i + 1), kernel="srt_enc_c8", form=form, nunits=_cdiv(Wo, TW) * _cdiv(Ho, TH) * _cdiv(ntiles, NI),
                        pairs=(cout // 32) * nstems, table=table, measured=cin >= 64, ni=NI, nsp=_cdiv(Wo, TW) * _cdiv(Ho, TH)))
    for i in range(5):
        cin, cout = DEC_CH[i]
        H, W = T >> (6 - i), F >> (6 - i)
        cs = cout == 16
        if W > 16 and H % 16 == 0 and not cs and (nr2 & 1):
            form, TH, TW, NI, table = "dec 16x32x1 (NRW 2)", 16, 32, 1, 1536
        elif W > 16:
            form, TH, TW, NI, table = "dec 8x32x1", 8, 32, 1, 1280 if cs else 1536
        else:
            form, TH, TW, NI, table = "dec 4x16x4", 4, 16, 4, 1024
        out.append(dict(name="up%d" % (i + 1), kernel="srt_dec_c8", form=form, nunits=_cdiv(W, TW) * _cdiv(H, TH) * _cdiv(ntiles, NI),
                        pairs=(1 if cs else cout // 32) * nstems, table=table, measured=not cs, ni=NI, nsp=_cdiv(W, TW) * _cdiv(H, TH)))
    return out


def c8_split(nunits, pairs, wgs):
    """c8_tpw and the launcher's grid -> (units per run, grid size, units in the last run)"""
    upw = max(wgs // pairs, 1)
    tpw = max(_cdiv(nunits, upw), 1)
    runs = _cdiv(nunits, tpw)
    return tpw, runs * pairs, nunits - (runs - 1) * tpw


def edges_hit(layer, wgs):
    tpw, grid, last = c8_split(layer["nunits"], layer["pairs"], wgs)
    hit = set()
    if tpw == layer["nunits"]:
        hit.add("whole")                  # one workgroup per (stem, M block)
    if tpw == 1:
        hit.add("single")                 # one unit per workgroup
    if last == 1 and tpw > 1:
        hit.add("last1")                  # a last run of exactly one unit behind longer runs
    if grid % 8:
        hit.add("grid_odd")               # srt_xcd_order's r != 0 branch
    return hit


def reachable_edges(layer):
    """the edges some workgroup count can reach on this layer (upw = WGS / pairs takes every value >= 1)"""
    got = set()
    for u in range(1, layer["nunits"] + 1):
        got |= edges_hit(layer, u * layer["pairs"])
    return got


def edge_wgs(T, F, ntiles, nstems):
    """a small set of SPLEETERRT_C8_WGS values that together put every C8 layer of the geometry at each edge it can reach (greedy cover; ties go to
    the value nearest the table's 1024, so the runs stay quick)"""
    layers = c8_layers(T, F, ntiles, nstems)
    want = {(L["name"], e) for L in layers for e in reachable_edges(L)}
    cands = {1} | {u * L["pairs"] for L in layers for u in range(1, L["nunits"] + 1)}
    cover = {w: {(L["name"], e) for L in layers for e in edges_hit(L, w)} & want for w in cands}
    chosen = []
    while want:
        w = max(sorted(cands), key=lambda c: (len(cover[c] & want), -abs(math.log(c / 1024.0))))
        chosen.append(w)
        want -= cover[w]
    return sorted(chosen)


def xcd_partition_ok(nunits, pairs, wgs):
    """srt_xcd_order + the kernels' (stem, M block, run) decode over the whole grid: every unit of every (stem, M block) in exactly one run"""
    tpw, grid, _ = c8_split(nunits, pairs, wgs)
    upw = _cdiv(nunits, tpw)
    L = np.arange(grid)
    xcd, j = L & 7, L >> 3
    q, r = grid >> 3, grid & 7
    pos = np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + j
    if not np.array_equal(np.sort(pos), L):
        return False
    wsel, unit0 = pos // upw, (pos % upw) * tpw
    unit1 = np.minimum(unit0 + tpw, nunits)
    count = np.zeros((pairs, nunits), np.int32)
    for w, a, b in zip(wsel, unit0, unit1):
        count[w, a:b] += 1
    return bool((count == 1).all())


def seam_tile(T, F, ntiles, nstems):
    """an interior tile that starts or ends a run in as many C8 layers as possible at the table split (ties: the lowest)"""
    score = {}
    for L in c8_layers(T, F, ntiles, nstems):
        tpw, _, _ = c8_split(L["nunits"], L["pairs"], L["table"])
        for u in range(tpw, L["nunits"], tpw):                  # first unit of every run but the first, and the last unit before it
            for uu in (u - 1, u):
                g = uu // L["nsp"]
                for t in range(g * L["ni"], min((g + 1) * L["ni"], ntiles)):
                    if 0 < t < ntiles - 1:
                        score[t] = score.get(t, 0) + 1
    return min(score, key=lambda t: (-score[t], t)) if score else ntiles // 2


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_edge_workgroup_counts_hit_the_edges(geo):
    """The SPLEETERRT_C8_WGS values part 1 runs really reach every edge of every C8 layer of its geometries, and the restated grids partition the work."""
    T, F, nt, modes = GEOMETRIES[geo]
    S = len(modes)
    layers = c8_layers(T, F, nt, S)
    assert [L["name"] for L in layers][-5:] == ["up1", "up2", "up3", "up4", "up5"]
    vals = edge_wgs(T, F, nt, S)
    assert len(vals) <= 8, vals
    for L in layers:
        reach = reachable_edges(L)
        assert {"whole", "single"} <= reach, (L, reach)        # (a last run of one unit needs nunits = 1 mod some reachable tpw > 1: not every layer has it)
        got = set().union(*(edges_hit(L, w) for w in vals))
        assert got == reach, (geo, L["name"], L["form"], sorted(reach - got), vals)
        for w in sorted(set(vals) | set(TUNE_CANDIDATES) | {L["table"]}):
            assert xcd_partition_ok(L["nunits"], L["pairs"], w), (geo, L["name"], w)
    # every edge kind occurs somewhere in the geometry (a layer whose pairs are a multiple of 8 cannot have an odd grid, but not every layer's are)
    assert set(EDGES) == set().union(*(reachable_edges(L) for L in layers)), geo


def test_restated_forms_cover_every_launcher_form():
    """the geometries exercise every C8 form the product library launches: both encoder forms, the three decoder forms, down2 on srt_enc_c8 and on
    the planar-input kernel"""
    forms, d2 = set(), set()
    for T, F, nt, modes in GEOMETRIES.values():
        layers = c8_layers(T, F, nt, len(modes))
        forms |= {L["form"] for L in layers}
        d2.add(layers[0]["name"] == "down2")
    assert forms == {"enc 8x32x1", "enc 4x16x4", "dec 16x32x1 (NRW 2)", "dec 8x32x1", "dec 4x16x4"}, forms
    assert d2 == {True, False}
    assert "dec 16x32x1 (NRW 2)" not in {L["form"] for L in c8_layers(256, 1024, 64, 5, nr2=0)}


# ------------------------------------------------------------------ GPU helpers
@contextlib.contextmanager
def _env(**kv):
    """environment switches the engine reads per launch / forward, restored on exit (None: unset)"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _mag(oracle, ntiles, T, F, seed):
    x = np.abs(oracle.lcg(seed, ntiles * 2 * T * F, 6.0)).reshape(ntiles, 2, T, F)
    x[:, :, ::7, ::13] *= 8.0
    return np.ascontiguousarray(x, np.float32)


def _layer_kernels(eng, xd):
    eng.set_timing(True)
    eng.forward(xd)
    ks = dict(eng.get_timing_kernels())
    eng.set_timing(False)
    return ks


def _f16_engine(coeffs, T, F, modes, max_tiles):
    import spleeterrt_amd as srt
    eng = srt.Engine(F=F, T=T, stem_modes=modes, variant=srt.VARIANT_VST, max_tiles=max_tiles, precision=srt.PREC_F16)
    for s in range(len(modes)):
        eng.set_coeff(s, coeffs(s))
    return eng


def _taps(eng, picks, names=C8_TAPS):
    return {(n, s, t): eng.tensor(n, s, t) for (s, t) in picks for n in names}


def _assert_taps_equal(got, ref, what):
    for k in ref:
        a, b = got[k], ref[k]
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError("%s: tap %s stem %d tile %d differs in %d values, first at %r: %r vs %r" % (
                what, k[0], k[1], k[2], len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def _assert_same(got, ref, what):
    """torch.equal with a short message (the count and the first differing index, not the tensors)"""
    import torch
    if not torch.equal(got, ref):
        d = (got != ref).nonzero()
        raise AssertionError("%s: %d values differ, first at %r" % (what, d.shape[0], tuple(d[0].tolist()) if d.shape[0] else None))


# ------------------------------------------------------------------ part 1: every split, the same bits
@pytest.mark.gpu
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_every_split_gives_the_same_bits(oracle, coeffs, geo):
    """Masks of every (stem, tile) and the C8 taps of the first / last stem at the first tile, the last tile (a partly empty 4-instance group of the deep
    layers) and a tile at a run seam: identical under every split to the table split, the engine naming the C8 kernels for every restated C8 layer."""
    import torch
    T, F, nt, modes = GEOMETRIES[geo]
    S = len(modes)
    eng = _f16_engine(coeffs, T, F, modes, nt)
    xa = torch.from_numpy(_mag(oracle, nt, T, F, seed=1701 + T)).cuda()
    xb = torch.from_numpy(_mag(oracle, nt, T, F, seed=2903 + F)).cuda()
    picks = [(s, t) for s in sorted({0, S - 1}) for t in sorted({0, nt - 1, seam_tile(T, F, nt, S)})]
    with _env(SPLEETERRT_C8_TUNE=0, SPLEETERRT_C8_WGS=None, SPLEETERRT_C8_NR2=None, SPLEETERRT_C8_WRES=None):
        ks = _layer_kernels(eng, xa)
        for L in c8_layers(T, F, nt, S):
            assert ks[L["name"]].startswith(L["kernel"] + "<"), (L["name"], ks[L["name"]])
        eng.forward(xb)
        ref = eng.forward(xa).clone()
        ref_taps = _taps(eng, picks)
    assert torch.isfinite(ref).all()
    runs = [dict(SPLEETERRT_C8_WGS=w) for w in sorted(set(TUNE_CANDIDATES) | set(edge_wgs(T, F, nt, S)))]
    runs += [dict(SPLEETERRT_C8_TUNE=0, SPLEETERRT_C8_NR2=0), dict(SPLEETERRT_C8_TUNE=0, SPLEETERRT_C8_WRES=0)]
    for kv in runs:
        with _env(**kv):
            eng.forward(xb)                                     # the buffers now hold another input's values
            _assert_same(eng.forward(xa), ref, "%s %r: masks (stem, tile, ch, y, x)" % (geo, kv))
            _assert_taps_equal(_taps(eng, picks), ref_taps, "%s %r" % (geo, kv))
    if geo == "configs4":                                      # the forms switched off really left the NRW = 2 kernel
        with _env(SPLEETERRT_C8_TUNE=0, SPLEETERRT_C8_NR2=0):
            k0 = _layer_kernels(eng, xa)
        assert ks["up3"].startswith("srt_dec_c8<32, 16,") and k0["up3"].startswith("srt_dec_c8<32, 8,"), (ks["up3"], k0["up3"])
    eng.close()
    print("%s: %d splits bit-identical to the table split" % (geo, len(runs)))


# ------------------------------------------------------------------ part 2: the tuner
TUNER_GEO = (128, 512, 9, (1, 0, 1))                          # a shape no other test launches: the child process starts with an empty cache anyway

_TUNER_CHILD = r"""
import hashlib, json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import spleeterrt_amd as srt
from oracle import pyoracle as O
T, F, nt, modes = json.loads(sys.argv[2])
eng = srt.Engine(F=F, T=T, stem_modes=modes, variant=srt.VARIANT_VST, max_tiles=nt, precision=srt.PREC_F16)
for s in range(len(modes)):
    eng.set_coeff(s, O.synth_coeff(s))
def mag(seed):
    x = np.abs(O.lcg(seed, nt * 2 * T * F, 6.0)).reshape(nt, 2, T, F)
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
xa, xb = mag(515), mag(616)
names = ["conv%d" % i for i in range(2, 7)] + ["up%d" % i for i in range(1, 6)]
def digest(m):
    h = hashlib.sha256(m.cpu().numpy().tobytes())
    for s in range(len(modes)):
        for t in range(nt):
            for n in names:
                h.update(eng.tensor(n, s, t).tobytes())
    return h.hexdigest()
out = {"tuning": digest(eng.forward(xa))}
eng.forward(xb)
out["cached"] = digest(eng.forward(xa))
os.environ["SPLEETERRT_C8_TUNE"] = "0"
eng.forward(xb)
out["table"] = digest(eng.forward(xa))
for w in json.loads(sys.argv[3]):
    os.environ["SPLEETERRT_C8_WGS"] = str(w)
    eng.forward(xb)
    out[str(w)] = digest(eng.forward(xa))
eng.close()
print("DIGESTS " + json.dumps(out))
"""


@pytest.mark.gpu
def test_tuner_output_equals_every_fixed_split():
    """c8_tuned in a fresh process (SPLEETERRT_C8_TUNE=2 reports each measured layer): one line per measured layer with a winner from the candidates;
    the measuring call (it returns the last candidate's launch), a cached call, the table split and every candidate give the same digest of the masks
    and of every C8 tap of every instance."""
    T, F, nt, modes = TUNER_GEO
    env = dict(os.environ, SPLEETERRT_C8_TUNE="2")
    for k in ("SPLEETERRT_C8_WGS", "SPLEETERRT_C8_NR2", "SPLEETERRT_C8_WRES", "SPLEETERRT_C8"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _TUNER_CHILD, ROOT, json.dumps([T, F, nt, list(modes)]), json.dumps(list(TUNE_CANDIDATES))],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "child exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = re.findall(r"\[spleeterrt_amd\] C8 (enc|dec) Cin (\d+) Cout (\d+) (\d+)x(\d+) x(\d+) x(\d+): (\d+) workgroups", r.stderr)
    measured = {("enc" if L["kernel"] == "srt_enc_c8" else "dec", L["name"]) for L in c8_layers(T, F, nt, len(modes)) if L["measured"]}
    assert sorted(n for _, n in measured) == ["down4", "down5", "down6", "up1", "up2", "up3", "up4"]
    want = sorted([("enc",) + ENC_CH[int(n[-1]) - 1] for k, n in measured if k == "enc"] + [("dec",) + DEC_CH[int(n[-1]) - 1] for k, n in measured if k == "dec"])
    assert sorted((k, int(ci), int(co)) for k, ci, co, *_ in lines) == want, r.stderr
    winners = set()
    for k, ci, co, h, w, ntl, ns, best in lines:
        assert (int(ntl), int(ns)) == (nt, len(modes)), (ntl, ns)
        assert int(best) in TUNE_CANDIDATES, "layer %s %s/%s: no winner (%s)" % (k, ci, co, best)
        winners.add(int(best))
    dig = json.loads(r.stdout.split("DIGESTS ", 1)[1].strip().splitlines()[0])
    ref = dig["table"]
    assert dig["tuning"] == ref, "the measuring call's output differs from the table split"
    assert dig["cached"] == ref, "a cached call's output differs from the table split"
    for w in TUNE_CANDIDATES:
        assert dig[str(w)] == ref, "SPLEETERRT_C8_WGS=%d differs from the table split (winners %r)" % (w, sorted(winners))
    print("tuner: winners %r; tuning call, cached call and every candidate bit-identical" % sorted(winners))


# ------------------------------------------------------------------ part 3: graph replay in the C8 layout
GRAPH_GEO = (256, 1024, 6, (1, 0, 1))                         # 18 instances: the C8 layers, and a head launch large enough for the masks as halves (srtSeparate)
LAYOUT_GEO = (128, 512, 8, (1, 0, 1))                         # 24 instances: the C8 layers


@pytest.mark.gpu
def test_graph_replay_fp16_c8_equals_eager(oracle, coeffs):
    """forward and separate captured and replayed on a non-default stream (a capture takes the table split, eager calls the tuned one) equal the
    eager runs and an eager run under a forced split; SPLEETERRT_M16 flipped between two graph-mode separates of the same tensors captures anew."""
    import torch
    T, F, nt, modes = GRAPH_GEO
    S = len(modes)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng = _f16_engine(coeffs, T, F, modes, nt)
        xd = torch.from_numpy(_mag(oracle, nt, T, F, seed=4711)).cuda()
        n = (nt * T - 8) * 1024                                  # a signal of nt tiles
        rows = eng.L.srtStftRows(n)
        assert (rows + T - 1) // T == nt
        Lp, Rp = oracle.synth_audio(n, 99, True)
        Ld, Rd = torch.from_numpy(Lp).cuda(), torch.from_numpy(Rp).cuda()
        ks = _layer_kernels(eng, xd)
        assert ks["down4"].startswith("srt_enc_c8<") and ks["up2"].startswith("srt_dec_c8<"), ks
        m_e = eng.forward(xd).clone()
        s_e = eng.separate(Ld, Rd).clone()
        with _env(SPLEETERRT_C8_WGS=512):                        # no C8 layer's table value at this shape
            assert all(L["table"] != 512 for L in c8_layers(T, F, nt, S))
            m_w = eng.forward(xd).clone()
            s_w = eng.separate(Ld, Rd).clone()
        with _env(SPLEETERRT_M16=0):
            s_f = eng.separate(Ld, Rd).clone()                   # masks kept as floats between the head and the inverse transform
        eng.set_graph_mode(True)
        out = torch.empty_like(m_e)
        eng.forward(xd, out)                                     # captures (table split)
        first = out.clone()
        out.zero_()
        eng.forward(xd, out)                                     # replays
        so = torch.empty_like(s_e)
        eng.separate(Ld, Rd, so)
        sfirst = so.clone()
        so.zero_()
        eng.separate(Ld, Rd, so)
        ssave = so.clone()
        so.zero_()
        with _env(SPLEETERRT_M16=0):                             # the same tensors under another layout switch: a new graph, not the halves one replayed
            eng.separate(Ld, Rd, so)
        sf = so.clone()
        so.zero_()
        eng.separate(Ld, Rd, so)                                 # ... and the switch back replays the first graph
        side.synchronize()
        eng.set_graph_mode(False)
        eng.close()
    _assert_same(m_w, m_e, "forward under a forced split vs the tuned one")
    _assert_same(s_w, s_e, "separate under a forced split vs the tuned one")
    _assert_same(first, m_e, "forward: graph capture vs eager")
    _assert_same(out, m_e, "forward: graph replay vs eager")
    _assert_same(sfirst, s_e, "separate: graph capture vs eager")
    _assert_same(ssave, s_e, "separate: graph replay vs eager")
    same = torch.equal(s_f, s_e)
    assert not same, "SPLEETERRT_M16=0 does not change the output: the check below cannot tell the graphs apart"
    _assert_same(sf, s_f, "separate under SPLEETERRT_M16=0 in graph mode vs eager (the graph captured with halves replayed?)")
    _assert_same(so, s_e, "separate with SPLEETERRT_M16 back on: the first graph's replay vs eager")


# ------------------------------------------------------------------ part 4: the layout a replay leaves for srtCopyTensor
@pytest.mark.gpu
def test_taps_after_replay_follow_the_replayed_layout(oracle, coeffs):
    """srtCopyTensor reads the taps in the layout of the forward that ran last: after a replay, that of the replayed graph, not that of an eager
    forward in between (a C8 graph after an eager planar forward, and a planar graph after an eager C8 forward)."""
    import torch
    T, F, nt, modes = LAYOUT_GEO
    S = len(modes)
    names = ["conv%d" % i for i in range(1, 7)] + ["act%d" % i for i in range(1, 6)] + ["up%d" % i for i in range(1, 7)]
    big_picks = [(0, 0), (S - 1, nt - 1)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng = _f16_engine(coeffs, T, F, modes, nt)
        xb = torch.from_numpy(_mag(oracle, nt, T, F, seed=808)).cuda()
        xs = torch.from_numpy(_mag(oracle, 1, T, F, seed=909)).cuda()
        # eager references: the large batch (C8 layers), one tile (planar)
        ks = _layer_kernels(eng, xb)
        assert ks["up3"].startswith("srt_dec_c8<"), ks["up3"]
        m_big = eng.forward(xb).clone()
        t_big = _taps(eng, big_picks, names)
        m_one = eng.forward(xs).clone()
        t_one = _taps(eng, [(s, 0) for s in range(S)], names)
        eng.set_graph_mode(True)
        ob, os1, scratch = torch.empty_like(m_big), torch.empty_like(m_one), torch.empty_like(m_big)
        # (a) a C8 graph replayed after an eager planar forward
        eng.forward(xb, ob)                                      # capture
        eng.forward_stems(xs, os1, 0, S)                         # eager, one tile: planar
        ob.zero_()
        eng.forward(xb, ob)                                      # replay
        ta = _taps(eng, big_picks, names)
        # (b) a planar graph replayed after an eager C8 forward
        eng.forward(xs, os1)                                     # capture
        eng.forward_stems(xb, scratch, 0, S)                     # eager, large batch: C8
        os1.zero_()
        eng.forward(xs, os1)                                     # replay
        tb = _taps(eng, [(s, 0) for s in range(S)], names)
        side.synchronize()
        eng.set_graph_mode(False)
        eng.close()
    _assert_same(ob, m_big, "C8 graph replay vs eager")
    _assert_same(os1, m_one, "planar graph replay vs eager")
    _assert_taps_equal(ta, t_big, "C8 graph replayed after an eager planar forward")
    _assert_taps_equal(tb, t_one, "planar graph replayed after an eager C8 forward")


SWITCH_GEO = (64, 1024, 48, (1,))                             # the smallest batch on which down1 writes C8 (srt_down1_c8_ok: 8 x 48 column workgroups)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["SPLEETERRT_C8", "SPLEETERRT_C8L1", "SPLEETERRT_D1F16", "SPLEETERRT_D1S2"])
def test_layout_switch_is_part_of_the_graph_key(oracle, coeffs, switch):
    """A layout switch flipped between two graph-mode forwards of the SAME tensors captures a new graph: masks and taps equal an eager forward under
    the switch (not the first graph replayed), and switching back replays the first graph with its own layout.  (On this batch every one of the four
    switches moves down1 off srt_down1_f16_kernel - D1S2=0 through srt_down1_c8_ok - so the masks tell the two graphs apart.)"""
    import torch
    T, F, nt, modes = SWITCH_GEO
    assert down1_c8(T, F, nt)
    names = ["conv%d" % i for i in range(1, 7)] + ["act%d" % i for i in range(1, 6)] + ["up%d" % i for i in range(1, 7)]
    picks = [(0, 0), (0, nt - 1)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng = _f16_engine(coeffs, T, F, modes, nt)
        xd = torch.from_numpy(_mag(oracle, nt, T, F, seed=1234)).cuda()
        ks = _layer_kernels(eng, xd)
        assert ks["down1"].startswith("srt_down1_f16_kernel<") and ks["down2"].startswith("srt_enc_c8<"), (ks["down1"], ks["down2"])
        m_on = eng.forward(xd).clone()
        t_on = _taps(eng, picks, names)
        with _env(**{switch: 0}):
            k_off = _layer_kernels(eng, xd)
            m_off = eng.forward(xd).clone()
            t_off = _taps(eng, picks, names)
        assert not k_off["down1"].startswith("srt_down1_f16_kernel<"), k_off["down1"]
        eng.set_graph_mode(True)
        out = torch.empty_like(m_on)
        eng.forward(xd, out)                                     # capture, switch on
        out.zero_()
        with _env(**{switch: 0}):
            eng.forward(xd, out)                                 # switch off: must capture anew
            g_off = out.clone()
            tg_off = _taps(eng, picks, names)
        out.zero_()
        eng.forward(xd, out)                                     # switch on again: replays the first graph
        side.synchronize()
        tg_on = _taps(eng, picks, names)
        eng.set_graph_mode(False)
        eng.close()
    same = torch.equal(m_off, m_on)
    assert not same, "%s=0 does not change the masks: the checks below cannot tell the graphs apart" % switch
    _assert_same(g_off, m_off, "%s=0 in graph mode vs eager (the graph captured with the switch on replayed?)" % switch)
    _assert_same(out, m_on, "%s back on: the first graph's replay vs eager" % switch)
    _assert_taps_equal(tg_off, t_off, "graph-mode forward with %s=0" % switch)
    _assert_taps_equal(tg_on, t_on, "graph replayed with %s back on" % switch)
