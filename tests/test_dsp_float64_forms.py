"""The derived forms of the inverse transform (csrc/srt_dsp.hip: OV, EXT, MIX, RATIO x those, SEAM / SEAM_BUS, in the three-per-CU family F <= 1024 and the
table family F > 1024) and srt_stft_ov_kernel against float64, in tests/test_dsp_float64.py's norm: every output hop over the hop's own scale, within
MARGIN x e_cpu (+ MARGIN x the window term for F <= 1024), CAP outside.  No kernel is a reference for its sibling here.

The reference is a full-band gain per (output, channel, row, bin) in two versions built from the same fp32 masks (form_gains): g64, the rule in float64 - the
truth the float64 inverse multiplies by - and g32, the same chain stepped in fp32, which the fp32 oracle multiplies by to give e_cpu.
  overlap    srt_overlap.h: j1 = min(r / (T - O), nt - 1), k = r - j1 (T - O); blended when j1 > 0 and k < O: a + w (b - a), a = row k + T - O of tile j1 - 1,
             b = row k of tile j1, w = (k + 1/2) / O.  The fp32 version is tests/test_overlap.py's _blend_rows bit for bit (asserted).
  ratio      after the blend: (m_s^2 + eps / S) / (sum_j m_j^2 + eps), eps = 1e-10; oracle.ratio_mask of the fp32 blend / float64 of the float64 blend
  average    bins >= F of a row and channel take that row's entry of the gain table.  The table is DATA: read back from the device after the call under test and
             used in g32 and g64 alike; the same case holds it to the float64 mean of g64's in-band row within (F / 64 + 6 + 1) 2^-24 (the additions of the
             kernel's longest chain and the division, tests/test_mask_extension.py), which catches a wrong row or channel of the table
  remix      h = G[m][S]; h = fma(G[m][s], g_s, h), s ascending, over the full-band g_s above: tests/test_mix.py's chain32 for g32, the float64 sum for g64;
             the M outputs are the M "stems" of istft_case, and the launcher's G is restated with columns = n_out
  seam       separate_host_overlap adds the three hops after a piece boundary in another association than one pass does: those hops, and no others, get the
             additive term 3 x 2^-24 x (sum of peak_f, f in [s - 3, s]) / scale(s) - three fp32 additions in any order, from the float64 reference alone
             (istft_case, seam_hops); the share of it a case needed is printed

(form, family, regime) -> test.  Every case asserts the kernel it launched by name (get_timing_kernels).
  OV, EXT, OV+EXT, MIX<OV>, MIX<EXT>, MIX<OV,EXT>    ola3 F = 576 / 1024, ola F = 1088; 145 rows, G = 5, O = 1 / 16 / 32, ragged last tile   test_forms_geometry
  OV                                                 ola3 F = 64, ola F = 2048 (band edge inside a thread's bins / the widest band)            test_forms_geometry
  OV+EXT                                             ola3 F = 576, ola F = 1088; 157 rows at O = 16: the last tile's clamp on 13 rows          test_last_tile_clamp
  OV, OV+EXT                                         ola3 F = 1024, ola F = 1088; G = 5, frames 4, 13..17 (one tile) and 65..69 (a tile seam)  test_forms_run_seams
  OV+EXT                                             ola3 F = 1024, ola F = 1088; 1400 frames x 3 stems, G = 13                                test_forms_long_regime
  srt_stft_ov_kernel                                 rows 1025 (fpb 2), 4099 (fpb 6), last workgroup of one frame                              test_forward_overlapped
  RATIO x OV, EXT, OV+EXT; MIX<OV,EXT> with ratio    ola3 F = 576, ola F = 1088; 145 rows, O = 16, through separate()                          test_ratio_forms
  SEAM<ratio, ext> (4), SEAM_BUS<ext> (2)            ola3 F = 576, ola F = 1088; 277 rows, O = 16, three pieces of two tiles                   test_seam_forms
The run-seam case: the engine refuses T < 64, and at T = 64 no overlap (<= 32) puts a tile seam inside 17 frames - a second tile starts only past row 64.  So
frames 4, 13..17 run the OV forms on one tile at O = 32 (nseg mod G takes every value, no blended row), and frames 65..69 at O = 32 add the smallest signals
whose rows 32..63 are blended while runs of five hops cross them (nseg mod 5 takes every value again).

Not in scope: the half-mask (masks16) instantiations - their applied halves are not an input a test can set; the batched and the Wiener-spectrum inverse
kernels - they are tied bit for bit to the single-signal forms, which this file anchors; the live hop kernels.

The CPU tests hold the restated blend to _blend_rows bit for bit, O = 0 and all-ones masks to the old path / gain 1 exactly, and show on perturbed restatements
(w = k / O, the partner row off by one, the partner from tile j1 + 1, the last tile's clamp dropped, the table entry of row r - 1 / of the other channel, ratio
before blend, the matrix columns reversed, a lost seam carry) that each leaves MARGIN x e_cpu by more than two orders of magnitude."""
import functools

import numpy as np
import pytest

import test_dsp_float64 as D
import test_mix as MX
from test_mask_extension import U, _chain
from test_overlap import _blend_rows

EPS = 1e-10
T_S, S3 = 64, 3
ROWS = 2 * T_S + 17                                    # 145: the last tile is ragged at O = 1, 16 and 32
OOB3 = D.OOB[:S3]
MIX2 = MX.NOCANCEL[:2]
BLEND_KEYS = ("weight", "partner_row", "partner_tile", "clamp", "assoc")


# ---------------------------------------------------------------- the gains of a form, fp32 and float64
def tiles(rows, T, O):
    from spleeterrt_amd import stream
    return stream.overlap_tiles(rows, T, O)


def blend(masks, rows, T, O, dtype=np.float64, weight="half", partner_row=0, partner_tile=-1, clamp=True, assoc=False):
    """masks [S][tiles][2][T][F] in the overlapped layout -> per-row gains [S][2][rows][F], every step in dtype.
    weight / partner_row / partner_tile / clamp perturb the rule for the negative controls; assoc blends as a (1 - w) + b w (the same rule, other roundings)."""
    nt, st = masks.shape[1], T - O
    assert nt == tiles(rows, T, O)
    r = np.arange(rows)
    j1 = r // st
    if clamp:
        j1 = np.minimum(j1, nt - 1)
    k = r - j1 * st
    jt = np.minimum(j1, nt - 1)                            # (clamp dropped: row k of the last tile, the wrong row of the right tile)
    m = masks.astype(dtype, copy=False)
    b = m[:, jt, :, k].transpose(1, 2, 0, 3)               # (the two index arrays come first: [rows][S][2][F])
    two = (j1 > 0) & (k < O)
    if not two.any():
        return np.ascontiguousarray(b)
    ja, ka = np.clip(jt + partner_tile, 0, nt - 1), np.clip(k + st + partner_row, 0, T - 1)
    a = m[:, np.where(two, ja, 0), :, np.where(two, ka, 0)].transpose(1, 2, 0, 3)
    w = ({"half": k + 0.5, "k": k + 0.0, "k+1": k + 1.0}[weight].astype(dtype) / dtype(O))[None, None, :, None]
    return np.where(two[None, None, :, None], a * (1 - w) + b * w if assoc else a + w * (b - a), b)


def ratio64(g):
    sq = g ** 2
    return (sq + EPS / g.shape[0]) / (sq.sum(axis=0) + EPS)


def host_table(g32):
    """a stand-in for the device's gain table where no device is (the CPU tests): the fp32 mean of the fp32 in-band gains, [S][rows][2]"""
    return g32.mean(axis=-1, dtype=np.float32).transpose(0, 2, 1)


def lose_carry(masks, T, O, P):
    """what a lost seam carry gives (tests/test_host_overlap.py): rows [T - O, T) of each tile before a piece boundary replaced by rows [0, O) of the next tile"""
    m = masks.copy()
    for j in range(P, m.shape[1], P):
        m[:, j - 1, :, T - O:] = m[:, j, :, :O]
    return m


class Gains:
    """m32 / m64: the in-band gains [outputs][1][2][rows][F] (one "tile" of `rows` rows for istft_case); o32 / o64: per output the gain of bins >= F, a scalar
    or [2][rows]; s64: the stems' float64 in-band gains [S][2][rows][F] before any remix (what the table is a mean of)"""


def form_gains(oracle, masks, rows, T, F, O, oob, ratio=False, table=None, mix=None, ratio_first=False, table_row=0, table_swap=False, mix_reversed=False, **bl):
    assert set(bl) <= set(BLEND_KEYS), bl
    S = masks.shape[0]
    if ratio_first:                                        # (control) normalised per tile, then blended
        g32 = blend(oracle.ratio_mask(masks), rows, T, O, np.float32, **bl)
        g64 = blend(ratio64(masks.astype(np.float64)), rows, T, O, np.float64, **bl)
    else:
        g32, g64 = blend(masks, rows, T, O, np.float32, **bl), blend(masks, rows, T, O, np.float64, **bl)
        if ratio:
            g32, g64 = oracle.ratio_mask(g32), ratio64(g64)
    fg = Gains()
    fg.s64 = g64
    if table is not None:                                  # data, the same in both versions
        tab = np.asarray(table, np.float32)
        assert tab.shape == (S, rows, 2)
        if table_row:
            tab = np.roll(tab, -table_row, axis=1)         # (control) row r takes the entry of row r + table_row
        if table_swap:
            tab = tab[:, :, ::-1]                          # (control) the other channel's entry
        x32 = [np.ascontiguousarray(tab[s].T) for s in range(S)]
    else:
        x32 = [np.float32(oob[s]) for s in range(S)]
    if mix is None:
        fg.m32, fg.m64, fg.o32, fg.o64 = g32[:, None], g64[:, None], x32, x32
        return fg
    G = np.asarray(mix, np.float32)
    if mix_reversed:                                       # (control) stem s takes the gain of stem S - 1 - s
        G = np.concatenate([G[:, S - 1::-1], G[:, S:]], axis=1)
    xs = np.stack([np.broadcast_to(x, (2, rows)) for x in x32]).astype(np.float32)
    g64sum = lambda row, v: float(row[S]) + sum(float(row[s]) * v[s] for s in range(S))          # noqa: E731
    fg.m32 = np.stack([MX.chain32(row, g32) for row in G])[:, None]
    fg.m64 = np.stack([g64sum(row, g64) for row in G])[:, None]
    fg.o32 = [MX.chain32(row, xs) for row in G]
    fg.o64 = [g64sum(row, xs.astype(np.float64)) for row in G]
    return fg


def case_errors(oracle, spec, fg, F, got=None, fg64=None, seam_hops=None):
    """istft_case on the gains of a form (fg64: another form's float64 side, for the controls)"""
    t = fg if fg64 is None else fg64
    return D.istft_case(oracle, spec, fg.m32, fg.o32, spec.shape[1], F, got, t.m64, oob64=t.o64, seam_hops=seam_hops)


def oracle_inverse(oracle, spec, fg, F):
    """the fp32 oracle's inverse under the fp32 gains of a form, [outputs][2][(rows + 3) * 1024]: a stand-in for a device result in the CPU tests"""
    rows, out = spec.shape[1], []
    for c in range(len(fg.o32)):
        g32 = D.gains(fg.m32[c, 0], fg.o32[c], rows, F, np.float32)
        ore, oim = np.zeros((2, rows, D.FFT), np.float32), np.zeros((2, rows, D.FFT), np.float32)
        ore[:, :, :D.HALF], oim[:, :, :D.HALF] = spec[:, :, :D.HALF, 0] * g32, spec[:, :, :D.HALF, 1] * g32
        out.append(oracle.istft(ore, oim))
    return np.stack(out)


def check_table(tag, table, fg, F):
    """the device's table against the float64 mean of the float64 in-band gains, [S][rows][2]"""
    err = float(np.abs(table - fg.s64.mean(axis=-1).transpose(0, 2, 1)).max())
    bound = (_chain(F) + 1) * U
    print("%s | table against the float64 mean of g64: %.3g (bound %.3g)" % (tag, err, bound))
    assert np.isfinite(table).all() and err <= bound, (tag, err, bound)


# ================================================================ CPU
@pytest.mark.parametrize("rows,T,O,F", [(145, 64, 16, 576), (145, 64, 32, 64), (145, 64, 1, 64), (157, 64, 16, 64), (277, 64, 32, 64), (300, 128, 64, 64), (13, 64, 32, 64)])
def test_blend_restated_is_test_overlaps_bit_for_bit(rows, T, O, F):
    m = D.mask_input(S3, tiles(rows, T, O), T, F, 11 + O)
    got, want = blend(m, rows, T, O, np.float32), _blend_rows(m, rows, T, O)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    d = float(np.abs(blend(m, rows, T, O) - want).max())
    assert d <= 3 * U, d                                   # three roundings of values below 1 between the float64 rule and its fp32 steps


def test_zero_overlap_is_the_old_path_and_ones_stay_one(oracle):
    F, rows = 576, 37
    spec = D.spectrum_input(rows, 5)
    masks = D.mask_input(2, 1, T_S, F, 6)
    fg = form_gains(oracle, masks, rows, T_S, F, 0, (1.0, 0.25))
    for s in range(2):
        assert np.array_equal(fg.m32[s, 0], D.mag_rows(masks[s])[:, :rows]) and np.array_equal(fg.m64[s, 0], D.mag_rows(masks[s])[:, :rows].astype(np.float64))
    new, old = case_errors(oracle, spec, fg, F), D.istft_case(oracle, spec, masks, (1.0, 0.25), T_S, F)
    for k in D.HOP_NAMES + D.HOP_CH_NAMES:
        assert new["cpu"][k].v == old["cpu"][k].v > 0 and new["cpu"][k].at == old["cpu"][k].at, k
    # a [2][rows] out-of-band gain that repeats the scalar is the scalar
    arr = D.istft_case(oracle, spec, masks, (np.full((2, rows), 1.0, np.float32), np.full((2, rows), 0.25, np.float32)), T_S, F)
    assert arr["cpu"]["hop max"].v == old["cpu"]["hop max"].v
    ones = np.ones((S3, tiles(ROWS, T_S, 16), 2, T_S, F), np.float32)
    for kw in (dict(), dict(ratio=False, mix=np.array([(0, 1, 0, 0), (0, 0, 0, 1)], np.float32))):
        fg = form_gains(oracle, ones, ROWS, T_S, F, 16, OOB3, table=host_table(blend(ones, ROWS, T_S, 16, np.float32)), **kw)
        for a in (fg.m32, fg.m64) + tuple(fg.o32) + tuple(fg.o64):
            assert np.all(np.asarray(a) == 1.0)


@functools.lru_cache(maxsize=None)
def _control_inputs():
    F, O = 576, 16
    return F, O, D.spectrum_input(ROWS, 21), D.mask_input(S3, tiles(ROWS, T_S, O), T_S, F, 22)


_HONEST = {}


def _honest(oracle, form):
    """the unperturbed gains of a control's form and the oracle's e_cpu under them, computed once"""
    if form not in _HONEST:
        F, O, spec, masks = _control_inputs()
        kw = dict(ratio="ratio" in form, mix=MIX2 if "mix" in form else None)
        if "ext" in form:
            kw["table"] = host_table(blend(masks, ROWS, T_S, O, np.float32))
        fg = form_gains(oracle, masks, ROWS, T_S, F, O, OOB3, **kw)
        _HONEST[form] = (kw, fg, case_errors(oracle, spec, fg, F)["cpu"]["hop max"].v)
    return _HONEST[form]


CONTROLS = [("w = k / O", "ov", dict(weight="k")), ("w = (k + 1) / O", "ov", dict(weight="k+1")), ("partner row off by one", "ov", dict(partner_row=-1)),
            ("partner from tile j1 + 1", "ov", dict(partner_tile=1)), ("last tile's clamp dropped", "ov", dict(clamp=False)),
            ("table entry of row r - 1", "ov+ext", dict(table_row=-1)), ("table entry of the other channel", "ov+ext", dict(table_swap=True)),
            ("ratio before blend", "ratio+ov", dict(ratio_first=True)), ("matrix columns reversed", "mix+ov", dict(mix_reversed=True)),
            ("lost seam carry", "ov", "carry")]


@pytest.mark.parametrize("name,form,perturb", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_the_norm_sees_a_perturbed_form(oracle, name, form, perturb):
    """negative controls: the oracle under the honest fp32 gains against the float64 inverse under a perturbed restatement of the rule"""
    F, O, spec, masks = _control_inputs()
    kw, fg, e_cpu = _honest(oracle, form)
    assert 0 < e_cpu <= D.RESTATE_TOL
    if perturb == "carry":
        bad = form_gains(oracle, lose_carry(masks, T_S, O, 2), ROWS, T_S, F, O, OOB3, **kw)
    else:
        bad = form_gains(oracle, masks, ROWS, T_S, F, O, OOB3, **kw, **perturb)
    w = case_errors(oracle, spec, fg, F, fg64=bad)["cpu"]["hop max"]
    print("%s (%s) | e_cpu %.3g, against the perturbed float64 %.3g at %r: %.0f x MARGIN x e_cpu" % (name, form, e_cpu, w.v, w.at, w.v / (D.MARGIN * e_cpu)))
    assert w.v > 100.0 * D.MARGIN * e_cpu, (name, w.v, e_cpu)


def test_the_bound_passes_another_association(oracle):
    """positive control: a "device" result = the fp32 oracle under gains blended as a (1 - w) + b w - an honest difference of roundings, not of the rule -
    stays inside MARGIN x e_cpu with no term added"""
    F, O, spec, masks = _control_inputs()
    kw, fg, e_cpu = _honest(oracle, "ov")
    alt = form_gains(oracle, masks, ROWS, T_S, F, O, OOB3, assoc=True, **kw)
    assert (alt.m32 != fg.m32).any() and float(np.abs(alt.m32 - fg.m32).max()) <= 4 * U
    w = case_errors(oracle, spec, fg, F, got=oracle_inverse(oracle, spec, alt, F))["gpu"]["hop max"]
    print("a (1 - w) + b w | e_cpu %.3g, the other association %.3g at %r: %.2f x e_cpu" % (e_cpu, w.v, w.at, w.v / e_cpu))
    assert 0 < w.v <= D.MARGIN * e_cpu


def test_the_seam_term_touches_its_hops_only(oracle):
    """istft_case's seam_hops: on a "device" result = the oracle's, the term is listed for the seam hops alone and lies in its derived range; an error put on a
    seam hop is reported less exactly its term, the same error on another hop as it is"""
    F, rows = 576, 60
    spec = D.spectrum_input(rows, 31)
    fg = form_gains(oracle, D.mask_input(1, 1, T_S, F, 32), rows, T_S, F, 0, (0.25,))
    out = oracle_inverse(oracle, spec, fg, F)
    res = case_errors(oracle, spec, fg, F, got=out, seam_hops=(20, 21, 22))
    assert res["gpu"]["hop max"].v <= res["cpu"]["hop max"].v and [h for _, h, _, _ in sorted(res["seam"])] == [20, 21, 22]
    terms = {h: t for _, h, _, t in res["seam"]}
    assert all(3 * U <= t <= 12 * U for t in terms.values()), terms       # 3 x 2^-24 x (one to four frames' peaks over the largest of them)
    for h in (20, 50):
        bump = out.copy().reshape(1, 2, rows + 3, D.HOP)
        bump[0, :, h, 7] += np.float32(1e-3 * np.abs(bump[0, :, h]).max())
        with_term = case_errors(oracle, spec, fg, F, got=bump.reshape(out.shape), seam_hops=(20, 21, 22))
        plain = case_errors(oracle, spec, fg, F, got=bump.reshape(out.shape))
        assert with_term["gpu"]["hop max"].at == plain["gpu"]["hop max"].at == (0, h) and plain["gpu"]["hop max"].v > 1e-5
        assert with_term["gpu"]["hop max"].v == plain["gpu"]["hop max"].v - (terms[20] if h == 20 else 0.0)


# ================================================================ GPU
def _bool(x):
    return "true" if x else "false"


def inverse_kernel(F, ov=False, ext=False, mix=False, ratio=False):
    if mix:
        return MX._mix_kernel(F, ov, ext)
    form = ("_ov" if ov else "") + ("_ext" if ext else "")
    return "srt_istft_ola3%s_kernel<4, %s, false>" % (form, _bool(ratio)) if F <= 1024 else "srt_istft_ola%s_kernel<%s>" % (form, _bool(ratio))


def seam_kernel(F, ext=False, mix=False, ratio=False):
    if mix:
        return "srt_istft_ola3_seam_bus_kernel<4, %s>" % _bool(ext) if F <= 1024 else "srt_istft_ola_seam_bus_kernel<%s>" % _bool(ext)
    return ("srt_istft_ola3_seam_kernel<4, %s, %s>" if F <= 1024 else "srt_istft_ola_seam_kernel<%s, %s>") % (_bool(ratio), _bool(ext))


def hold(oracle, tag, spec, fg, F, got, seam_hops=None, silent=0):
    """every hop of a device result within the bound; prints the figures DESIGN.md 4.1 records"""
    rows, cols = spec.shape[1], len(fg.o32)
    assert got.shape == (cols, 2, (rows + 3) * D.HOP), got.shape
    res = case_errors(oracle, spec, fg, F, got=got, seam_hops=seam_hops)
    G = D.launcher_G(rows, cols, F)
    extra = D.MARGIN * D.ola3_window_delta() if F <= 1024 else 0.0
    tag = "%s F %d frames %d columns %d G %d" % (tag, F, rows, cols, G)
    assert res["silent"] >= silent, tag
    e_cpu, bound = res["cpu"]["hop max"].v, D.MARGIN * res["cpu"]["hop max"].v + extra
    share, raw = 0.0, 0.0
    for s, h, e, term in res["seam"]:
        share, raw = max(share, (e - bound) / term), max(raw, e)
    print("FIGURE %s | E_gpu / e_cpu %.2f%s" % (tag, res["gpu"]["hop max"].v / e_cpu, "" if seam_hops is None else
          " (seam hops less their term) | the %d seam hops before the term %.2f | share of the seam term used %.2f" % (len(res["seam"]), raw / e_cpu, share)))
    D.report(tag, res, ("hop max",), extra=extra, period=G)
    D.check_cap(tag, res)
    return res


def _engine(F, S=S3, max_tiles=5, oob=OOB3, **kw):
    import spleeterrt_amd as srt
    return srt.Engine(F=F, T=T_S, stem_modes=MX.MODES[:S], oob_weights=oob, variant=srt.VARIANT_VST, max_tiles=max_tiles, **kw)


def _table(eng, rows):
    return np.stack([eng.mask_ext(s, rows) for s in range(eng.S)])


def run_form(oracle, tag, eng, spec, masks, F, O, ext=False, mix=None, oob=OOB3):
    """srtIstft of one form on an arbitrary spectrum: the kernel by name, the table, every hop"""
    import torch
    rows = spec.shape[1]
    eng.set_overlap(O)
    eng.set_mask_extension("average" if ext else "constant")
    eng.set_mix(mix)
    sd, md = torch.from_numpy(spec).cuda(), torch.from_numpy(masks).cuda()
    got, ks = MX._timed(eng, lambda: eng.istft(sd, md).cpu().numpy())
    assert ks == ([("mask_ext", "srt_mask_ext_kernel<false, false, %s>" % _bool(O > 0))] if ext else []) + [("istft", inverse_kernel(F, O > 0, ext, mix is not None))], ks
    table = _table(eng, rows) if ext else None
    fg = form_gains(oracle, masks, rows, T_S, F, O, oob, table=table, mix=mix)
    tag = "%s O %d" % (tag, O)
    if ext:
        check_table(tag, table, fg, F)
    return hold(oracle, tag, spec, fg, F, got, silent=2 if rows >= D.ZERO_ROW + 6 else 0)


FORMS = {"OV": dict(ov=True), "EXT": dict(ext=True), "OV+EXT": dict(ov=True, ext=True),
         "MIX<OV>": dict(ov=True, mix=MIX2), "MIX<EXT>": dict(ext=True, mix=MIX2), "MIX<OV,EXT>": dict(ov=True, ext=True, mix=MIX2)}
GEOMETRY = [(F, form) for F in (576, 1024, 1088) for form in FORMS] + [(64, "OV"), (2048, "OV")]


@pytest.mark.gpu
@pytest.mark.parametrize("F,form", GEOMETRY, ids=["%d-%s" % c for c in GEOMETRY])
def test_forms_geometry(oracle, F, form):
    """145 rows x 3 stems under distinct masks: O = 1 (one blended row, w = 1/2), 16, 32; the last tile ragged at each; at O = 16 row 144 and at O = 32 rows
    128..144 lie past the last tile's start (the clamp)"""
    kw = dict(FORMS[form])
    ov = kw.pop("ov", False)
    spec = D.spectrum_input(ROWS, 1100 + F)
    eng = _engine(F)
    for O in ((1, 16, 32) if ov else (0,)):
        nt = tiles(ROWS, T_S, O)
        assert (nt - 1) * (T_S - O) + T_S > ROWS                                     # ragged
        run_form(oracle, form, eng, spec, D.mask_input(S3, nt, T_S, F, 1200 + F + O), F, O, **kw)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [576, 1088])
def test_last_tile_clamp(oracle, F):
    """157 rows at O = 16: three tiles, and rows 144..156 have r / (T - O) = 3 >= nt - they live at rows 48..60 of the last tile"""
    rows, O = 157, 16
    nt = tiles(rows, T_S, O)
    assert nt == 3 and (rows - 1) // (T_S - O) >= nt and sum(1 for r in range(rows) if r // (T_S - O) >= nt) == 13
    eng = _engine(F)
    run_form(oracle, "clamp OV+EXT", eng, D.spectrum_input(rows, 1300 + F), D.mask_input(S3, nt, T_S, F, 1400 + F), F, O, ext=True)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ext", [False, True], ids=["OV", "OV+EXT"])
@pytest.mark.parametrize("F", [1024, 1088])
def test_forms_run_seams(oracle, F, ext):
    """G = 5, one stem, T = 64 (the smallest the engine takes), O = 32: frames 4, 13..17 on one tile, frames 65..69 with rows 32..63 blended (module docstring)"""
    O = 32
    eng = _engine(F, S=1, max_tiles=2, oob=(0.25,))
    for frames in (4, 13, 14, 15, 16, 17, 65, 66, 67, 68, 69):
        nt = tiles(frames, T_S, O)
        assert nt == (1 if frames <= T_S else 2) and D.launcher_G(frames, 1, F) == 5
        run_form(oracle, "seams", eng, D.spectrum_input(frames, 1500 + frames), D.mask_input(1, nt, T_S, F, 1600 + frames), F, O, ext=ext, oob=(0.25,))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1024, 1088])
def test_forms_long_regime(oracle, F):
    """1400 frames x 3 stems at O = 16, OV+EXT: G = 13 in both families, and 48 mod 13 = 9 walks every phase of a tile seam inside a run"""
    frames, O = 1400, 16
    nt = tiles(frames, T_S, O)
    assert D.launcher_G(frames, S3, F) == 13 and (frames + 3) * S3 >= 4096 and nt == 29
    eng = _engine(F, max_tiles=nt)
    run_form(oracle, "long OV+EXT", eng, D.spectrum_input(frames, 1700 + F), D.mask_input(S3, nt, T_S, F, 1800 + F), F, O, ext=True)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1025, 4099])
def test_forward_overlapped(oracle, rows):
    """srt_stft_ov_kernel at fpb = 2 and 6 (a last workgroup of one frame), T = 64, O = 16, F = 1024: the spectrum is srt_stft_kernel's bit for bit (held to float64
    at these rows by test_dsp_float64.py::test_stft_regimes), and every magnitude tile is rows [j (T - O), j (T - O) + T) of the O = 0 magnitudes, zeros past the end"""
    import torch
    F, O = 1024, 16
    st, nt = T_S - O, tiles(rows, T_S, O)
    assert D.launcher_fpb(rows) == (2 if rows == 1025 else 6) and rows % D.launcher_fpb(rows) == 1
    L, R = D.signal_rows("staircase", rows)
    Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    eng = _engine(F, S=1, max_tiles=nt, oob=(1.0,))
    (spec0, mag0), ks0 = MX._timed(eng, lambda: eng.stft(Ld, Rd))
    assert ks0 == [("stft", "srt_stft_kernel")], ks0
    eng.set_overlap(O)
    (spec, mag), ks = MX._timed(eng, lambda: eng.stft(Ld, Rd))
    assert ks == [("stft", "srt_stft_ov_kernel")], ks
    assert spec.shape[1] == rows and mag.shape == (nt, 2, T_S, F) and torch.equal(spec, spec0)
    rows0 = mag0.permute(1, 0, 2, 3).reshape(2, -1, F)                                # [2][tiles * T][F]: row r of the signal at index r
    assert bool((rows0[:, rows:] == 0).all()) and int((rows0.amax(dim=(0, 2)) > 0).sum()) >= rows - 10     # (all but the silent frames and the rows past the tail frame)
    flat = torch.zeros((2, (nt - 1) * st + T_S, F), device="cuda")
    flat[:, :rows] = rows0[:, :rows]
    want = flat.unfold(1, T_S, st).permute(1, 0, 3, 2)                               # [nt][2][T][F]: tile j = rows [j st, j st + T)
    bad = torch.nonzero((mag != want).any(dim=3).any(dim=1))
    assert bad.numel() == 0, "rows %d: %d (tile, row) pairs differ, first %r" % (rows, bad.shape[0], tuple(bad[0].tolist()))
    eng.close()


RATIO_FORMS = {"RATIO+OV": dict(ov=True), "RATIO+EXT": dict(ext=True), "RATIO+OV+EXT": dict(ov=True, ext=True), "RATIO+MIX<OV,EXT>": dict(ov=True, ext=True, mix=MIX2)}


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(RATIO_FORMS))
@pytest.mark.parametrize("F", [576, 1088])
def test_ratio_forms(oracle, coeffs, F, form):
    """separate() on a ratio_mask engine (batch_invariant, synthetic weights, the staircased signal): the raw masks of stft -> forward are data, and the output
    is held to the float64 inverse of the engine's own spectrum under blend -> ratio -> table -> remix in float64.  (The project claims separate() bit-equal
    to its stages for none of these forms - srtIstft never normalises, and a caller-side srtRatioMask would come before the blend - so there is no chain to
    compare bits with, as test_ratio_in_the_prologue has for the plain form: separate() itself is the device result.)"""
    import torch
    kw = dict(RATIO_FORMS[form])
    O, ext, mix = 16 if kw.get("ov") else 0, kw.get("ext", False), kw.get("mix")
    L, R = D.signal_rows("staircase", ROWS)
    Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    eng = _engine(F, ratio_mask=True, batch_invariant=True)
    for s in range(S3):
        eng.set_coeff(s, coeffs(s))
    eng.set_overlap(O)
    eng.set_mask_extension("average" if ext else "constant")
    eng.set_mix(mix)
    got, ks = MX._timed(eng, lambda: eng.separate(Ld, Rd).cpu().numpy())
    assert ks[-1] == ("istft", inverse_kernel(F, O > 0, ext, mix is not None, ratio=True)), ks[-1]
    if ext:
        assert ks[-2] == ("mask_ext", "srt_mask_ext_kernel<false, true, %s>" % _bool(O > 0)), ks[-2]
    table = _table(eng, ROWS) if ext else None
    spec, mag = eng.stft(Ld, Rd)
    assert mag.shape[0] == tiles(ROWS, T_S, O)
    raw = eng.forward(mag).cpu().numpy()
    eng.close()
    fg = form_gains(oracle, raw, ROWS, T_S, F, O, OOB3, ratio=True, table=table, mix=mix)
    if ext:
        check_table(form, table, fg, F)
    hold(oracle, form, spec.cpu().numpy(), fg, F, got)


SEAM_FORMS = {"SEAM": dict(), "SEAM<ratio>": dict(ratio=True), "SEAM<ext>": dict(ext=True), "SEAM<ratio,ext>": dict(ratio=True, ext=True),
              "SEAM_BUS": dict(mix=MIX2), "SEAM_BUS<ext>": dict(mix=MIX2, ext=True)}
SEAM_ROWS = 277


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(SEAM_FORMS))
@pytest.mark.parametrize("F", [576, 1088])
def test_seam_forms(oracle, coeffs, F, form):
    """separate_host_overlap in three pieces of two tiles (277 rows, O = 16) against the float64 inverse of the whole signal: spectrum, raw masks in the
    overlapped layout and the gain table come from an engine that holds the signal (data; every row's gain is the same bits under batch_invariant)"""
    import torch
    from spleeterrt_amd import capi
    kw = SEAM_FORMS[form]
    O, ratio, ext, mix = 16, kw.get("ratio", False), kw.get("ext", False), kw.get("mix")
    L, R = D.signal_rows("staircase", SEAM_ROWS)
    Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    pieces = capi.host_overlap_pieces(SEAM_ROWS, T_S, O, 2)
    assert len(pieces) == 3 and tiles(SEAM_ROWS, T_S, O) == 6
    engines = []
    for max_tiles in (6, 2):
        eng = _engine(F, max_tiles=max_tiles, ratio_mask=ratio, batch_invariant=True)
        for s in range(S3):
            eng.set_coeff(s, coeffs(s))
        eng.set_mask_extension("average" if ext else "constant")
        eng.set_mix(mix)
        engines.append(eng)
    whole, small = engines
    whole.set_overlap(O)
    table = None
    if ext:
        whole.separate(Ld, Rd)
        table = _table(whole, SEAM_ROWS)
    spec, mag = whole.stft(Ld, Rd)
    raw = whole.forward(mag).cpu().numpy()
    spec = spec.cpu().numpy()
    whole.close()
    out = np.full((small.outputs, 2, (SEAM_ROWS + 3) * D.HOP), np.nan, np.float32)
    (got, clipped), ks = MX._timed(small, lambda: small.separate_host_overlap((L, R), O, out=out))
    small.release_staging()
    small.close()
    inv = [k for name, k in ks if name == "istft"]
    assert inv == [inverse_kernel(F, True, ext, mix is not None, ratio)] + [seam_kernel(F, ext, mix is not None, ratio)] * 2, inv
    assert not np.isnan(got).any() and not clipped.any()
    fg = form_gains(oracle, raw, SEAM_ROWS, T_S, F, O, OOB3, ratio=ratio, table=table, mix=mix)
    if ext:
        check_table(form, table, fg, F)
    hold(oracle, form, spec, fg, F, got, seam_hops=tuple(p["row0"] + i for p in pieces[1:] for i in range(3)))
