"""The Wiener filter with per-call options (srtIstftWienerEx / srtSeparateWiener): overlapped tiles, the average mask extension and the stem
remix under the filter, for a single signal.  `wiener_opts_np` restates the definitions in float64 on top of test_wiener.wiener_np; the CPU tests check the
restatement and the binding's argument checks, the GPU tests hold the two new kernels and the entry points to it.

Shapes: 277 rows (N_RAGGED), T = 64, S = 3, F in {512, 1536}, O in {16, 32}: six and eight overlapped tiles with a ragged last one, O = 32 = T / 2 blends every
row of every tile but the first, 18 statistics chunks of 16 rows straddle the 48- and 32-row strides, and F = 1536 takes the inverse transform's other family."""
import ctypes as C
import re

import numpy as np
import pytest

from test_overlap import N_RAGGED, _audio, _blend_rows, _engine, _pack_rows
from test_wiener import _compare, _istft_of, _mask_rows, _rand_spec, _spec_tensor, _stereo_clip, _to_complex, wiener_np

T_S, S_S = 64, 3
OOB = (0.0, 1.0, 0.25)          # visibly wrong wherever the average rule should have replaced them
KARAOKE = np.array([[-1.0, 0.0, 0.0, 1.0]], np.float32)


def wiener_opts_np(spec, masks, T, F, iters, oob, overlap=0, average=False, mix=None):
    """float64 restatement.  masks [S, tiles, 2, T, F] in the layout of `overlap`.  The filter is wiener_np on the blended per-row masks; above F stem j is
    oob[j] s or, average, e_j(r, c) s with e_j the mean over the band of the blended mask row; a mix is G[:, :S] applied to the stems' spectra plus G[:, S] s.
    Returns (spectra [n_out or S, 2, rows, 2049], covs, e [S, 2, rows])."""
    rows = spec.shape[1]
    m = _blend_rows(masks, rows, T, overlap) if overlap else np.ascontiguousarray(_mask_rows(masks, rows))
    out, covs = wiener_np(spec, _pack_rows(m, T), T, F, iters, oob)
    e = m.astype(np.float64).mean(axis=-1)
    if average:
        out[..., F:] = e[..., None] * spec[None, :, :, F:2049]
    if mix is not None:
        G = np.asarray(mix, np.float64)
        S = out.shape[0]
        out = np.einsum("ms,scrk->mcrk", G[:, :S], out) + G[:, S][:, None, None, None] * spec[None, :, :, :2049]
    return out, covs, e


def _overlapped_from_rows(m, T, O):
    """per-row masks [S, 2, rows, F] -> the overlapped layout whose tiles AGREE on the rows they share (rows past the signal: zero)"""
    from spleeterrt_amd import stream
    S, _, rows, F = m.shape
    nt, st = stream.overlap_tiles(rows, T, O), T - O
    p = np.zeros((S, nt, 2, T, F), np.float32)
    for j in range(nt):
        hi = min(j * st + T, rows)
        p[:, j, :, :hi - j * st] = m[:, :, j * st:hi]
    return p


# ------------------------------------------------------------------------------------------------------------------------------ CPU: the restatement
def _small(seed, S=3, T=16, F=64, rows=40):
    rng = np.random.default_rng(seed)
    return rng, S, T, F, rows, _rand_spec(rng, rows)


def test_restatement_agreeing_tiles_give_the_back_to_back_result():
    rng, S, T, F, rows, spec = _small(1)
    m = rng.random((S, 2, rows, F)).astype(np.float32)
    ref, _, _ = wiener_opts_np(spec, _pack_rows(m, T), T, F, 2, OOB)
    for O in (4, 8):
        out, _, _ = wiener_opts_np(spec, _overlapped_from_rows(m, T, O), T, F, 2, OOB, overlap=O)
        assert np.array_equal(out, ref), O


def test_restatement_mix_rows():
    from spleeterrt_amd import stream
    rng, S, T, F, rows, spec = _small(2)
    O = 4
    masks = rng.random((S, stream.overlap_tiles(rows, T, O), 2, T, F)).astype(np.float32)
    for average in (False, True):
        stems, _, _ = wiener_opts_np(spec, masks, T, F, 1, OOB, overlap=O, average=average)
        hot, _, _ = wiener_opts_np(spec, masks, T, F, 1, OOB, overlap=O, average=average, mix=np.eye(S, S + 1))
        assert np.array_equal(hot, stems)
        total, _, _ = wiener_opts_np(spec, masks, T, F, 1, OOB, overlap=O, average=average, mix=[[1.0] * S + [0.0]])
        assert np.allclose(total[0], stems.sum(0), rtol=0, atol=1e-15)


def test_restatement_average_of_equal_masks_is_that_value():
    rng, S, T, F, rows, spec = _small(3)
    c = 0.375
    out, _, e = wiener_opts_np(spec, np.full((S, 3, 2, T, F), c, np.float32), T, F, 1, OOB, average=True)
    assert np.array_equal(e, np.full((S, 2, rows), c))
    for j in range(S):
        assert np.array_equal(out[j][..., F:], c * spec[:, :, F:2049])


class _Stub:
    """stands in for an Engine: any library call is a failure of the test"""
    S, T = 3, 64

    def __getattr__(self, name):
        raise AssertionError("the argument checks must raise before %r is touched" % name)


@pytest.mark.parametrize("kw,match", [
    (dict(mix=np.zeros((2, 3))), r"\[n_out, n_stems \+ 1\]"),
    (dict(mix=np.zeros(4)), r"\[n_out, n_stems \+ 1\]"),
    (dict(mix=np.zeros((4, 4))), r"\[n_out, n_stems \+ 1\]"),                # n_out > n_stems
    (dict(mix=[[1.0, float("nan"), 0.0, 0.0]]), "finite"),
    (dict(mask_extension="zeros"), "mask_extension"),
    (dict(mask_extension=2), "mask_extension"),
    (dict(iterations=0), "iterations"),
    (dict(iterations=4), "iterations"),
    (dict(overlap=33), "overlap"),
    (dict(overlap=-1), "overlap"),
])
def test_binding_refuses_bad_options_before_any_call(kw, match):
    from spleeterrt_amd.capi import Engine, EngineError
    from spleeterrt_amd import capi
    with pytest.raises(EngineError, match=match):
        Engine.istft_wiener(_Stub(), None, None, **kw)
    with pytest.raises(EngineError, match=match):
        Engine.separate_wiener(_Stub(), None, None, **kw)
    assert [f[0] for f in capi._WienerOpts._fields_] == ["iterations", "overlap_rows", "mask_extension", "n_out", "h_gain"]


# ------------------------------------------------------------------------------------------------------------------------------ GPU
_CASES = {}


def _case(oracle, F):
    """the spectrum of the ragged clip (277 rows) on the device and as complex128, shared by the tests of one F"""
    if F not in _CASES:
        L, R = _stereo_clip(N_RAGGED, 100 + F)
        re_, im_ = oracle.stft(L, R)
        spec_t = _spec_tensor(re_, im_)
        assert spec_t.shape[1] == 277
        _CASES[F] = (spec_t, _to_complex(spec_t))
    return _CASES[F]


def _masks(rows, F, O, seed, S=S_S):
    from spleeterrt_amd import stream
    return np.random.default_rng(seed).random((S, stream.overlap_tiles(rows, T_S, O), 2, T_S, F), dtype=np.float32)


def _bare(F, max_tiles=8, S=S_S, **kw):
    """an engine without networks (the transform-level entry points need none)"""
    import spleeterrt_amd as srt
    return srt.Engine(F=F, T=T_S, stem_modes=(1, 0, 1, 0)[:S], oob_weights=OOB[:S] if S <= 3 else None, max_tiles=max_tiles, **kw)


def _opts(iters=1, O=0, ext=0, G=None, n_out=None):
    """(srt_wiener_opts, the matrix it points into).  n_out: overrides the matrix's row count (out of range, or in range with a null matrix)"""
    from spleeterrt_amd.capi import _WienerOpts
    g = None if G is None else np.ascontiguousarray(G, np.float32)
    o = _WienerOpts(iters, O, ext, 0 if g is None else g.shape[0], None if g is None else g.ctypes.data_as(C.POINTER(C.c_float)))
    if n_out is not None:
        o.n_out = n_out
    return o, g


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ex(eng, spec_t, masks_t, out_t, iters=1, rows=277, **kw):
    """srtIstftWienerEx itself (Engine.istft_wiener takes srtIstftWiener when every option is off); returns the code"""
    o, _g = _opts(iters, **kw)
    return eng.L.srtIstftWienerEx(eng.h, _p(spec_t), rows, _p(masks_t), C.byref(o), _p(out_t))


def _sep(eng, L, R, n, out_t, **kw):
    """srtSeparateWiener itself; returns the code"""
    o, _g = _opts(**kw)
    return eng.L.srtSeparateWiener(eng.h, _p(L), _p(R), n, C.byref(o), _p(out_t))


def _timed(eng, call):
    eng.set_timing(True)
    out = call()
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    return out, ks


def _rel_rms_stems(got, ref):
    return [float(np.sqrt(np.mean((got[j] - ref[j]) ** 2)) / np.sqrt(np.mean(ref[j] ** 2))) for j in range(ref.shape[0])]


def _check_covs(eng, covs, S):
    """the R tables, weight sums and a of every iteration against the restatement's: test_wiener.py's bounds"""
    for it, (Rn, wsum, a) in enumerate(covs, 1):
        for j in range(S):
            Rg, wg, ag = eng.wiener_cov(j, it)
            assert abs(ag - a) <= 1e-6 * a
            Rref = np.stack([Rn[j, :, 0, 0].real, Rn[j, :, 1, 1].real, Rn[j, :, 0, 1].real, Rn[j, :, 0, 1].imag], 1)
            d = np.abs(Rg - Rref).max() / np.abs(Rref).max()
            assert d <= 1e-4, (it, j, d)
            wref = wsum[j] * a * a / 4096.0 ** 2
            assert np.abs(wg - wref).max() <= 1e-4 * np.abs(wref).max()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_defaults_are_the_old_path(oracle, F):
    """srtIstftWienerEx with every option off against srtIstftWiener: the same bits, the same launches, the same R tables"""
    import torch
    spec_t, _ = _case(oracle, F)
    rows = spec_t.shape[1]
    m_t = torch.from_numpy(_masks(rows, F, 0, 5)).cuda()
    eng = _bare(F)
    for iters in (1, 3):
        old, ks_old = _timed(eng, lambda: eng.istft_wiener(spec_t, m_t, iters))
        cov_old = [eng.wiener_cov(j, it) for j in range(S_S) for it in range(1, iters + 1)]
        new = torch.full_like(old, float("nan"))
        rc, ks_new = _timed(eng, lambda: _ex(eng, spec_t, m_t, new, iters))
        assert rc == 0, eng.L.srtLastError()
        assert ks_new == ks_old and len(ks_old) == 2 * iters + 1 + S_S, (ks_old, ks_new)
        assert torch.equal(new, old)
        cov_new = [eng.wiener_cov(j, it) for j in range(S_S) for it in range(1, iters + 1)]
        for (Ra, wa, aa), (Rb, wb, ab) in zip(cov_old, cov_new):
            assert np.array_equal(Ra, Rb) and np.array_equal(wa, wb) and aa == ab
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2])
def test_separate_wiener_defaults_are_separate_under_set_wiener(oracle, coeffs, iters):
    import torch
    L, R = _audio(oracle, N_RAGGED, 61)
    eng = _engine(coeffs, max_tiles=8, batch_invariant=True)
    new, ks_new = _timed(eng, lambda: eng.separate_wiener(L, R, iters).clone())
    eng.set_wiener(iters)
    old, ks_old = _timed(eng, lambda: eng.separate(L, R).clone())
    assert ks_new == ks_old, (ks_old, ks_new)
    assert torch.equal(new, old)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("O", [16, 32])
@pytest.mark.parametrize("F", [512, 1536])
def test_overlap_in_the_statistics_and_the_filter(oracle, F, O, iters):
    """ref64: wiener_np on the host-blended rows through oracle.istft.  err_old: the existing srtIstftWiener at O = 0 on the host-blended, repacked masks
    (the parent's kernels).  err_new: srtIstftWienerEx on the overlapped layout.  err_new <= max(2 err_old, 1e-6) in rel-RMS per stem: the two kernel pairs
    may differ in contraction and in nothing else.  At n = 1 also the project's absolute bounds; the R tables and a to test_wiener.py's bounds."""
    import torch
    spec_t, spec_c = _case(oracle, F)
    rows = spec_t.shape[1]
    m = _masks(rows, F, O, 7 * O + iters)
    packed = _pack_rows(_blend_rows(m, rows, T_S, O), T_S)
    out, covs = wiener_np(spec_c, packed, T_S, F, iters, OOB)
    ref64 = _istft_of(oracle, out)
    eng = _bare(F)
    old = eng.istft_wiener(spec_t, torch.from_numpy(packed).cuda(), iters).cpu().numpy()
    new, ks = _timed(eng, lambda: eng.istft_wiener(spec_t, torch.from_numpy(m).cuda(), iters, overlap=O).cpu().numpy())
    names = [k for _, k in ks]
    assert sum(k == "srt_wiener_stats_ov_kernel" for k in names) == iters, names
    assert sum(k.startswith("srt_wiener_filter_opt_kernel<true>") for k in names) == 1, names
    assert not any(k.startswith(("srt_wiener_stats_kernel", "srt_wiener_filter_kernel")) for k in names), names
    assert sum(n == "istft" for n, _ in ks) == S_S
    err_old, err_new = _rel_rms_stems(old, ref64), _rel_rms_stems(new, ref64)
    print("F=%d O=%d n=%d: err_old %s err_new %s, old and new bit-equal: %s" % (F, O, iters, ["%.3g" % x for x in err_old], ["%.3g" % x for x in err_new], np.array_equal(old, new)))
    for j in range(S_S):
        assert err_new[j] <= max(2 * err_old[j], 1e-6), (j, err_new[j], err_old[j])
    if iters == 1:
        _compare(new, ref64, "overlap F=%d O=%d" % (F, O))
    _check_covs(eng, covs, S_S)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_one_tile_with_an_overlap_equals_no_overlap(oracle, F):
    """rows <= T: one tile at any overlap, no row is blended - the overlap kernels give the bits of the O = 0 call"""
    import torch
    spec_t, _ = _case(oracle, F)
    rows = 50
    sp = torch.zeros((2, rows, spec_t.shape[2], 2), device="cuda")
    sp.copy_(spec_t[:, 100:100 + rows])
    m_t = torch.from_numpy(_masks(rows, F, 16, 9)).cuda()
    assert m_t.shape[1] == 1
    eng = _bare(F)
    for iters in (1, 2):
        ref = eng.istft_wiener(sp, m_t, iters)
        got, ks = _timed(eng, lambda: eng.istft_wiener(sp, m_t, iters, overlap=16))
        assert any(k == "srt_wiener_stats_ov_kernel" for _, k in ks), ks
        assert torch.equal(got, ref), float((got - ref).abs().max())
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O", [0, 16])
@pytest.mark.parametrize("F", [512, 1536])
def test_average_extension(oracle, F, O):
    """the table is the one srtIstft leaves for the same masks and overlap (set_overlap + set_mask_extension("average") + istft, an existing path), bit for bit;
    the stems follow the restatement with e_j(r, c) s above F (the oob weights (0, 1, 0.25) would miss by far)"""
    import torch
    spec_t, spec_c = _case(oracle, F)
    rows = spec_t.shape[1]
    m = _masks(rows, F, O, 13 + O)
    m_t = torch.from_numpy(m).cuda()
    ref_eng = _bare(F, mask_extension="average")
    ref_eng.set_overlap(O)
    ref_eng.istft(spec_t, m_t)
    want = np.stack([ref_eng.mask_ext(s, rows) for s in range(S_S)])
    ref_eng.close()
    eng = _bare(F)                                                          # never called srtSetMaskExtension: the call allocates the table
    got, ks = _timed(eng, lambda: eng.istft_wiener(spec_t, m_t, 1, overlap=O, mask_extension="average").cpu().numpy())
    assert ("mask_ext", "srt_mask_ext_kernel<false, false, %s>" % ("true" if O else "false")) in ks, ks
    assert sum(k.startswith("srt_wiener_filter_opt_kernel<%s>" % ("true" if O else "false")) for _, k in ks) == 1, ks
    tab = np.stack([eng.mask_ext(s, rows) for s in range(S_S)])
    assert np.array_equal(tab, want)
    out, _, e = wiener_opts_np(spec_c, m, T_S, F, 1, OOB, overlap=O, average=True)
    assert np.abs(tab - e.transpose(0, 2, 1)).max() <= 1e-5
    _compare(got, _istft_of(oracle, out), "average F=%d O=%d" % (F, O))
    const, _, _ = wiener_opts_np(spec_c, m, T_S, F, 1, OOB, overlap=O)
    assert max(_rel_rms_stems(got, _istft_of(oracle, const))) > 1e-2      # the constant rule is far away: the bound above is not vacuous
    assert eng.mask_extension == 0
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_mix_one_hot_is_the_stems(oracle, F):
    import torch
    spec_t, _ = _case(oracle, F)
    rows = spec_t.shape[1]
    m_t = torch.from_numpy(_masks(rows, F, 16, 17)).cuda()
    eng = _bare(F)
    for iters in (1, 2):
        stems = eng.istft_wiener(spec_t, m_t, iters, overlap=16, mask_extension="average")
        hot, ks = _timed(eng, lambda: eng.istft_wiener(spec_t, m_t, iters, overlap=16, mask_extension="average", mix=np.eye(S_S, S_S + 1)))
        assert sum(k.startswith("srt_wiener_filter_opt_kernel<true>") for _, k in ks) == 1, ks
        assert torch.equal(hot, stems)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F,O,average", [(512, 16, True), (1536, 0, False), (1536, 32, True)])
def test_mix_against_the_restatement(oracle, F, O, average):
    """a karaoke row and a general 2 x (S + 1) matrix; only n_out spectra are inverted"""
    import torch
    spec_t, spec_c = _case(oracle, F)
    rows = spec_t.shape[1]
    m = _masks(rows, F, O, 19 + O)
    m_t = torch.from_numpy(m).cuda()
    eng = _bare(F)
    general = np.random.default_rng(23).uniform(-1.0, 1.0, (2, S_S + 1)).astype(np.float32)
    for name, G in (("karaoke", KARAOKE), ("general", general)):
        got, ks = _timed(eng, lambda: eng.istft_wiener(spec_t, m_t, 1, overlap=O, mask_extension="average" if average else "constant", mix=G).cpu().numpy())
        assert got.shape[0] == G.shape[0] and sum(n == "istft" for n, _ in ks) == G.shape[0], ks
        assert sum(k.startswith("srt_wiener_filter_opt_kernel<%s>" % ("true" if O else "false")) for _, k in ks) == 1, ks
        out, _, _ = wiener_opts_np(spec_c, m, T_S, F, 1, OOB, overlap=O, average=average, mix=G)
        _compare(got, _istft_of(oracle, out), "mix %s F=%d O=%d" % (name, F, O))
    eng.close()


@pytest.mark.gpu
def test_mix_writes_its_planes_and_nothing_else(oracle):
    import torch
    F = 512
    spec_t, _ = _case(oracle, F)
    rows = spec_t.shape[1]
    m_t = torch.from_numpy(_masks(rows, F, 16, 29)).cuda()
    eng = _bare(F)
    G = np.random.default_rng(31).uniform(-1.0, 1.0, (2, S_S + 1)).astype(np.float32)
    out = torch.full((3, 2, eng.L.srtIstftLength(rows)), float("nan"), device="cuda")
    assert _ex(eng, spec_t, m_t, out, 1, O=16, ext=1, G=G) == 0, eng.L.srtLastError()
    assert bool(torch.isfinite(out[:2]).all()) and bool(torch.isnan(out[2]).all())
    assert torch.equal(out[:2], eng.istft_wiener(spec_t, m_t, 1, overlap=16, mask_extension="average", mix=G))
    eng.close()


def _state_probe(eng, spec_t, m_t):
    """what an existing entry point does under the engine's own settings: output and launch list of srtIstft"""
    out, ks = _timed(eng, lambda: eng.istft(spec_t, m_t).clone())
    return out, ks, eng.mix_outputs, eng.overlap, eng.mask_extension


@pytest.mark.gpu
def test_separate_wiener_is_the_composition_of_its_stages(oracle, coeffs):
    """S = 2 with real networks: separate_wiener with every option on = stft + forward in the overlapped layout, then istft_wiener with the same options;
    the engine's own overlap / mix / extension settings (all on, all different) are as before the call"""
    import torch
    L, R = _audio(oracle, N_RAGGED, 62)
    G = np.array([[-1.0, 0.0, 1.0], [0.5, 0.25, 0.0]], np.float32)
    eng = _engine(coeffs, max_tiles=8, batch_invariant=True)
    eng.set_overlap(16)
    spec, mag = eng.stft(L, R)
    masks = eng.forward(mag)
    eng.set_overlap(0)
    want = eng.istft_wiener(spec, masks, 1, overlap=16, mask_extension="average", mix=G)
    eng.set_overlap(32)
    eng.set_mask_extension("average")
    eng.set_mix([[0.0, 1.0, 0.5]])
    m32 = torch.rand((2, eng.tiles(spec.shape[1]), 2, T_S, 512), device="cuda")
    before = _state_probe(eng, spec, m32)
    got, ks = _timed(eng, lambda: eng.separate_wiener(L, R, 1, overlap=16, mask_extension="average", mix=G))
    assert ks[0] == ("stft", "srt_stft_ov_kernel"), ks[0]
    assert torch.equal(got, want)
    after = _state_probe(eng, spec, m32)
    assert torch.equal(before[0], after[0]) and before[1:] == after[1:] and after[2:] == (1, 32, 1)
    eng.close()


@pytest.mark.gpu
def test_fp16_mode(oracle, coeffs):
    """precision 1: the stems against the engine's own stft + forward masks through the restatement; the masks the forward left are fp32 (no half head kernel)"""
    import torch
    import spleeterrt_amd as srt
    L, R = _audio(oracle, N_RAGGED, 63)
    eng = _engine(coeffs, max_tiles=8, precision=srt.PREC_F16)
    got, ks = _timed(eng, lambda: eng.separate_wiener(L, R, 1, overlap=16).cpu().numpy())
    assert not any(re.match(r"srt_head_rows_kernel<\w+, 4, true>", k) for _, k in ks), ks
    assert any(k == "srt_wiener_stats_ov_kernel" for _, k in ks)
    eng.set_overlap(16)
    spec, mag = eng.stft(L, R)
    masks = eng.forward(mag)
    assert masks.dtype == torch.float32
    eng.set_overlap(0)
    assert torch.equal(torch.from_numpy(got).cuda(), eng.istft_wiener(spec, masks, 1, overlap=16))
    out, _, _ = wiener_opts_np(_to_complex(spec), masks.cpu().numpy(), T_S, 512, 1, [0.1, 0.1], overlap=16)
    _compare(got, _istft_of(oracle, out), "fp16 mode")
    eng.close()


@pytest.mark.gpu
def test_engine_state_is_ignored(oracle):
    import torch
    import spleeterrt_amd as srt
    F = 512
    spec_t, _ = _case(oracle, F)
    rows = spec_t.shape[1]
    m16 = torch.from_numpy(_masks(rows, F, 16, 37)).cuda()
    m0 = torch.from_numpy(_masks(rows, F, 0, 38)).cuda()
    G = np.array([[0.25, -1.0, 0.5, 1.0]], np.float32)
    fresh = _bare(F)
    want = fresh.istft_wiener(spec_t, m16, 2, overlap=16, mix=G)
    want0 = fresh.istft_wiener(spec_t, m0, 2)
    fresh.close()
    eng = _bare(F)
    eng.set_overlap(32)
    eng.set_mix([[1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.5]])
    eng.set_mask_extension("average")
    assert torch.equal(eng.istft_wiener(spec_t, m16, 2, overlap=16, mix=G), want)
    got0 = torch.full_like(want0, float("nan"))
    assert _ex(eng, spec_t, m0, got0, 2) == 0, eng.L.srtLastError()         # every option off, the engine's three all on
    assert torch.equal(got0, want0)
    assert (eng.mix_outputs, eng.overlap, eng.mask_extension) == (2, 32, 1)
    for undo, word in ((lambda: eng.set_mix(None), "mix"), (lambda: eng.set_overlap(0), "overlap"), (lambda: eng.set_mask_extension("constant"), "mask extension")):
        with pytest.raises(srt.EngineError, match="srtIstftWiener: not available with .*" + word):
            eng.istft_wiener(spec_t, m0, 1)
        undo()
    assert torch.equal(eng.istft_wiener(spec_t, m0, 2), want0)
    eng.close()


@pytest.mark.gpu
def test_refusals(oracle, coeffs):
    """-1 (or -5) with a text that names the function, the NaN-prefilled output untouched, nothing launched"""
    import torch
    F = 512
    spec_t, _ = _case(oracle, F)
    rows = spec_t.shape[1]
    m_t = torch.from_numpy(_masks(rows, F, 32, 41)).cuda()                 # 8 tiles: enough for every layout below
    L, R = _audio(oracle, N_RAGGED, 64)
    nan = float("nan")
    bad = np.eye(S_S, S_S + 1, dtype=np.float32)
    bad[1, 2] = np.inf
    def refused(eng, call, code, who, word=None):
        out = torch.full((eng.S, 2, eng.L.srtIstftLength(rows)), nan, device="cuda")
        eng.set_timing(True)
        rc = call(out)
        launched = eng.get_timing()
        eng.set_timing(False)
        text = eng.L.srtLastError().decode()
        assert rc == code and who in text and (word is None or word in text), (rc, text)
        assert launched == [] and bool(torch.isnan(out).all()), (launched, text)

    bad_opts = (dict(iters=0), dict(iters=4), dict(O=-1), dict(O=33), dict(ext=2), dict(ext=-1), dict(n_out=-1), dict(n_out=S_S + 1), dict(n_out=2), dict(G=bad))
    eng = _bare(F)
    net = _engine(coeffs, S=S_S, max_tiles=8)
    for kw in bad_opts:
        word = "n_stems spectra" if kw.get("n_out") == S_S + 1 else None
        refused(eng, lambda out: _ex(eng, spec_t, m_t, out, **kw), -1, "srtIstftWienerEx", word)
        refused(net, lambda out: _sep(net, L, R, N_RAGGED, out, **kw), -1, "srtSeparateWiener", word)
    # null arguments and opts
    refused(eng, lambda out: _ex(eng, None, m_t, out), -1, "srtIstftWienerEx")
    refused(eng, lambda out: _ex(eng, spec_t, None, out), -1, "srtIstftWienerEx")
    refused(eng, lambda out: eng.L.srtIstftWienerEx(eng.h, _p(spec_t), rows, _p(m_t), None, _p(out)), -1, "srtIstftWienerEx")
    assert _ex(eng, spec_t, m_t, None) == -1 and b"srtIstftWienerEx" in eng.L.srtLastError()
    refused(net, lambda out: _sep(net, None, R, N_RAGGED, out), -1, "srtSeparateWiener")
    refused(net, lambda out: _sep(net, L, None, N_RAGGED, out), -1, "srtSeparateWiener")
    refused(net, lambda out: net.L.srtSeparateWiener(net.h, _p(L), _p(R), N_RAGGED, None, _p(out)), -1, "srtSeparateWiener")
    assert _sep(net, L, R, N_RAGGED, None) == -1 and b"srtSeparateWiener" in net.L.srtLastError()
    refused(net, lambda out: _sep(net, L, R, 4095, out), -1, "srtSeparateWiener")
    # weights not set
    refused(eng, lambda out: _sep(eng, L, R, N_RAGGED, out), -5, "srtSeparateWiener")
    eng.close()
    net.close()
    # more than max_tiles overlapped tiles: 277 rows are 5 tiles back to back, 6 at O = 16
    small = _bare(F, max_tiles=5)
    refused(small, lambda out: _ex(small, spec_t, m_t, out, O=16), -1, "srtIstftWienerEx")
    out = torch.full((S_S, 2, small.L.srtIstftLength(rows)), nan, device="cuda")
    assert _ex(small, spec_t, m_t, out) == 0 and bool(torch.isfinite(out).all())
    small.close()
    small = _engine(coeffs, S=2, max_tiles=5)
    refused(small, lambda out: _sep(small, L, R, N_RAGGED, out, O=16), -1, "srtSeparateWiener")
    small.close()
    # ratio_mask
    rm = _bare(F, ratio_mask=True)
    refused(rm, lambda out: _ex(rm, spec_t, m_t, out), -1, "srtIstftWienerEx")
    rm.close()
    rm = _engine(coeffs, S=2, max_tiles=8, ratio_mask=True)
    refused(rm, lambda out: _sep(rm, L, R, N_RAGGED, out), -1, "srtSeparateWiener")
    rm.close()
