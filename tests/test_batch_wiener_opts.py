"""srtSeparateBatchWienerEx: the Wiener filter per track of a packed batch with the per-call options of srtSeparateWiener - overlapped tiles
inside every track, the average mask extension and a stem remix per track.  The contract: output m of track k is what srtSeparateWiener writes for that track
alone under the same options (bit for bit with batch_invariant), whatever else the batch holds and wherever the track sits in it.

Shapes: T = 64, F in {512, 1536}, the five tracks of tests/test_batch_wiener.py at its LEVELS: 64, 4, 105, 49 and 137 rows - 8 packed tiles at O = 0 and O = 16,
10 at O = 32 (max_tiles is sized from srtBatchPlanOverlap).  One-tile tracks (the overlap is a no-op; 64 rows = T exactly), a two-tile track whose last rows hit
the primary-tile clamp (105 rows at O = 16: rows 96..104 have r / 48 = 2), a three- or four-tile track, row counts that are no multiple of 16 (a filter block
straddles a track's end) and tile padding between tracks.  The float64 restatement is tests/test_wiener_opts.py's wiener_opts_np at tests/test_wiener.py's bounds
(measured on an MI355X: rel-RMS <= 4.3e-7, max <= 4.3e-7 of the peak; all six solo cases bit-equal).  The refusal of more than 65 535 blocks of 16 packed rows
has no test here: it needs max_tiles * T >= 1 048 576 rows, an engine of tens of GB."""
import ctypes as C

import numpy as np
import pytest

import test_wiener as TW
from test_batch_wiener import TRACKS, T_S, _covs, _engine, _same_covs, _tracks
from test_wiener_opts import wiener_opts_np

ROWS = (64, 4, 105, 49, 137)
WHO = "srtSeparateBatchWienerEx"
SINGLE_KERNELS = ("srt_wiener_stats_kernel", "srt_wiener_stats_ov_kernel", "srt_wiener_finalize_kernel", "srt_wiener_filter_kernel", "srt_wiener_filter_opt_kernel")


def _karaoke(S):
    """the input minus stem 0"""
    g = np.zeros((1, S + 1), np.float32)
    g[0, 0], g[0, S] = -1.0, 1.0
    return g


def _per_track(S, K, n_out=2, seed=5):
    """K different general matrices [n_out, S + 1]"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (K, n_out, S + 1)).astype(np.float32)


PLANS = {0: ([0, 1, 2, 4, 5], 8), 16: ([0, 1, 2, 4, 5], 8), 32: ([0, 1, 2, 5, 6], 10)}      # TRACKS: (tile0, packed tiles) the docstring's cases rest on


def _plan(ns, O, T=T_S):
    """(tile0 per track, packed tile total) from srtBatchPlanOverlap; for TRACKS at T = 64 also the guard that the shapes are the ones the docstring names"""
    import spleeterrt_amd
    L = spleeterrt_amd.load_library()
    K = len(ns)
    tile0, total = (C.c_size_t * K)(), C.c_size_t(0)
    assert L.srtBatchPlanOverlap((C.c_size_t * K)(*ns), K, T, O, tile0, C.byref(total)) == 0, L.srtLastError()
    if tuple(ns) == TRACKS and T == T_S and O in PLANS:
        assert tuple(L.srtStftRows(n) for n in ns) == ROWS and (list(tile0), int(total.value)) == PLANS[O], (O, list(tile0), total.value)
    return list(tile0), int(total.value)


# ------------------------------------------------------------------------------------------------------------------------------ CPU: refusals without a device
def test_null_engine_and_null_opts_are_refused():
    import spleeterrt_amd
    from spleeterrt_amd.capi import _BatchWienerOpts
    L = spleeterrt_amd.load_library()
    o = _BatchWienerOpts(1, 0, 0, 0, None, 0)
    assert L.srtSeparateBatchWienerEx(None, 1, None, None, None, None, C.byref(o)) == -1
    assert WHO.encode() in L.srtLastError()
    assert L.srtSeparateBatchWienerEx(None, 1, None, None, None, None, None) == -1
    assert WHO.encode() in L.srtLastError()
    assert [f[0] for f in _BatchWienerOpts._fields_] == ["iterations", "overlap_rows", "mask_extension", "n_out", "h_gain", "gain_stride"]


class _Stub:
    """stands in for an Engine: any library call is a failure of the test"""
    S, T = 4, 64

    def __getattr__(self, name):
        raise AssertionError("the argument checks must raise before %r is touched" % name)


@pytest.mark.parametrize("kw,match", [
    (dict(iterations=0), "iterations"),
    (dict(iterations=4), "iterations"),
    (dict(iterations="two"), "iterations"),
    (dict(overlap=-1), "overlap"),
    (dict(overlap=33), "overlap"),
    (dict(mask_extension="zeros"), "mask_extension"),
    (dict(mask_extension=2), "mask_extension"),
    (dict(mix=np.zeros((2, 4))), r"\[n_out, n_stems \+ 1\]"),                # S columns instead of S + 1
    (dict(mix=np.zeros(5)), r"\[n_out, n_stems \+ 1\]"),
    (dict(mix=np.zeros((5, 5))), r"\[n_out, n_stems \+ 1\]"),                # n_out > n_stems
    (dict(mix=np.zeros((3, 2, 5))), r"\[n_out, n_stems \+ 1\]"),             # three matrices for two tracks
    (dict(mix=[[1.0, float("nan"), 0.0, 0.0, 0.0]]), "finite"),
    (dict(mix=[np.zeros((2, 5)), np.full((2, 5), np.inf)]), "finite"),
    (dict(mix=[np.zeros((1, 5)), np.zeros((2, 5))]), "same n_out"),          # per-track matrices with two different n_out
])
def test_binding_refuses_bad_options_before_any_call(kw, match):
    from spleeterrt_amd.capi import Engine, EngineError
    with pytest.raises(EngineError, match=match):
        Engine.separate_batch_wiener(_Stub(), [(None, None), (None, None)], **kw)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _p(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in ts])


def _raw(eng, tr, outs, iters=1, O=0, ext=0, G=None, n_out=None, stride=None, ns=None, k=None, opts=True):
    """srtSeparateBatchWienerEx itself; G [n_out, S + 1] (stride 0) or [K, n_out, S + 1]; n_out / stride override what G implies.  Returns the code"""
    from spleeterrt_amd.capi import _BatchWienerOpts
    g = None if G is None else np.ascontiguousarray(G, np.float32)
    no = 0 if g is None else g.shape[-2]
    st = 0 if g is None or g.ndim == 2 else no * g.shape[-1]
    o = _BatchWienerOpts(iters, O, ext, no if n_out is None else n_out, None if g is None else g.ctypes.data_as(C.POINTER(C.c_float)), st if stride is None else stride)
    ns = [int((b if a is None else a).numel()) for a, b in tr] if ns is None else ns
    return eng.L.srtSeparateBatchWienerEx(eng.h, len(tr) if k is None else k, _p([a for a, _ in tr]), _p([b for _, b in tr]), (C.c_size_t * len(ns))(*ns), _p(outs),
                                          C.byref(o) if opts else None)


def _nan_outs(eng, ns, planes, guard=0):
    import torch
    L = eng.L
    return [torch.full((planes * 2 * L.srtIstftLength(L.srtStftRows(n)) + guard,), float("nan"), device="cuda") for n in ns]


def _timed(eng, call):
    eng.set_timing(True)
    out = call()
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    return out, ks


def _tables(eng, S, total):
    """the gain table over the packed rows, [S, total * T, 2]"""
    return np.stack([eng.mask_ext(s, total * T_S) for s in range(S)])


def _solo_against_batch(eng, tr, S, iters, O, ext, G, tile0, total, tag):
    """ONE batch call, then srtSeparateWiener per track: stems, R tables, weight sums, a and (average) the track's rows of the gain table, all bit for bit.
    G: None, [n_out, S + 1] for all, or [K, n_out, S + 1].  Returns (the batch outputs, the batch launches)"""
    import torch
    got, ks = _timed(eng, lambda: [o.clone() for o in eng.separate_batch_wiener(tr, iterations=iters, overlap=O, mask_extension=ext, mix=G)])
    covs = [_covs(eng, S, iters, track=k) for k in range(len(tr))]
    tab = _tables(eng, S, total) if ext == "average" else None
    for k, (L, R) in enumerate(tr):
        Gk = None if G is None else (G if np.ndim(G) == 2 else G[k])
        ref = eng.separate_wiener(L, R, iters, overlap=O, mask_extension=ext, mix=Gk)
        assert got[k].shape == ref.shape, (tag, k)
        assert _same_covs(covs[k], _covs(eng, S, iters)), (tag, k)
        if tab is not None:
            rows = ROWS[TRACKS.index(int(L.numel()))]
            solo = np.stack([eng.mask_ext(s, rows) for s in range(S)])
            assert np.array_equal(tab[:, tile0[k] * T_S:tile0[k] * T_S + rows], solo), (tag, k)
        assert torch.equal(got[k], ref), (tag, k, float((got[k] - ref).abs().max()))
    return got, ks


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_options_off_is_the_old_call(oracle, coeffs, F):
    """overlap 0, the constant rule, no mix: the launches, the bits and the tables of srtSeparateBatchWiener"""
    import torch
    S = 2
    eng = _engine(coeffs, S, F=F, max_tiles=_plan(TRACKS, 0)[1])
    tr = _tracks(oracle, TRACKS, seed=1100)
    for iters in (1, 2):
        old, ks_old = _timed(eng, lambda: [o.clone() for o in eng.separate_batch(tr, wiener=iters)])
        cov_old = [_covs(eng, S, iters, track=k) for k in range(len(tr))]
        new = _nan_outs(eng, TRACKS, S)
        rc, ks_new = _timed(eng, lambda: _raw(eng, tr, new, iters))
        assert rc == 0, eng.L.srtLastError()
        assert ks_new == ks_old, (ks_old, ks_new)
        assert any(k == "srt_wiener_filter_batch_kernel" for _, k in ks_new), ks_new
        for k in range(len(tr)):
            assert torch.equal(new[k], old[k].reshape(-1)), k
            assert _same_covs(cov_old[k], _covs(eng, S, iters, track=k)), k
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F,O,iters,ext,mix", [
    (512, 16, 1, "constant", None),
    (1536, 32, 2, "average", None),
    (512, 16, 2, "average", "per-track"),
    (1536, 0, 1, "average", None),
    (512, 0, 3, "constant", "karaoke"),
    (1536, 32, 3, "constant", None),
])
def test_every_track_equals_the_solo_call(oracle, coeffs, F, O, iters, ext, mix):
    """batch_invariant, 4 stems: stems, tables and the gain table of every track are srtSeparateWiener's on it alone, bit for bit; the launches are the batch
    kernels and none of the single-signal Wiener kernels"""
    S = 4
    tile0, total = _plan(TRACKS, O)
    eng = _engine(coeffs, S, F=F, max_tiles=total, batch_invariant=True)
    tr = _tracks(oracle, TRACKS, seed=1200)
    G = {None: None, "per-track": _per_track(S, len(tr)), "karaoke": _karaoke(S)}[mix]
    _, ks = _solo_against_batch(eng, tr, S, iters, O, ext, G, tile0, total, "F=%d O=%d n=%d %s %s" % (F, O, iters, ext, mix))
    names = [k for _, k in ks]
    assert sum(k == ("srt_wiener_stats_batch_ov_kernel" if O else "srt_wiener_stats_batch_kernel") for k in names) == iters, names
    assert sum(k == "srt_wiener_finalize_batch_kernel" for k in names) == iters, names
    assert sum(k.startswith("srt_wiener_filter_batch_opt_kernel<%s>" % ("true" if O else "false")) for k in names) == 1, names
    assert [k for k in names if k.startswith("srt_istft")] == ["srt_istft_batch_spec_kernel<%s>" % ("true" if F <= 1024 else "false")], names
    assert not any(k.startswith(SINGLE_KERNELS) or k == "srt_wiener_filter_batch_kernel" for k in names), names
    assert sum(n == "mask_ext" for n, _ in ks) == (1 if ext == "average" else 0), ks
    eng.close()


@pytest.mark.gpu
def test_position_independent(oracle, coeffs):
    """the same tracks (and their matrices) in reversed order: the same bits per track - stems, tables and gain-table rows"""
    import torch
    S, iters, O = 4, 2, 16
    tile0, total = _plan(TRACKS, O)
    rev0, _ = _plan(TRACKS[::-1], O)
    eng = _engine(coeffs, S, max_tiles=total, batch_invariant=True)
    tr = _tracks(oracle, TRACKS, seed=1300)
    G = _per_track(S, len(tr), seed=7)
    K = len(tr)
    fwd = [o.clone() for o in eng.separate_batch_wiener(tr, iterations=iters, overlap=O, mask_extension="average", mix=G)]
    cf, tf = [_covs(eng, S, iters, track=k) for k in range(K)], _tables(eng, S, total)
    rev = eng.separate_batch_wiener(tr[::-1], iterations=iters, overlap=O, mask_extension="average", mix=G[::-1])
    cr, trv = [_covs(eng, S, iters, track=k) for k in range(K)], _tables(eng, S, total)
    for k in range(K):
        assert torch.equal(fwd[k], rev[K - 1 - k]), k
        assert _same_covs(cf[k], cr[K - 1 - k]), k
        a, b = tile0[k] * T_S, rev0[K - 1 - k] * T_S
        assert np.array_equal(tf[:, a:a + ROWS[k]], trv[:, b:b + ROWS[k]]), k
    eng.close()


@pytest.mark.gpu
def test_against_the_float64_restatement(oracle, coeffs):
    """default mode, 4 stems, one iteration, O = 16, the average extension: each track against wiener_opts_np fed with the engine's own spectrum of that track and
    its masks from ONE srtForward over the packed overlapped magnitudes, through oracle.istft; tests/test_wiener.py's bounds (rel-RMS 1e-4, max 1e-3 of the peak)"""
    import torch
    S, O, F = 4, 16, 512
    _, total = _plan(TRACKS, O)
    eng = _engine(coeffs, S, max_tiles=total)
    tr = _tracks(oracle, TRACKS, seed=1400)
    got = [o.cpu().numpy() for o in eng.separate_batch_wiener(tr, iterations=1, overlap=O, mask_extension="average")]
    eng.set_overlap(O)
    st = [eng.stft(L, R) for L, R in tr]
    masks = eng.forward(torch.cat([m for _, m in st])).cpu().numpy()
    eng.set_overlap(0)
    t0 = 0
    for k, (spec, mag) in enumerate(st):
        nt = mag.shape[0]
        out, _, _ = wiener_opts_np(TW._to_complex(spec), masks[:, t0:t0 + nt], T_S, F, 1, [0.1] * S, overlap=O, average=True)
        t0 += nt
        ref = TW._istft_of(oracle, out)
        assert got[k].shape == ref.shape
        TW._compare(got[k], ref, "batch wiener opts track %d" % k)
    assert t0 == total
    eng.close()


@pytest.mark.gpu
def test_one_hot_matrices_give_the_stems(oracle, coeffs):
    """one-hot rows that differ per track reproduce the call's own stems bit for bit; the row (0, .., 0, 1) is the track's STFT -> iSTFT round trip"""
    import torch
    S, O, iters = 4, 16, 2
    _, total = _plan(TRACKS, O)
    eng = _engine(coeffs, S, max_tiles=total, batch_invariant=True)
    tr = _tracks(oracle, TRACKS, seed=1500)
    K = len(tr)
    stems = [o.clone() for o in eng.separate_batch_wiener(tr, iterations=iters, overlap=O, mask_extension="average")]
    G = np.zeros((K, 2, S + 1), np.float32)
    pick = [((k + 1) % S, S if k % 2 == 0 else (k + 2) % S) for k in range(K)]       # even tracks: a stem and the input; odd tracks: two stems
    for k, (a, b) in enumerate(pick):
        G[k, 0, a] = 1.0
        G[k, 1, b] = 1.0
    hot = eng.separate_batch_wiener(tr, iterations=iters, overlap=O, mask_extension="average", mix=G)
    for k, (a, b) in enumerate(pick):
        assert torch.equal(hot[k][0], stems[k][a]), k
        if b < S:
            assert torch.equal(hot[k][1], stems[k][b]), k
        else:
            spec, _ = eng.stft(*tr[k])
            ref = TW._istft_of(oracle, TW._to_complex(spec)[None, :, :, :2049])
            TW._compare(hot[k][1:2].cpu().numpy(), ref, "round trip track %d" % k)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 1])
def test_one_launch_per_stage(oracle, coeffs, K):
    """2 iterations, O = 16, average, one karaoke row: 1 stft_batch, 2 x (wiener_stats_batch, wiener_cov_batch), 1 mask_ext, 1 wiener_filter_batch, 1 istft_batch
    whatever K is; the network launches are srtForward's over the packed tile count"""
    import torch
    S, O = 2, 16
    ns = TRACKS[:K] if K > 1 else TRACKS[4:]
    _, total = _plan(ns, O)
    eng = _engine(coeffs, S, max_tiles=total)
    tr = _tracks(oracle, ns, seed=1600)
    kw = dict(iterations=2, overlap=O, mask_extension="average", mix=_karaoke(S))
    eng.separate_batch_wiener(tr, **kw)                              # (first call allocates; not part of the count)
    out, ks = _timed(eng, lambda: eng.separate_batch_wiener(tr, **kw))
    assert all(bool(torch.isfinite(o).all()) for o in out)
    names = [n for n, _ in ks]
    tail = ["wiener_stats_batch", "wiener_cov_batch", "wiener_stats_batch", "wiener_cov_batch", "mask_ext", "wiener_filter_batch", "istft_batch"]
    assert names[0] == "stft_batch" and names[-7:] == tail, names
    for n in set(tail) | {"stft_batch"}:
        assert names.count(n) == ([names[0]] + tail).count(n), (n, names)
    assert not any(n in ("wiener_stats", "wiener_cov", "wiener_filter", "istft", "stft") for n in names), names
    mag = torch.zeros((total, 2, T_S, 512), device="cuda")
    eng.forward(mag)
    _, ref = _timed(eng, lambda: eng.forward(mag))
    assert ks[1:-7] == ref
    eng.close()


@pytest.mark.gpu
def test_writes_its_planes_nothing_past_and_repeats(oracle, coeffs):
    """n_out = 1 of S = 2: NaN-filled outputs come back finite over the one plane pair, the second pair and the guard after it stay, two calls give the same bits"""
    import torch
    S, O = 2, 16
    _, total = _plan(TRACKS, O)
    eng = _engine(coeffs, S, max_tiles=total)
    tr = _tracks(oracle, TRACKS, seed=1700)
    L = eng.L
    need = [2 * L.srtIstftLength(L.srtStftRows(n)) for n in TRACKS]      # floats of ONE output
    G = _per_track(S, len(tr), n_out=1, seed=11)
    runs = []
    for _ in range(2):
        outs = _nan_outs(eng, TRACKS, S, guard=5000)
        for o, m in zip(outs, need):
            o[S * m:] = 12345.0
        assert _raw(eng, tr, outs, 2, O=O, ext=1, G=G) == 0, L.srtLastError()
        runs.append(outs)
    for k, m in enumerate(need):
        h = runs[0][k].cpu().numpy()
        assert np.isfinite(h[:m]).all(), (k, int(np.isnan(h[:m]).sum()))
        assert np.isnan(h[m:S * m]).all(), k                             # the plane pair beyond n_out
        assert (h[S * m:] == 12345.0).all(), k
        assert torch.equal(runs[0][k][:m], runs[1][k][:m]), k
    # every stem (n_out = 0): all S pairs written, the guard stays
    outs = _nan_outs(eng, TRACKS, S, guard=100)
    assert _raw(eng, tr, outs, 1, O=O) == 0, L.srtLastError()
    for k, m in enumerate(need):
        h = outs[k].cpu().numpy()
        assert np.isfinite(h[:S * m]).all() and np.isnan(h[S * m:]).all(), k
    eng.close()


@pytest.mark.gpu
def test_fp16_mode(oracle, coeffs):
    """SRT_PREC_F16, 5 stems, batch_invariant: no half-mask kernel among the launches, and each track equals the solo call"""
    import spleeterrt_amd as srt
    S, O = 5, 16
    tile0, total = _plan(TRACKS, O)
    eng = _engine(coeffs, S, max_tiles=total, precision=srt.PREC_F16, batch_invariant=True)
    tr = _tracks(oracle, TRACKS, seed=1800)
    _, ks = _solo_against_batch(eng, tr, S, 1, O, "average", None, tile0, total, "fp16")
    for _, k in ks:
        assert not k.startswith("srt_istft_batch_kernel") and not k.startswith("srt_istft_ola") and not k.startswith("srt_istft_batch_ov_kernel"), ks
        if k.startswith("srt_head_rows_kernel"):
            assert not k.rstrip("> ").endswith(", 4, true"), k                                             # the head's half-mask form
        if k.startswith("srt_mask_ext"):
            assert k.startswith("srt_mask_ext_batch_kernel<false,"), k                                     # the table from float masks
    assert [k for _, k in ks if k.startswith("srt_istft")] == ["srt_istft_batch_spec_kernel<true>"], ks
    eng.close()


@pytest.mark.gpu
def test_engine_state_is_ignored(oracle, coeffs):
    """set_overlap(16), set_mask_extension("average") and set_mix on the engine: the call gives the bits of a clean engine and leaves all three as they were"""
    import torch
    S, O = 2, 32
    _, total = _plan(TRACKS, O)
    tr = _tracks(oracle, TRACKS, seed=1900)
    G = _per_track(S, len(tr), seed=13)
    kw = dict(iterations=2, overlap=O, mask_extension="constant", mix=G)
    clean = _engine(coeffs, S, max_tiles=total, batch_invariant=True)
    want = [o.clone() for o in clean.separate_batch_wiener(tr, **kw)]
    want0 = [o.clone() for o in clean.separate_batch_wiener(tr, iterations=1)]
    clean.close()
    eng = _engine(coeffs, S, max_tiles=total, batch_invariant=True)
    eng.set_overlap(16)
    eng.set_mask_extension("average")
    eng.set_mix([[1.0, 1.0, 0.0], [0.0, 0.5, 0.25], [0.0, 0.0, 1.0]])
    Lq, Rq = tr[1]
    spec, mag = eng.stft(Lq, Rq)                                           # 4 rows: one tile at any overlap
    m_t = torch.rand((S,) + tuple(mag.shape), device="cuda")

    def probe():
        """what an existing entry point does under the engine's own settings: output and launch list of srtIstft"""
        out, ks = _timed(eng, lambda: eng.istft(spec, m_t).clone())
        return out, ks, eng.mix_outputs

    before = probe()
    for w, g in zip(want, eng.separate_batch_wiener(tr, **kw)):
        assert torch.equal(g, w)
    for w, g in zip(want0, eng.separate_batch_wiener(tr, iterations=1)):      # every option off under the engine's settings: still off
        assert torch.equal(g, w)
    after = probe()
    assert torch.equal(before[0], after[0]) and before[1:] == after[1:] and after[2] == 3
    assert (eng.overlap, eng.mask_extension) == (16, 1)
    eng.close()


@pytest.mark.gpu
def test_refusals(oracle, coeffs):
    """every refusal: -1 (or -5) with a text that names the function, nothing launched, the NaN-prefilled outputs untouched; a valid call afterwards succeeds; the
    four older batch entry points still refuse what they refused"""
    import torch
    import spleeterrt_amd as srt
    S = 2
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                   # (a non-default stream, so that the capture case below can capture it)
        eng = _engine(coeffs, S, max_tiles=4)
    L = eng.L
    tr = _tracks(oracle, TRACKS[:3], seed=2000)                    # 1 + 1 + 2 = 4 tiles at O = 0 and O = 16
    ns = [int(a.numel()) for a, _ in tr]
    outs = _nan_outs(eng, ns, S)
    torch.cuda.synchronize()

    def refused(code, word, e=None, **kw):
        e = e or eng
        e.set_timing(True)
        rc = _raw(e, kw.pop("tr", tr), kw.pop("outs", outs), **kw)
        launched = e.get_timing()
        e.set_timing(False)
        text = L.srtLastError().decode()
        assert rc == code and WHO in text and word in text, (rc, text, kw)
        assert launched == [], (launched, text)
        assert all(bool(torch.isnan(o).all()) for o in outs), text

    bad = np.zeros((3, 1, S + 1), np.float32)
    bad[2, 0, 1] = np.inf
    refused(-1, "opts", opts=False)
    refused(-1, "null", tr=[tr[0], (None, tr[1][1]), tr[2]])
    refused(-1, "null", tr=[tr[0], (tr[1][0], None), tr[2]])
    refused(-1, "null", outs=[outs[0], outs[1], None])
    refused(-1, "4096", ns=[ns[0], 4095, ns[2]])
    refused(-1, "ntracks", k=0)
    assert L.srtSeparateBatchWienerEx(eng.h, 3, None, None, None, None, None) == -1 and WHO.encode() in L.srtLastError()
    for it in (0, 4, -1):
        refused(-1, "iterations", iters=it)
    for O in (-1, 33):
        refused(-1, "overlap", O=O)
    for ext in (2, -1):
        refused(-1, "mask_extension", ext=ext)
    refused(-1, "n_stems spectra", n_out=S + 1)
    refused(-1, "n_out", n_out=-1)
    refused(-1, "null gain", n_out=1)
    refused(-1, "gain_stride", G=bad, stride=S)
    refused(-1, "track 2", G=bad)
    refused(-1, "finite", G=bad[2])
    (Ll, Rl), = _tracks(oracle, [140077], seed=2100)
    ol = _nan_outs(eng, [140077], S)[0]
    big = dict(tr=[tr[0], tr[1], (Ll, Rl)], outs=[outs[0], outs[1], ol])
    refused(-1, "max_tiles", O=16, **big)                           # 1 + 1 + 3 overlapped tiles
    assert bool(torch.isnan(ol).all())
    er = _engine(coeffs, S, max_tiles=4, ratio_mask=True)
    refused(-1, "ratio_mask", e=er)
    er.close()
    bare = srt.Engine(F=512, T=T_S, stem_modes=(1, 0), variant=srt.VARIANT_VST, max_tiles=4)
    refused(-5, "weights", e=bare)
    bare.close()
    torch.cuda.synchronize()
    dummy = torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                      # the engine's stream is capturing: refused before anything is enqueued
        dummy += 1.0                                                # (so that the captured graph is not empty)
        rc = _raw(eng, tr, outs, 1, O=16, ext=1)
        msg = L.srtLastError()
    assert rc == -1 and b"capture" in msg and WHO.encode() in msg, (rc, msg)
    del graph
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)
    with torch.cuda.stream(side):
        assert _raw(eng, tr, outs, 1, O=16, ext=1) == 0, L.srtLastError()
        side.synchronize()
    for o in outs:
        assert torch.isfinite(o).all()
    # the older entry points keep their refusals
    args = (eng.h, 3, _p([a for a, _ in tr]), _p([b for _, b in tr]), (C.c_size_t * 3)(*ns), _p(outs))
    eng.set_wiener(1)
    assert L.srtSeparateBatch(*args) == -1 and b"Wiener" in L.srtLastError()
    assert L.srtSeparateBatchOverlap(*args, 16) == -1 and b"Wiener" in L.srtLastError()
    assert L.srtSeparateBatchMix(*args, 16, 0, None, 0) == -1 and b"Wiener" in L.srtLastError()
    eng.set_wiener(0)
    eng.set_overlap(8)
    assert L.srtSeparateBatchWiener(*args, 1) == -1 and b"overlap" in L.srtLastError()
    eng.set_overlap(0)
    eng.set_mask_extension("average")
    assert L.srtSeparateBatchWiener(*args, 1) == -1 and b"mask extension" in L.srtLastError()
    eng.set_mask_extension("constant")
    eng.set_mix([[1.0, 0.0, 0.0]])
    assert L.srtSeparateBatchWiener(*args, 1) == -1 and b"remix" in L.srtLastError()
    eng.set_mix(None)
    eng.close()


@pytest.mark.gpu
def test_python_splits_into_calls(oracle, coeffs):
    """separate_batch_wiener at a small max_tiles: several srtSeparateBatchWienerEx calls, each with its own tracks' matrices; the results equal the one-call
    results per track"""
    import torch
    from spleeterrt_amd import stream
    S, O = 2, 16
    ns = list(TRACKS) + [4096 * 9 + 11, 64 * 1024 * 2]
    _, total = _plan(ns, O)
    groups = stream.pack_tracks(ns, T_S, 4, O)
    assert len(groups) >= 3 and sum(g.ntiles for g in groups) == total
    tr = _tracks(oracle, ns, seed=2200)
    G = _per_track(S, len(tr), seed=17)
    kw = dict(iterations=2, overlap=O, mask_extension="average", mix=G)
    one = _engine(coeffs, S, max_tiles=total, batch_invariant=True)
    want = [o.clone() for o in one.separate_batch_wiener(tr, **kw)]
    one.close()
    eng = _engine(coeffs, S, max_tiles=4, batch_invariant=True)
    eng.set_timing(True)
    got = eng.separate_batch_wiener(tr, **kw)
    names = [n for n, _ in eng.get_timing()]
    eng.set_timing(False)
    for stage in ("stft_batch", "mask_ext", "wiener_filter_batch", "istft_batch"):
        assert names.count(stage) == len(groups), (stage, names)
    for k in range(len(tr)):
        assert torch.equal(got[k], want[k]), k
    eng.close()
