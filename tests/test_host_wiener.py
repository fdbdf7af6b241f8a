"""The Wiener filter over a host stream longer than max_tiles (srtSeparateHostWiener).  Every GPU test runs a small-max_tiles engine's
separate_host_wiener against separate_wiener of the whole signal on an engine large enough to hold it: the R tables, weight sums and a must be the same BITS
(a statistics chunk that straddles a piece boundary continues its partial sum in the slab), the stems agree within 2e-6 of the peak - the project's bound for the
overlap-add association at chunk seams (test_c4_stream, test_mask_extension::test_host_stream).

Geometries (T = 64, batch_invariant everywhere, so a tile's masks do not depend on the batch it ran in):
  rows = 225, F = 512, max_tiles 2 | 4:     rpc = 15, chunk 8 = rows [120, 135) straddles the seam at 128; the last piece (97 rows) is ragged
  rows = 4100, F = 64, max_tiles 8 | 65:    the 256-chunk clamp (rpc = 17, 242 chunks), no chunk boundary on a 512-row piece boundary
  rows = 16400, F = 64, max_tiles 1 | 257:  rpc = 65 > 64: pieces that lie wholly inside one chunk (piece 0 leaves chunk 0 unfinished, piece 64 is handed chunk 63)
  rows = 17000, F = 64, max_tiles 1 | 266:  rpc = 67: piece 22 = rows [1408, 1472) lies strictly inside chunk 21 = [1407, 1474) - continued and not finished"""
import ctypes as C

import numpy as np
import pytest

from test_mask_extension import _engine, _noisy_host, _timed
from test_pcm16 import rule
from test_wiener_opts import _opts

T_S = 64
N_225 = 225 * 1024 - 300
KARAOKE = np.array([[0.0, -1.0, 1.0]], np.float32)          # S = 2: the input minus stem 1
ONE_HOT = np.array([[0.0, 1.0, 0.0]], np.float32)


def _chunks(rows):
    """wiener_issue's rule: (rows per chunk, chunks)"""
    nch = min((rows + 15) // 16, 256)
    rpc = (rows + nch - 1) // nch
    return rpc, (rows + rpc - 1) // rpc


def _store_bytes(n, F, T, S):
    """the issue's formula: 2 * 2052 * 8 bytes of spectrum per row, n_stems * 2 * F * 4 bytes of masks per row of whole tiles"""
    rows = (n + 1023) // 1024
    return rows * 2 * 2052 * 8 + ((rows + T - 1) // T) * T * S * 2 * F * 4


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_the_geometries_are_what_the_docstring_says():
    assert _chunks(225) == (15, 15) and 8 * 15 < 128 < 9 * 15 and 225 - 128 == 97
    rpc, nch = _chunks(4100)
    assert (rpc, nch) == (17, 242) and all((p * 512) % 17 for p in range(1, 9))
    inside = lambda rpc, p: [c for c in (p * 64 // rpc,) if c * rpc <= p * 64 and (p + 1) * 64 <= (c + 1) * rpc]      # noqa: E731
    assert _chunks(16400)[0] == 65 and inside(65, 0) == [0] and inside(65, 64) == [63] and 63 * 65 < 64 * 64
    assert _chunks(17000)[0] == 67 and inside(67, 22) == [21] and 21 * 67 < 22 * 64 and 23 * 64 < 22 * 67


@pytest.mark.parametrize("F,T,S,max_tiles,n", [
    (1024, 256, 4, 64, 44100 * 600), (512, 64, 2, 2, N_225), (64, 64, 2, 1, 16400 * 1024), (64, 64, 2, 257, 16400 * 1024), (1536, 128, 5, 3, 4096), (2048, 64, 8, 7, 1000001)])
def test_host_wiener_bytes(F, T, S, max_tiles, n):
    """the store's size is the formula's, whatever max_tiles cuts the stream into (the tile padding is per stream, a piece being whole tiles)"""
    from spleeterrt_amd import capi
    assert capi.host_wiener_bytes(n, F, T, S, max_tiles) == _store_bytes(n, F, T, S)


def test_host_wiener_bytes_is_zero_below_one_frame_and_for_a_bad_config():
    from spleeterrt_amd import capi
    L = capi.load_library()
    cfg = capi._Config()
    cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles = 512, 64, 2, 2
    for n in (0, 1, 4095):
        assert L.srtHostWienerBytes(C.byref(cfg), n) == 0 and b"srtHostWienerBytes" in L.srtLastError() and b"4096" in L.srtLastError()
    assert L.srtHostWienerBytes(C.byref(cfg), 4096) == _store_bytes(4096, 512, 64, 2)
    for field, bad in (("F", 500), ("T", 0), ("n_stems", 9), ("max_tiles", 0)):
        c2 = capi._Config()
        c2.F, c2.T, c2.n_stems, c2.max_tiles = 512, 64, 2, 2
        setattr(c2, field, bad)
        assert L.srtHostWienerBytes(C.byref(c2), N_225) == 0 and b"srtHostWienerBytes" in L.srtLastError(), field
    assert L.srtHostWienerBytes(None, N_225) == 0
    with pytest.raises(capi.EngineError, match="4096"):
        capi.host_wiener_bytes(4095, 512, 64, 2, 2)


class _Stub:
    """stands in for an Engine: any library call is a failure of the test"""
    S, T = 2, 64

    def __getattr__(self, name):
        raise AssertionError("the argument checks must raise before %r is touched" % name)


@pytest.mark.parametrize("kw,match", [
    (dict(overlap=16), "overlap"),
    (dict(overlap=-1), "overlap"),
    (dict(overlap="x"), "overlap"),
    (dict(iterations=0), "iterations"),
    (dict(iterations=4), "iterations"),
    (dict(mask_extension="zeros"), "mask_extension"),
    (dict(mask_extension=2), "mask_extension"),
    (dict(mix=np.zeros((3, 3))), r"\[n_out, n_stems \+ 1\]"),              # n_out > n_stems
    (dict(mix=np.zeros((1, 2))), r"\[n_out, n_stems \+ 1\]"),
    (dict(mix=[[1.0, float("inf"), 0.0]]), "finite"),
])
def test_binding_refuses_bad_options_before_any_call(kw, match):
    from spleeterrt_amd.capi import Engine, EngineError
    with pytest.raises(EngineError, match=match):
        Engine.separate_host_wiener(_Stub(), None, **kw)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _signal(n, seed):
    """two tones plus white noise, different per channel, peak below 1: made without the oracle's transform, for the long geometries"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float32)
    L = (0.2 * np.sin(t * np.float32(0.031)) + 0.15 * rng.standard_normal(n)).astype(np.float32)
    R = (0.2 * np.sin(t * np.float32(0.047)) + 0.15 * rng.standard_normal(n)).astype(np.float32)
    return L, R


def _covs(eng, S, iters):
    return [eng.wiener_cov(j, it) for j in range(S) for it in range(1, iters + 1)]


def _same_covs(got, want):
    for (Ra, wa, aa), (Rb, wb, ab) in zip(got, want):
        assert np.array_equal(Ra, Rb) and np.array_equal(wa, wb) and aa == ab


def _reference(coeffs, L, R, F, max_tiles, iters, S=2, **kw):
    """separate_wiener of the whole signal on an engine that holds it -> (stems, [(R, weight sums, a)])"""
    import torch
    big = _engine(coeffs, S=S, F=F, max_tiles=max_tiles, batch_invariant=True)
    ref = big.separate_wiener(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), iters, **kw).cpu().numpy()
    covs = _covs(big, S, iters)
    big.close()
    return ref, covs


def _within(got, ref, tag):
    assert got.shape == ref.shape and np.isfinite(got).all()
    peak = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("%s: max-abs / peak = %.3g" % (tag, err / peak))
    assert err <= 2e-6 * peak, (tag, err / peak)


_REF225 = {}


def _ref225(oracle, coeffs, iters=1, **kw):
    """the rows = 225 clip and its whole-signal reference per option set, computed once"""
    L, R = _noisy_host(oracle, N_225, 71, 512)
    key = (iters, kw.get("mask_extension", "constant"), None if kw.get("mix") is None else kw["mix"].tobytes())
    if key not in _REF225:
        _REF225[key] = _reference(coeffs, L, R, 512, 4, iters, **kw)
    return (L, R) + _REF225[key]


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_a_chunk_split_over_two_pieces(oracle, coeffs, iters):
    """rows = 225 on max_tiles = 2 (pieces of 128 and 97 rows): chunk 8 is begun by piece 0 and finished by piece 1"""
    L, R, ref, covs = _ref225(oracle, coeffs, iters)
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    (got, clipped), ks = _timed(eng, lambda: eng.separate_host_wiener((L, R), iters))
    _same_covs(_covs(eng, 2, iters), covs)
    _within(got, ref, "rows 225 iters %d" % iters)
    assert clipped.tolist() == [0, 0]
    stats = [k for n, k in ks if n == "wiener_stats"]
    assert stats == ["srt_wiener_stats_seg_kernel"] * (2 * iters), ks
    assert [k for n, k in ks if n == "wiener_cov"] == ["srt_wiener_finalize_kernel"] * iters, ks
    assert [k for n, k in ks if n == "wiener_filter"] == ["srt_wiener_filter_kernel"] * 2, ks
    assert sum(n == "stft" for n, _ in ks) == 2 and sum(n == "istft" for n, _ in ks) == 4, ks      # the networks and the transforms run once per piece
    assert eng.host_wiener_bytes(N_225) == _store_bytes(N_225, 512, T_S, 2)
    eng.close()


@pytest.mark.gpu
def test_the_chunk_clamp(coeffs):
    """rows = 4100: 242 chunks of 17 rows over nine pieces of 512 rows (the last: 4 rows), two iterations"""
    n = 4100 * 1024
    L, R = _signal(n, 72)
    ref, covs = _reference(coeffs, L, R, 64, 65, 2)
    eng = _engine(coeffs, S=2, F=64, max_tiles=8, batch_invariant=True)
    got, _ = eng.separate_host_wiener((L, R), 2)
    _same_covs(_covs(eng, 2, 2), covs)
    _within(got, ref, "rows 4100")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [16400, 17000])
def test_pieces_inside_one_chunk(coeffs, rows):
    """max_tiles = 1: chunks of 65 (67) rows over 64-row pieces, so a piece can lie inside one chunk - beginning it and leaving it open, finishing one it was
    handed, or (rows = 17000) neither"""
    n = rows * 1024
    L, R = _signal(n, 73)
    ref, covs = _reference(coeffs, L, R, 64, (rows + 63) // 64, 1)
    eng = _engine(coeffs, S=2, F=64, max_tiles=1, batch_invariant=True)
    got, _ = eng.separate_host_wiener((L, R), 1)
    _same_covs(_covs(eng, 2, 1), covs)
    _within(got, ref, "rows %d" % rows)
    eng.close()


@pytest.mark.gpu
def test_options(oracle, coeffs):
    """the average extension, a karaoke row and a one-hot row on the rows = 225 geometry, each against separate_wiener under the same options; the one-hot row
    gives the bits of that stem's plane of the same engine's all-stem call through the same (option) kernel; a mix writes n_out planes and nothing else"""
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    L, R, ref, covs = _ref225(oracle, coeffs, 1, mask_extension="average")
    (stems, _), ks = _timed(eng, lambda: eng.separate_host_wiener((L, R), 1, mask_extension="average"))
    assert [k for n, k in ks if n == "wiener_filter"] == ["srt_wiener_filter_opt_kernel<false>"] * 2, ks
    assert sum(n == "mask_ext" for n, _ in ks) == 2, ks
    _same_covs(_covs(eng, 2, 1), covs)
    _within(stems, ref, "average")
    plain = _ref225(oracle, coeffs, 1)[2]
    assert np.abs(stems - plain).max() > 1e-3 * np.abs(plain).max()          # the constant rule is far away: the bound above is not vacuous
    for name, G in (("karaoke", KARAOKE), ("one-hot", ONE_HOT)):
        _, _, ref, _ = _ref225(oracle, coeffs, 1, mask_extension="average", mix=G)
        out = np.full((3, 2, ref.shape[2]), np.nan, np.float32)             # oversized: planes 1 and 2 must stay as they are
        got, _ = eng.separate_host_wiener((L, R), 1, mask_extension="average", mix=G, out=out[:1])
        assert got.shape == (1, 2, ref.shape[2]) and np.isnan(out[1:]).all()
        _within(out[:1], ref, name)
        if name == "one-hot":
            assert np.array_equal(out[0], stems[1])
    eng.close()


@pytest.mark.gpu
def test_a_signal_that_fits_is_separate_wiener(oracle, coeffs):
    """one piece: the same engine's separate_wiener, bit for bit, R tables included"""
    import torch
    L, R = _noisy_host(oracle, N_225, 71, 512)
    eng = _engine(coeffs, S=2, F=512, max_tiles=4, batch_invariant=True)
    for iters in (1, 2):
        want = eng.separate_wiener(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), iters).cpu().numpy()
        covs = _covs(eng, 2, iters)
        (got, _), ks = _timed(eng, lambda: eng.separate_host_wiener((L, R), iters))
        assert [k for n, k in ks if n == "wiener_stats"] == ["srt_wiener_stats_seg_kernel"] * iters, ks
        _same_covs(_covs(eng, 2, iters), covs)
        assert np.array_equal(got, want)
    eng.close()


@pytest.mark.gpu
def test_pcm16_io(oracle, coeffs):
    """both flags: the 16-bit input is the float call on its unpacked samples, the 16-bit output the float call's output under srtPcm16Pack's rule, and the
    clipped counts are numpy's"""
    L, R = _noisy_host(oracle, N_225, 71, 512)
    s = np.float32(1.05 / max(np.abs(L).max(), np.abs(R).max()))            # the loudest input samples clip at 16 bits
    (qL, cL), (qR, cR) = rule(L * s), rule(R * s)
    assert cL.sum() + cR.sum() > 0
    q = np.ascontiguousarray(np.stack([qL, qR], 1))
    Lq, Rq = qL.astype(np.float32) / np.float32(32768), qR.astype(np.float32) / np.float32(32768)
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    want, zero = eng.separate_host_wiener((Lq, Rq), 1)
    assert zero.tolist() == [0, 0]
    f_in16, _ = eng.separate_host_wiener(q, 1)
    assert np.array_equal(f_in16, want)

    def packed(x):
        wq, wc = rule(x)
        return np.ascontiguousarray(wq.transpose(0, 2, 1)), wc.sum(axis=(1, 2)).tolist()
    wq, wclip = packed(want)
    for src in ((Lq, Rq), q):                                               # the out flag alone, then both flags
        out, clipped = eng.separate_host_wiener(src, 1, out_pcm16=True)
        assert out.dtype == np.int16 and out.shape == wq.shape and np.array_equal(out, wq)
        assert clipped.tolist() == wclip
    # float input three times as loud (16-bit input cannot be): output samples past full scale
    L3, R3 = np.float32(3.0) * Lq, np.float32(3.0) * Rq
    want3, _ = eng.separate_host_wiener((L3, R3), 1)
    wq3, wclip3 = packed(want3)
    out3, clipped3 = eng.separate_host_wiener((L3, R3), 1, out_pcm16=True)
    print("clipped per stem:", wclip, wclip3)
    assert np.array_equal(out3, wq3) and clipped3.tolist() == wclip3 and sum(wclip3) > 0
    eng.close()


@pytest.mark.gpu
def test_engine_state_is_ignored_and_unchanged(oracle, coeffs):
    """the engine's srtSetWiener / srtSetOverlap / srtSetMix / srtSetMaskExtension at values other than the call's: the same bits, and every setting reads the same
    afterwards (the setters keep the filter apart from the mix and the extension, so two rounds)"""
    import torch
    import spleeterrt_amd as srt
    L, R = _noisy_host(oracle, N_225, 71, 512)
    Ld, Rd = torch.from_numpy(L[:100000]).cuda(), torch.from_numpy(R[:100000]).cuda()      # 98 rows: two tiles, back to back and at O = 16
    fresh = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    want, _ = fresh.separate_host_wiener((L, R), 2, mix=KARAOKE)
    want_cov = _covs(fresh, 2, 2)
    fresh.close()
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    # round 1: the filter on with another iteration count
    eng.set_wiener(3)
    before, ks_before = _timed(eng, lambda: eng.separate(Ld, Rd).clone())
    got, _ = eng.separate_host_wiener((L, R), 2, mix=KARAOKE)
    assert np.array_equal(got, want)
    _same_covs(_covs(eng, 2, 2), want_cov)
    after, ks_after = _timed(eng, lambda: eng.separate(Ld, Rd).clone())
    assert torch.equal(before, after) and ks_before == ks_after and sum(n == "wiener_stats" for n, _ in ks_after) == 3
    with pytest.raises(srt.EngineError, match="srtSeparateHostStream: the Wiener filter"):        # the streaming path keeps its refusal
        eng.separate_host_stream(L, R)
    eng.set_wiener(1)
    with pytest.raises(srt.EngineError, match="srtSeparateHostStream: the Wiener filter"):
        eng.separate_host_stream(L, R)
    eng.set_wiener(0)
    # round 2: overlap, another mix and the average extension on
    eng.set_overlap(16)
    eng.set_mix([[1.0, 1.0, 0.0], [0.0, 0.5, 0.25]])
    eng.set_mask_extension("average")
    before, ks_before = _timed(eng, lambda: eng.separate(Ld, Rd).clone())
    got, _ = eng.separate_host_wiener((L, R), 2, mix=KARAOKE)
    assert np.array_equal(got, want)
    after, ks_after = _timed(eng, lambda: eng.separate(Ld, Rd).clone())
    assert torch.equal(before, after) and ks_before == ks_after and before.shape[0] == 2
    assert (eng.mix_outputs, eng.overlap, eng.mask_extension) == (2, 16, 1)
    assert ks_after[0] == ("stft", "srt_stft_ov_kernel"), ks_after[0]         # the engine's overlap is still what its own calls run under
    eng.close()


def _raw(eng, L, R, n, out, flags=0, h_in2="R", **kw):
    """srtSeparateHostWiener itself on float buffers; returns the code"""
    o, _g = _opts(**kw)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)           # noqa: E731
    return eng.L.srtSeparateHostWiener(eng.h, p(L), p(R) if h_in2 == "R" else h_in2, n, C.byref(o), p(out), flags, None)


@pytest.mark.gpu
def test_refusals_and_cleanup(oracle, coeffs):
    """-1 (or -5) with a text that names the function, the NaN-prefilled output untouched, nothing launched; srtSeparateHostStream keeps refusing the engine's
    filter; the store comes back after release_staging"""
    import spleeterrt_amd as srt
    L, R = _noisy_host(oracle, N_225, 71, 512)
    bad = np.array([[1.0, np.inf, 0.0]], np.float32)

    def refused(eng, call, code, word=None):
        out = np.full((eng.S, 2, eng.L.srtIstftLength(225)), np.nan, np.float32)
        eng.set_timing(True)
        rc = call(out)
        launched = eng.get_timing()
        eng.set_timing(False)
        text = eng.L.srtLastError().decode()
        assert rc == code and "srtSeparateHostWiener" in text and (word is None or word in text), (rc, text)
        assert launched == [] and np.isnan(out).all(), (launched, text)

    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    for kw, word in ((dict(O=16), "overlap"), (dict(O=32), "overlap"), (dict(O=-1), "overlap"), (dict(iters=0), "iterations"), (dict(iters=4), "iterations"),
                     (dict(n_out=3), "n_stems spectra"), (dict(n_out=-1), "n_out"), (dict(n_out=1), "null gain"), (dict(G=bad), "finite"), (dict(ext=2), "mask_extension")):
        refused(eng, lambda out: _raw(eng, L, R, N_225, out, **kw), -1, word)
    refused(eng, lambda out: _raw(eng, L, R, 4095, out), -1, "4096")
    refused(eng, lambda out: _raw(eng, None, R, N_225, out), -1, "null")
    refused(eng, lambda out: _raw(eng, L, None, N_225, out), -1, "null")
    refused(eng, lambda out: eng.L.srtSeparateHostWiener(eng.h, C.c_void_p(L.ctypes.data), C.c_void_p(R.ctypes.data), N_225, None, C.c_void_p(out.ctypes.data), 0, None), -1, "null")
    assert _raw(eng, L, R, N_225, None) == -1 and b"srtSeparateHostWiener" in eng.L.srtLastError()
    refused(eng, lambda out: _raw(eng, L, R, N_225, out, flags=8), -1, "flag")
    refused(eng, lambda out: _raw(eng, L, R, N_225, out, flags=srt.capi.HOST_IN_PCM16), -1, "SRT_HOST_IN_PCM16")      # a second buffer with the interleaved form
    # the streaming path keeps its refusal of the engine's own filter
    eng.set_wiener(1)
    with pytest.raises(srt.EngineError, match="srtSeparateHostStream: the Wiener filter"):
        eng.separate_host_stream(L, R)
    eng.set_wiener(0)
    # release_staging frees the store; the next call allocates it again and gives the same bits
    first, _ = eng.separate_host_wiener((L, R), 1)
    eng.release_staging()
    second, _ = eng.separate_host_wiener((L, R), 1)
    assert np.array_equal(first, second) and np.isfinite(first).all()
    eng.release_staging()
    eng.close()
    rm = _engine(coeffs, S=2, F=512, max_tiles=2, ratio_mask=True)
    refused(rm, lambda out: _raw(rm, L, R, N_225, out), -1, "ratio_mask")
    rm.close()
    bare = srt.Engine(F=512, T=T_S, stem_modes=(1, 0), max_tiles=2)           # no weights
    refused(bare, lambda out: _raw(bare, L, R, N_225, out), -5, "weights")
    bare.close()
