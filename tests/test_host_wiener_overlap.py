"""The Wiener filter on overlapped tiles over a host stream longer than max_tiles (srtSeparateHostWienerOverlap).  Every GPU test runs a
small-max_tiles engine's separate_host_wiener_overlap against separate_wiener(..., overlap=O) of the whole signal on an engine that holds it: the R tables, weight
sums and a must be the same BITS (a row enters the statistics once, with the blended mask of the whole-signal call, in that call's summation order), the stems
agree within 2e-6 of the peak - the project's bound for the overlap-add association at piece seams (test_c4_stream, test_host_wiener, test_host_overlap).

Geometries (T = 64, batch_invariant everywhere, so a tile's masks do not depend on the batch it ran in; S = T - O):
  1  rows = 225, F = 512, O = 16, max_tiles 2 | 5:   pieces own [0,96), [96,192), [192,225) and analyse 112, 112, 33 rows; rpc = 15: chunk 6 = [90,105) and
                                                     chunk 12 = [180,195) straddle both seams; the last piece is one ragged tile
  2  the same at O = 32 (T/2), max_tiles 2 | 7:      four pieces, seams at 64, 128, 192, every one inside a chunk
  3  the same at O = 16, max_tiles 1 | 5:            five pieces, every tile boundary a piece seam
  4  rows = 16400, F = 64, O = 16, max_tiles 1 | 342: rpc = 65 > the 48 rows a piece owns: 84 pieces strictly inside one chunk, 336 of 341 seams inside a chunk
  5  rows = 4100, F = 64, O = 16, max_tiles 8 | 86:  11 pieces, 242 chunks of 17 rows, 10 of 10 seams inside a chunk
  6  rows = 250, F = 64, O = 16, max_tiles 1 | 5:    the last piece owns rows [192, 250): 58, more than the 48 a full piece owns (its tile has no successor)"""
import ctypes as C

import numpy as np
import pytest

from test_host_wiener import KARAOKE, N_225, ONE_HOT, T_S, _chunks, _covs, _same_covs, _signal, _store_bytes, _within
from test_mask_extension import _engine, _noisy_host, _timed
from test_pcm16 import rule
from test_wiener_opts import _opts

SPEC_ROW = 2 * 2052 * 8                                     # bytes of one spectrum row: two channels of 2052 complex floats


def _pieces(rows, O, max_tiles):
    from spleeterrt_amd import stream
    return stream.host_overlap_pieces(rows, T_S, O, max_tiles)


def _ov_store_bytes(n, F, T, S, max_tiles, O):
    """the documented formula, piece by piece: spectrum of the rows a piece analyses, masks of its tiles, one carry per piece boundary"""
    from spleeterrt_amd import stream
    pcs = stream.host_overlap_pieces((n + 1023) // 1024, T, O, max_tiles)
    return sum(p["stft_rows"] * SPEC_ROW + S * p["tiles"] * 2 * T * F * 4 for p in pcs) + (len(pcs) - 1) * S * 2 * O * F * 4


def _seams_inside_a_chunk(rows, O, max_tiles):
    rpc, _ = _chunks(rows)
    return [p["row0"] for p in _pieces(rows, O, max_tiles)[1:] if p["row0"] % rpc]


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_the_geometries_are_what_the_docstring_says():
    own = lambda rows, O, P: [(p["row0"], p["row0"] + p["own_rows"]) for p in _pieces(rows, O, P)]      # noqa: E731
    assert own(225, 16, 2) == [(0, 96), (96, 192), (192, 225)] and [p["stft_rows"] for p in _pieces(225, 16, 2)] == [112, 112, 33]
    assert _pieces(225, 16, 2)[-1]["tiles"] == 1 and len(_pieces(225, 16, 5)) == 1 and len(_pieces(225, 16, 4)) == 2
    assert _chunks(225) == (15, 15) and 6 * 15 < 96 < 7 * 15 and 12 * 15 < 192 < 13 * 15
    assert [a for a, _ in own(225, 32, 2)] == [0, 64, 128, 192] and _seams_inside_a_chunk(225, 32, 2) == [64, 128, 192]
    assert len(_pieces(225, 32, 7)) == 1 and len(_pieces(225, 32, 6)) == 2
    assert len(_pieces(225, 16, 1)) == 5 and all(p["tiles"] == 1 for p in _pieces(225, 16, 1))
    rpc, _ = _chunks(16400)
    pcs = _pieces(16400, 16, 1)
    inside = [p for p in pcs if p["row0"] // rpc * rpc < p["row0"] and p["row0"] + p["own_rows"] < (p["row0"] // rpc + 1) * rpc]
    assert rpc == 65 and len(pcs) == 342 and pcs[0]["own_rows"] == 48 and len(inside) == 84 and len(_seams_inside_a_chunk(16400, 16, 1)) == 336
    assert len(_pieces(16400, 16, 342)) == 1 and len(_pieces(16400, 16, 341)) == 2
    assert _chunks(4100) == (17, 242) and len(_pieces(4100, 16, 8)) == 11 and len(_seams_inside_a_chunk(4100, 16, 8)) == 10
    assert len(_pieces(4100, 16, 86)) == 1 and len(_pieces(4100, 16, 85)) == 2
    assert len(_pieces(300, 16, 8)) == 1
    assert own(250, 16, 1)[-1] == (192, 250) and own(250, 16, 1)[0] == (0, 48) and len(_pieces(250, 16, 5)) == 1 and len(_pieces(250, 16, 4)) == 2


def test_the_symbols_are_exported():
    from spleeterrt_amd import capi
    L = capi.load_library()
    for sym in ("srtSeparateHostWienerOverlap", "srtHostWienerOverlapBytes"):
        getattr(L, sym)
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "spleeterrt_amd.h")).read()
    assert "srtSeparateHostWienerOverlap(srt_engine *e" in header and "srtHostWienerOverlapBytes(const srt_config *cfg, size_t n, int overlap_rows)" in header


@pytest.mark.parametrize("F,T,S,max_tiles,n", [
    (1024, 256, 4, 64, 44100 * 600), (512, 64, 2, 2, N_225), (64, 64, 2, 1, 16400 * 1024), (1536, 128, 5, 3, 4096), (2048, 64, 8, 7, 1000001)])
def test_bytes_without_an_overlap_are_host_wiener_bytes(F, T, S, max_tiles, n):
    from spleeterrt_amd import capi
    assert capi.host_wiener_overlap_bytes(n, F, T, S, max_tiles, 0) == capi.host_wiener_bytes(n, F, T, S, max_tiles) == _store_bytes(n, F, T, S)


def test_bytes_are_the_formula_over_a_grid():
    """piece by piece, and in closed form: (rows + (pieces - 1) O) spectrum rows, the masks of all N tiles, pieces - 1 carries"""
    from spleeterrt_amd import capi, stream
    F, S = 128, 3
    for rows in (4, 63, 64, 65, 112, 113, 225, 1000, 4100):
        n = max(4096, rows * 1024 - 17)
        rows = (n + 1023) // 1024
        for O in (0, 1, 16, 31, 32):
            for P in (1, 2, 3, 8, 100):
                got = capi.host_wiener_overlap_bytes(n, F, T_S, S, P, O)
                N = stream.overlap_tiles(rows, T_S, O)
                npieces = (N + P - 1) // P
                closed = (rows + (npieces - 1) * O) * SPEC_ROW + N * S * 2 * T_S * F * 4 + (npieces - 1) * S * 2 * O * F * 4
                assert got == _ov_store_bytes(n, F, T_S, S, P, O) == closed, (rows, O, P)


@pytest.mark.parametrize("O", [16, 32])
def test_bytes_grow_with_the_piece_count(O):
    """fewer tiles per piece: more pieces, each boundary paying O look-ahead rows and one carry"""
    from spleeterrt_amd import capi
    n, last = 4100 * 1024, None
    for P in (86, 43, 20, 8, 3, 2, 1):
        cur = (len(_pieces(4100, O, P)), capi.host_wiener_overlap_bytes(n, 64, T_S, 2, P, O))
        if last is not None:
            assert cur[0] > last[0] and cur[1] - last[1] == (cur[0] - last[0]) * (O * SPEC_ROW + 2 * 2 * O * 64 * 4), (P, cur, last)
        last = cur


def test_bytes_refusals():
    from spleeterrt_amd import capi
    L = capi.load_library()
    cfg = capi._Config()
    cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles = 512, 64, 2, 2
    assert L.srtHostWienerOverlapBytes(None, N_225, 16) == 0 and b"srtHostWienerOverlapBytes" in L.srtLastError() and b"null" in L.srtLastError()
    for field, bad in (("F", 500), ("T", 0), ("n_stems", 9), ("max_tiles", 0)):
        c2 = capi._Config()
        c2.F, c2.T, c2.n_stems, c2.max_tiles = 512, 64, 2, 2
        setattr(c2, field, bad)
        assert L.srtHostWienerOverlapBytes(C.byref(c2), N_225, 16) == 0 and b"srtHostWienerOverlapBytes" in L.srtLastError(), field
    for n in (0, 4095):
        assert L.srtHostWienerOverlapBytes(C.byref(cfg), n, 16) == 0 and b"srtHostWienerOverlapBytes" in L.srtLastError() and b"4096" in L.srtLastError()
    for O in (-1, 33, 64):
        assert L.srtHostWienerOverlapBytes(C.byref(cfg), N_225, O) == 0 and b"srtHostWienerOverlapBytes" in L.srtLastError() and b"overlap" in L.srtLastError()
    assert L.srtHostWienerOverlapBytes(C.byref(cfg), N_225, 32) == _ov_store_bytes(N_225, 512, 64, 2, 2, 32)
    with pytest.raises(capi.EngineError, match="overlap"):
        capi.host_wiener_overlap_bytes(N_225, 512, 64, 2, 2, 33)


class _Stub:
    """stands in for an Engine: any library call is a failure of the test"""
    S, T = 2, 64

    def __getattr__(self, name):
        raise AssertionError("the argument checks must raise before %r is touched" % name)


@pytest.mark.parametrize("kw,match", [
    (dict(overlap=33), "overlap"),
    (dict(overlap=-1), "overlap"),
    (dict(overlap="x"), "overlap"),
    (dict(overlap=16.5), "overlap"),
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
    kw.setdefault("overlap", 16)
    with pytest.raises(EngineError, match=match):
        Engine.separate_host_wiener_overlap(_Stub(), None, **kw)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _reference(coeffs, L, R, F, max_tiles, iters, O, ext_rows=None, **kw):
    """separate_wiener(overlap=O) of the whole signal on an engine that holds it -> (stems, [(R, weight sums, a)], the extension's gain tables or None)"""
    import torch
    big = _engine(coeffs, S=2, F=F, max_tiles=max_tiles, batch_invariant=True)
    ref = big.separate_wiener(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), iters, overlap=O, **kw).cpu().numpy()
    covs = _covs(big, 2, iters)
    ext = [big.mask_ext(j, ext_rows) for j in range(2)] if ext_rows else None
    big.close()
    return ref, covs, ext


_REF225 = {}


def _ref225(oracle, coeffs, O=16, iters=1, **kw):
    """the rows = 225 clip and its whole-signal reference per option set, computed once and never written to"""
    L, R = _noisy_host(oracle, N_225, 71, 512)
    ext = kw.get("mask_extension", "constant")
    key = (O, iters, ext, None if kw.get("mix") is None else kw["mix"].tobytes())
    if key not in _REF225:
        _REF225[key] = _reference(coeffs, L, R, 512, {16: 5, 32: 7}[O], iters, O, ext_rows=225 if ext == "average" else None, **kw)
    return (L, R) + _REF225[key]


def _names(ks, name):
    return [k for n, k in ks if n == name]


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_chunks_split_over_three_pieces(oracle, coeffs, iters):
    """geometry 1: chunks 6 and 12 are begun by one piece and finished by the next; the first 16 rows of pieces 1 and 2 blend with the carry"""
    L, R, ref, covs, _ = _ref225(oracle, coeffs, 16, iters)
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    (got, clipped), ks = _timed(eng, lambda: eng.separate_host_wiener_overlap((L, R), 16, iters))
    _same_covs(_covs(eng, 2, iters), covs)
    _within(got, ref, "rows 225 O 16 iters %d" % iters)
    assert clipped.tolist() == [0, 0]
    assert _names(ks, "wiener_stats") == ["srt_wiener_stats_seg_ov_kernel"] * (3 * iters), ks
    assert _names(ks, "wiener_cov") == ["srt_wiener_finalize_kernel"] * iters, ks
    assert _names(ks, "wiener_filter") == ["srt_wiener_filter_opt_kernel<true>"] + ["srt_wiener_filter_seam_kernel"] * 2, ks
    assert len(_names(ks, "mask_seam")) == 2 and all(k.startswith("srt_mask_seam_save_kernel") for k in _names(ks, "mask_seam")), ks
    assert _names(ks, "stft") == ["srt_stft_ov_kernel"] * 3 and len(_names(ks, "istft")) == 6, ks      # the networks and the transforms run once per piece
    assert eng.host_wiener_overlap_bytes(N_225, 16) == _ov_store_bytes(N_225, 512, T_S, 2, 2, 16)
    eng.close()


@pytest.mark.gpu
def test_half_a_tile_of_overlap(oracle, coeffs):
    """geometry 2: O = T / 2, four pieces, every row of a later piece's first tile half is a seam row"""
    L, R, ref, covs, _ = _ref225(oracle, coeffs, 32, 2)
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    got, _ = eng.separate_host_wiener_overlap((L, R), 32, 2)
    _same_covs(_covs(eng, 2, 2), covs)
    _within(got, ref, "rows 225 O 32")
    eng.close()


@pytest.mark.gpu
def test_one_tile_per_piece(oracle, coeffs):
    """geometry 3: max_tiles = 1 - no blend happens inside a piece, every one goes through the carry"""
    L, R, ref, covs, _ = _ref225(oracle, coeffs, 16, 1)
    eng = _engine(coeffs, S=2, F=512, max_tiles=1, batch_invariant=True)
    (got, _), ks = _timed(eng, lambda: eng.separate_host_wiener_overlap((L, R), 16, 1))
    assert len(_names(ks, "wiener_stats")) == 5 and len(_names(ks, "mask_seam")) == 4, ks
    _same_covs(_covs(eng, 2, 1), covs)
    _within(got, ref, "rows 225 O 16 max_tiles 1")
    eng.close()


@pytest.mark.gpu
def test_pieces_inside_one_chunk(coeffs):
    """geometry 4: 342 one-tile pieces of 48 owned rows under chunks of 65 rows, two iterations"""
    n = 16400 * 1024
    L, R = _signal(n, 73)
    ref, covs, _ = _reference(coeffs, L, R, 64, 342, 2, 16)
    eng = _engine(coeffs, S=2, F=64, max_tiles=1, batch_invariant=True)
    got, _ = eng.separate_host_wiener_overlap((L, R), 16, 2)
    _same_covs(_covs(eng, 2, 2), covs)
    _within(got, ref, "rows 16400 O 16")
    eng.close()


@pytest.mark.gpu
def test_the_chunk_clamp(coeffs):
    """geometry 5: 242 chunks of 17 rows over eleven pieces of 384 owned rows, two iterations"""
    n = 4100 * 1024
    L, R = _signal(n, 72)
    ref, covs, _ = _reference(coeffs, L, R, 64, 86, 2, 16)
    eng = _engine(coeffs, S=2, F=64, max_tiles=8, batch_invariant=True)
    got, _ = eng.separate_host_wiener_overlap((L, R), 16, 2)
    _same_covs(_covs(eng, 2, 2), covs)
    _within(got, ref, "rows 4100 O 16")
    eng.close()


@pytest.mark.gpu
def test_a_last_piece_that_owns_more_rows_than_a_full_one(coeffs):
    """geometry 6: every staging buffer and workspace has to hold the (max_tiles - 1) S + T rows the last piece may own, not the max_tiles S of a full piece"""
    n = 250 * 1024
    L, R = _signal(n, 75)
    ref, covs, _ = _reference(coeffs, L, R, 64, 5, 2, 16)
    eng = _engine(coeffs, S=2, F=64, max_tiles=1, batch_invariant=True)
    for out_pcm16 in (False, True):                                         # the 16-bit staging is sized from the same row count
        got, _ = eng.separate_host_wiener_overlap((L, R), 16, 2, out_pcm16=out_pcm16)
        _same_covs(_covs(eng, 2, 2), covs)
        if out_pcm16:
            assert np.array_equal(got, np.ascontiguousarray(rule(ref_f)[0].transpose(0, 2, 1)))
        else:
            _within(got, ref, "rows 250 O 16 max_tiles 1")
            ref_f = got
    eng.close()


@pytest.mark.gpu
def test_options(oracle, coeffs):
    """the average extension (its gain table of the last piece included), a karaoke row and a one-hot row on geometry 1, each against separate_wiener under the
    same options; the one-hot row gives the bits of that stem's plane of the same call path; a mix writes n_out planes and nothing else"""
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    L, R, ref, covs, ext = _ref225(oracle, coeffs, 16, 1, mask_extension="average")
    (stems, _), ks = _timed(eng, lambda: eng.separate_host_wiener_overlap((L, R), 16, 1, mask_extension="average"))
    assert _names(ks, "mask_ext") == ["srt_mask_ext_kernel<false, false, true>"] + ["srt_mask_ext_seam_kernel<false>"] * 2, ks
    _same_covs(_covs(eng, 2, 1), covs)
    for j in range(2):                                                      # the table holds the LAST piece's owned rows [192, 225), 16 of them seam rows
        assert np.array_equal(eng.mask_ext(j, 33), ext[j][192:225]), j
    _within(stems, ref, "average")
    plain = _ref225(oracle, coeffs, 16, 1)[2]
    assert np.abs(stems - plain).max() > 1e-3 * np.abs(plain).max()          # the constant rule is far away: the bound above is not vacuous
    for name, G in (("karaoke", KARAOKE), ("one-hot", ONE_HOT)):
        ref = _ref225(oracle, coeffs, 16, 1, mask_extension="average", mix=G)[2]
        out = np.full((3, 2, ref.shape[2]), np.nan, np.float32)             # oversized: planes 1 and 2 must stay as they are
        got, _ = eng.separate_host_wiener_overlap((L, R), 16, 1, mask_extension="average", mix=G, out=out[:1])
        assert got.shape == (1, 2, ref.shape[2]) and np.isnan(out[1:]).all()
        _within(out[:1], ref, name)
        if name == "one-hot":
            assert np.array_equal(out[0], stems[1])
    eng.close()


@pytest.mark.gpu
def test_a_signal_of_one_piece(coeffs):
    """rows = 300 on max_tiles = 8: at O = 16 the same engine's separate_wiener, bit for bit, R tables included; at O = 0 separate_host_wiener's bits and launches"""
    import torch
    n = 300 * 1024
    L, R = _signal(n, 74)
    eng = _engine(coeffs, S=2, F=64, max_tiles=8, batch_invariant=True)
    for iters in (1, 2):
        want = eng.separate_wiener(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), iters, overlap=16).cpu().numpy()
        covs = _covs(eng, 2, iters)
        got, _ = eng.separate_host_wiener_overlap((L, R), 16, iters)
        _same_covs(_covs(eng, 2, iters), covs)
        assert np.array_equal(got, want)
    (want, _), ks_want = _timed(eng, lambda: eng.separate_host_wiener((L, R), 2))
    covs = _covs(eng, 2, 2)
    (got, _), ks_got = _timed(eng, lambda: eng.separate_host_wiener_overlap((L, R), 0, 2))
    _same_covs(_covs(eng, 2, 2), covs)
    assert np.array_equal(got, want) and ks_got == ks_want and "srt_wiener_stats_seg_kernel" in _names(ks_got, "wiener_stats"), ks_got
    eng.close()


@pytest.mark.gpu
def test_without_an_overlap_it_is_host_wiener_and_with_one_it_is_not(oracle, coeffs):
    """geometry 1 at O = 0: separate_host_wiener's launches and bits over two pieces.  And the O = 16 result is far from it - the masks do vary across tiles, so
    the comparisons with the whole-signal call are not passed by masks that a missing blend would leave unchanged"""
    L, R, ref, _, _ = _ref225(oracle, coeffs, 16, 1)
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    (want, _), ks_want = _timed(eng, lambda: eng.separate_host_wiener((L, R), 1))
    covs = _covs(eng, 2, 1)
    (got, _), ks_got = _timed(eng, lambda: eng.separate_host_wiener_overlap((L, R), 0, 1))
    _same_covs(_covs(eng, 2, 1), covs)
    assert np.array_equal(got, want) and ks_got == ks_want
    ov, _ = eng.separate_host_wiener_overlap((L, R), 16, 1)
    peak = float(np.abs(ref).max())
    d = float(np.abs(ov - want).max()) / peak
    print("O = 16 against O = 0: max-abs / peak = %.3g" % d)
    assert d > 2e-6
    eng.close()


@pytest.mark.gpu
def test_pcm16_io(oracle, coeffs):
    """both flags on geometry 1: the 16-bit input is the float call on its unpacked samples, the 16-bit output the float call's output under srtPcm16Pack's rule,
    and the clipped counts are numpy's"""
    L, R = _noisy_host(oracle, N_225, 71, 512)
    s = np.float32(1.05 / max(np.abs(L).max(), np.abs(R).max()))            # the loudest input samples clip at 16 bits
    (qL, cL), (qR, cR) = rule(L * s), rule(R * s)
    assert cL.sum() + cR.sum() > 0
    q = np.ascontiguousarray(np.stack([qL, qR], 1))
    Lq, Rq = qL.astype(np.float32) / np.float32(32768), qR.astype(np.float32) / np.float32(32768)
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    want, zero = eng.separate_host_wiener_overlap((Lq, Rq), 16, 1)
    assert zero.tolist() == [0, 0]
    f_in16, _ = eng.separate_host_wiener_overlap(q, 16, 1)
    assert np.array_equal(f_in16, want)

    def packed(x):
        wq, wc = rule(x)
        return np.ascontiguousarray(wq.transpose(0, 2, 1)), wc.sum(axis=(1, 2)).tolist()
    wq, wclip = packed(want)
    for src in ((Lq, Rq), q):                                               # the out flag alone, then both flags
        out, clipped = eng.separate_host_wiener_overlap(src, 16, 1, out_pcm16=True)
        assert out.dtype == np.int16 and out.shape == wq.shape and np.array_equal(out, wq)
        assert clipped.tolist() == wclip
    # float input three times as loud (16-bit input cannot be): output samples past full scale
    L3, R3 = np.float32(3.0) * Lq, np.float32(3.0) * Rq
    want3, _ = eng.separate_host_wiener_overlap((L3, R3), 16, 1)
    wq3, wclip3 = packed(want3)
    out3, clipped3 = eng.separate_host_wiener_overlap((L3, R3), 16, 1, out_pcm16=True)
    print("clipped per stem:", wclip, wclip3)
    assert np.array_equal(out3, wq3) and clipped3.tolist() == wclip3 and sum(wclip3) > 0
    eng.close()


@pytest.mark.gpu
def test_engine_state_is_ignored_and_unchanged(oracle, coeffs):
    """the engine's srtSetWiener / srtSetOverlap / srtSetMix / srtSetMaskExtension at values other than the call's: the same bits, and every setting reads the same
    afterwards (the setters keep the filter apart from the mix and the extension, so two rounds)"""
    import torch
    L, R = _noisy_host(oracle, N_225, 71, 512)
    Ld, Rd = torch.from_numpy(L[:100000]).cuda(), torch.from_numpy(R[:100000]).cuda()      # 98 rows: two tiles, back to back and at O = 8
    fresh = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    want, _ = fresh.separate_host_wiener_overlap((L, R), 16, 2, mix=KARAOKE)
    want_cov = _covs(fresh, 2, 2)
    fresh.close()
    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    # round 1: the filter on with another iteration count
    eng.set_wiener(3)
    before, ks_before = _timed(eng, lambda: eng.separate(Ld, Rd).clone())
    got, _ = eng.separate_host_wiener_overlap((L, R), 16, 2, mix=KARAOKE)
    assert np.array_equal(got, want)
    _same_covs(_covs(eng, 2, 2), want_cov)
    after, ks_after = _timed(eng, lambda: eng.separate(Ld, Rd).clone())
    assert torch.equal(before, after) and ks_before == ks_after and sum(n == "wiener_stats" for n, _ in ks_after) == 3
    eng.set_wiener(0)
    # round 2: another overlap, another mix and the average extension on
    eng.set_overlap(8)
    eng.set_mix([[1.0, 1.0, 0.0], [0.0, 0.5, 0.25]])
    eng.set_mask_extension("average")
    before, ks_before = _timed(eng, lambda: eng.separate(Ld, Rd).clone())
    got, _ = eng.separate_host_wiener_overlap((L, R), 16, 2, mix=KARAOKE)
    assert np.array_equal(got, want)
    after, ks_after = _timed(eng, lambda: eng.separate(Ld, Rd).clone())
    assert torch.equal(before, after) and ks_before == ks_after and before.shape[0] == 2
    assert (eng.mix_outputs, eng.overlap, eng.mask_extension) == (2, 8, 1)
    assert ks_after[0] == ("stft", "srt_stft_ov_kernel"), ks_after[0]         # the engine's overlap is still what its own calls run under
    eng.close()


def _raw(eng, L, R, n, out, flags=0, h_in2="R", **kw):
    """srtSeparateHostWienerOverlap itself on float buffers; returns the code"""
    kw.setdefault("O", 16)
    o, _g = _opts(**kw)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)           # noqa: E731
    return eng.L.srtSeparateHostWienerOverlap(eng.h, p(L), p(R) if h_in2 == "R" else h_in2, n, C.byref(o), p(out), flags, None)


@pytest.mark.gpu
def test_refusals_and_cleanup(oracle, coeffs):
    """-1 (or -5) with a text that names the function, the NaN-prefilled output untouched, nothing launched; srtSeparateHostWiener keeps refusing an overlap;
    the store comes back after release_staging"""
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
        assert rc == code and "srtSeparateHostWienerOverlap" in text and (word is None or word in text), (rc, text)
        assert launched == [] and np.isnan(out).all(), (launched, text)

    eng = _engine(coeffs, S=2, F=512, max_tiles=2, batch_invariant=True)
    for kw, word in ((dict(O=33), "overlap"), (dict(O=64), "overlap"), (dict(O=-1), "overlap"), (dict(iters=0), "iterations"), (dict(iters=4), "iterations"),
                     (dict(n_out=3), "n_stems spectra"), (dict(n_out=-1), "n_out"), (dict(n_out=1), "null gain"), (dict(G=bad), "finite"), (dict(ext=2), "mask_extension")):
        refused(eng, lambda out: _raw(eng, L, R, N_225, out, **kw), -1, word)
    refused(eng, lambda out: _raw(eng, L, R, 4095, out), -1, "4096")
    refused(eng, lambda out: _raw(eng, None, R, N_225, out), -1, "null")
    refused(eng, lambda out: _raw(eng, L, None, N_225, out), -1, "null")
    refused(eng, lambda out: eng.L.srtSeparateHostWienerOverlap(eng.h, C.c_void_p(L.ctypes.data), C.c_void_p(R.ctypes.data), N_225, None, C.c_void_p(out.ctypes.data), 0, None), -1, "null")
    assert _raw(eng, L, R, N_225, None) == -1 and b"srtSeparateHostWienerOverlap" in eng.L.srtLastError()
    refused(eng, lambda out: _raw(eng, L, R, N_225, out, flags=8), -1, "flag")
    refused(eng, lambda out: _raw(eng, L, R, N_225, out, flags=srt.capi.HOST_IN_PCM16), -1, "SRT_HOST_IN_PCM16")      # a second buffer with the interleaved form
    with pytest.raises(srt.EngineError, match="overlap"):                   # the entry point without an overlap keeps its refusal
        eng.separate_host_wiener((L, R), 1, overlap=16)
    # release_staging frees the store and the carries in it; the next call allocates it again and gives the same bits
    first, _ = eng.separate_host_wiener_overlap((L, R), 16, 1)
    eng.release_staging()
    second, _ = eng.separate_host_wiener_overlap((L, R), 16, 1)
    assert np.array_equal(first, second) and np.isfinite(first).all()
    eng.release_staging()
    eng.close()
    rm = _engine(coeffs, S=2, F=512, max_tiles=2, ratio_mask=True)
    refused(rm, lambda out: _raw(rm, L, R, N_225, out), -1, "ratio_mask")
    rm.close()
    bare = srt.Engine(F=512, T=T_S, stem_modes=(1, 0), max_tiles=2)           # no weights
    refused(bare, lambda out: _raw(bare, L, R, N_225, out), -5, "weights")
    bare.close()
