"""Overlapped network tiles over a host stream of any length (srtSeparateHostStreamOverlap).

CPU: srtHostOverlapPieces against stream.host_overlap_pieces and a brute-force plan (ownership, tile partition, staging bounds, O = 0 is the present chunking),
bad arguments.  GPU (T = 64, the 277-row signal of tests/test_overlap.py, batch_invariant engines): the piece seams against srtSeparate under srtSetOverlap on an
engine that holds the signal (both inverse families, O = 16 and T/2, max_tiles = 1 and 3) at the project's seam bound of 2e-6 of the peak; the same comparison
on masks whose carry was lost, which must miss that bound by more than 50x; one piece = srtSeparate's bits; O = 0 = srtSeparateHostStreamIo's bits and
launches; ratio_mask, the average extension and a remix across seams; the fp16 mode; 16-bit I/O; the engine's own setting untouched; every refusal."""
import ctypes as C

import numpy as np
import pytest

from test_overlap import N_RAGGED, _audio, _blend_rows, _engine
from test_pcm16 import rule

T_S = 64
ROWS = 277
BOUND = 2e-6                      # of the peak: the chunked paths' seam bound (README "Streaming", tests/test_c4_stream.py)
SEED = 41


def _lib():
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def _brute_plan(rows, T, O, P):
    """every row goes to its primary tile (the last tile that starts at or before it, clamped), every tile to piece tile // P"""
    S = T - O
    nt = 0 if rows == 0 else 1
    while nt and (nt - 1) * S + T < rows:
        nt += 1
    owner = [min(r // S, nt - 1) // P for r in range(rows)]
    pieces = []
    for p in range((nt + P - 1) // P):
        tiles = [j for j in range(nt) if j // P == p]
        mine = [r for r in range(rows) if owner[r] == p]
        assert mine == list(range(mine[0], mine[-1] + 1))
        last_row = min(rows, tiles[-1] * S + T)                  # one past the last row any of its tiles covers
        pieces.append(dict(tile0=tiles[0], tiles=len(tiles), row0=mine[0], own_rows=len(mine), stft_rows=last_row - mine[0]))
    return pieces


def test_piece_plan_rule():
    from spleeterrt_amd import capi, stream
    rng = np.random.default_rng(17)
    for T in (64, 128, 256):
        for O in (0, 1, T // 4, T // 2):
            S = T - O
            for P in (1, 2, 3, 64):
                rows_set = [1, max(O, 1), T, T + 1, S + T, S + T + 1, P * S, P * S + O, P * S + O + 1, P * S + T, 2 * P * S + O + 1] + \
                           [int(x) for x in rng.integers(1, 9 * T, size=8)] + [int(x) for x in rng.integers(1, 3 * P * T + 2, size=4)]
                for rows in rows_set:
                    got = capi.host_overlap_pieces(rows, T, O, P)
                    assert got == stream.host_overlap_pieces(rows, T, O, P) == _brute_plan(rows, T, O, P), (rows, T, O, P, got)
                    N = stream.overlap_tiles(rows, T, O)
                    # tile ranges partition [0, N); every row is owned by exactly one piece
                    assert [p["tile0"] for p in got] == list(range(0, N, P)) and sum(p["tiles"] for p in got) == N
                    assert got[0]["row0"] == 0 and sum(p["own_rows"] for p in got) == rows
                    for a, b in zip(got, got[1:]):
                        assert a["row0"] + a["own_rows"] == b["row0"]
                    for p in got:
                        assert 1 <= p["tiles"] <= P and p["row0"] == p["tile0"] * S
                        assert p["own_rows"] <= p["stft_rows"] <= P * T, (rows, T, O, P, p)                 # the staging capacities hold
                        assert p["row0"] + p["stft_rows"] == min(rows, (p["tile0"] + p["tiles"] - 1) * S + T)      # covers the last tile's rows
                    if O == 0:          # today's chunking
                        assert [(p["row0"], p["own_rows"], p["stft_rows"]) for p in got] == \
                               [(r0, min(P * T, rows - r0), min(P * T, rows - r0)) for r0 in range(0, rows, P * T)]
    # the derived tile count the issue warns about: a full piece's own rows undercount its tiles at O = T/2
    assert stream.overlap_tiles(3 * 32, 64, 32) == 2 and capi.host_overlap_pieces(ROWS, 64, 32, 3)[0]["tiles"] == 3
    assert [(p["tiles"], p["own_rows"], p["stft_rows"]) for p in capi.host_overlap_pieces(ROWS, 64, 16, 3)] == [(3, 144, 160), (3, 133, 133)]
    assert [(p["tiles"], p["own_rows"], p["stft_rows"]) for p in capi.host_overlap_pieces(ROWS, 64, 32, 3)] == [(3, 96, 128), (3, 96, 128), (2, 85, 85)]


def test_piece_plan_bad_arguments():
    from spleeterrt_amd import capi, stream
    L = _lib()
    for rows, T, O, P in ((1000, 64, -1, 2), (1000, 64, 33, 2), (1000, 0, 0, 2), (1000, -64, 0, 2), (1000, 64, 16, 0), (1000, 64, 16, -3)):
        assert L.srtHostOverlapPieces(rows, T, O, P, None, 0) == 0 and b"srtHostOverlapPieces" in L.srtLastError(), (rows, T, O, P)
        with pytest.raises(capi.EngineError):
            capi.host_overlap_pieces(rows, T, O, P)
        with pytest.raises(ValueError):
            stream.host_overlap_pieces(rows, T, O, P)
    assert capi.host_overlap_pieces(0, 64, 16, 2) == [] == stream.host_overlap_pieces(0, 64, 16, 2)
    # a table shorter than the plan is filled up to its length and the count is still the whole plan's
    buf = (capi._HostPiece * 2)()
    assert L.srtHostOverlapPieces(ROWS, 64, 32, 1, C.cast(buf, C.c_void_p), 2) == 8
    assert (buf[1].tile0, buf[1].tiles, buf[1].row0, buf[1].own_rows, buf[1].stft_rows) == (1, 1, 32, 32, 64)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def host_pcm(oracle):
    L, R = oracle.synth_audio(N_RAGGED, SEED, True)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@pytest.fixture(scope="module")
def whole(oracle, coeffs):
    """srtSeparate under srtSetOverlap(O) on an engine that holds the signal (max_tiles = 12), per (F, O, switches): computed once, read-only"""
    cache = {}

    def get(F, O, ratio=False, ext=False, mix=None, precision=None):
        import spleeterrt_amd as srt
        key = (F, O, ratio, ext, None if mix is None else np.asarray(mix, np.float32).tobytes(), precision)
        if key not in cache:
            kw = {} if precision is None else {"precision": precision}
            eng = _engine(coeffs, S=3, F=F, max_tiles=12, batch_invariant=True, ratio_mask=ratio, **kw)
            eng.set_overlap(O)
            if ext:
                eng.set_mask_extension("average")
            if mix is not None:
                eng.set_mix(mix)
            L, R = _audio(oracle, N_RAGGED, SEED)
            ref = eng.separate(L, R).cpu().numpy()
            eng.close()
            ref.setflags(write=False)
            cache[key] = ref
        return cache[key]
    return get


def _small(coeffs, F, max_tiles, **kw):
    return _engine(coeffs, S=3, F=F, max_tiles=max_tiles, batch_invariant=True, **kw)


def _nan_out(eng):
    return np.full((eng.outputs, 2, ROWS * 1024 + 3072), np.nan, np.float32)


def _check(got, ref, tag):
    assert not np.isnan(got).any(), "%s: %d samples not written" % (tag, int(np.isnan(got).sum()))
    for s in range(ref.shape[0]):
        peak = float(np.abs(ref[s]).max())
        err = float(np.abs(got[s] - ref[s]).max())
        print("%s stem %d: max-abs / peak = %.3g" % (tag, s, err / peak))
        assert err <= BOUND * peak, (tag, s, err / peak)


@pytest.mark.gpu
@pytest.mark.parametrize("max_tiles", [1, 3])
@pytest.mark.parametrize("O", [16, 32])
@pytest.mark.parametrize("F", [512, 1536])
def test_piece_seams(coeffs, host_pcm, whole, F, O, max_tiles):
    """max_tiles = 1 sends every blend through the carry; 3 gives 3 + 3 tiles at O = 16 and 3 + 3 + 2 with a ragged last piece at O = 32"""
    eng = _small(coeffs, F, max_tiles)
    eng.set_timing(True)
    out, clipped = eng.separate_host_overlap(host_pcm, O, out=_nan_out(eng))
    kn = eng.get_timing_kernels()
    eng.set_timing(False)
    eng.close()
    assert clipped.tolist() == [0, 0, 0]
    npieces = -(-{16: 6, 32: 8}[O] // max_tiles)
    inv = [k for name, k in kn if name == "istft"]
    seam = "srt_istft_ola3_seam_kernel<4, false, false>" if F <= 1024 else "srt_istft_ola_seam_kernel<false, false>"
    first = "srt_istft_ola3_ov_kernel<4, false, false>" if F <= 1024 else "srt_istft_ola_ov_kernel<false>"
    assert len(inv) == npieces and inv[0].startswith(first) and all(k.startswith(seam) for k in inv[1:]), inv
    saves = [k for name, k in kn if name == "mask_seam"]
    assert len(saves) == npieces - 1 and all(k.startswith("srt_mask_seam_save_kernel") for k in saves), kn      # not after the last piece
    _check(out, whole(F, O), "seams F=%d O=%d max_tiles=%d" % (F, O, max_tiles))


@pytest.mark.gpu
@pytest.mark.parametrize("max_tiles", [1, 3])
@pytest.mark.parametrize("O", [16, 32])
def test_the_comparison_can_fail(oracle, coeffs, whole, O, max_tiles):
    """What a lost carry gives: rows [S, T) of each tile that precedes a piece boundary replaced by rows [0, O) of the next tile, so those rows take the next
    tile's mask unblended.  Through srtIstft on the large engine the result must miss the reference by more than 50 x the bound of test_piece_seams."""
    import torch
    F, S = 512, T_S - O
    eng = _engine(coeffs, S=3, F=F, max_tiles=12, batch_invariant=True)
    eng.set_overlap(O)
    L, R = _audio(oracle, N_RAGGED, SEED)
    spec, mag = eng.stft(L, R)
    masks = eng.forward(mag).cpu().numpy()
    nt = masks.shape[1]
    intact = eng.istft(spec, torch.from_numpy(masks).cuda()).cpu().numpy()
    assert np.array_equal(intact, whole(F, O))                  # the stages are srtSeparate (batch_invariant)
    rows = spec.shape[1]
    before = _blend_rows(masks, rows, T_S, O)
    for j in range(max_tiles, nt, max_tiles):
        masks[:, j - 1, :, S:] = masks[:, j, :, :O]
    # on the host the loss touches exactly the first O rows of every piece after the first, which now take their own tile's mask unblended
    changed = np.nonzero((_blend_rows(masks, rows, T_S, O) != before).any(axis=(0, 1, 3)))[0].tolist()
    assert changed == [j * S + k for j in range(max_tiles, nt, max_tiles) for k in range(O)], changed
    lost = eng.istft(spec, torch.from_numpy(masks).cuda()).cpu().numpy()
    eng.close()
    ref = whole(F, O)
    worst = max(float(np.abs(lost[s] - ref[s]).max()) / float(np.abs(ref[s]).max()) for s in range(3))
    print("lost carry O=%d max_tiles=%d: max-abs / peak = %.3g (%.0f x the bound)" % (O, max_tiles, worst, worst / BOUND))
    assert worst > 50 * BOUND, (O, max_tiles, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_one_piece_is_separate(coeffs, host_pcm, whole, F):
    import torch
    eng = _small(coeffs, F, 12)
    for O in (16, 32):
        out, _ = eng.separate_host_overlap(host_pcm, O, out=_nan_out(eng))
        assert torch.equal(torch.from_numpy(out), torch.from_numpy(whole(F, O).copy())), (F, O, float(np.abs(out - whole(F, O)).max()))
    eng.close()


@pytest.mark.gpu
def test_overlap_zero_is_the_host_stream(coeffs, host_pcm):
    eng = _small(coeffs, 512, 3)
    eng.set_timing(True)
    ref, _ = eng.separate_host_stream_io(host_pcm)
    kref = eng.get_timing_kernels()
    eng.set_timing(False)
    eng.set_timing(True)
    out, _ = eng.separate_host_overlap(host_pcm, 0, out=_nan_out(eng))
    kout = eng.get_timing_kernels()
    eng.set_timing(False)
    eng.close()
    assert len(kref) > 20 and kout == kref
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


MIX2 = [[0.5, 0.0, -1.0, 0.25], [0.0, 1.0, 1.0, 0.0]]          # two outputs over three stems and the input


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,ext,mix", [(True, False, None), (False, True, None), (False, False, MIX2), (True, True, MIX2)],
                         ids=["ratio", "average", "mix", "all"])
def test_options_across_seams(coeffs, host_pcm, whole, ratio, ext, mix):
    F, O = 512, 16
    eng = _small(coeffs, F, 3, ratio_mask=ratio)
    if ext:
        eng.set_mask_extension("average")
    plain, _ = eng.separate_host_overlap(host_pcm, O)
    if mix is not None:
        eng.set_mix(mix)
    out, _ = eng.separate_host_overlap(host_pcm, O, out=_nan_out(eng))
    _check(out, whole(F, O, ratio, ext, mix), "options ratio=%s ext=%s mix=%s" % (ratio, ext, mix is not None))
    # a one-hot row is that stem of the same call without the mix, bit for bit
    eng.set_mix([[0, 0, 1, 0], [1, 0, 0, 0]])
    hot, _ = eng.separate_host_overlap(host_pcm, O, out=_nan_out(eng))
    eng.close()
    assert np.array_equal(hot[0].view(np.uint32), plain[2].view(np.uint32)) and np.array_equal(hot[1].view(np.uint32), plain[0].view(np.uint32))


@pytest.mark.gpu
def test_fp16_mode_keeps_float_masks(coeffs, host_pcm, whole):
    """the reference keeps its masks as floats through a one-hot srtSetMix over all stems, as this call does by itself"""
    import spleeterrt_amd as srt
    F, O = 512, 16
    eye = np.eye(3, 4, dtype=np.float32)
    eng = _small(coeffs, F, 3, precision=srt.PREC_F16)
    out, _ = eng.separate_host_overlap(host_pcm, O, out=_nan_out(eng))
    eng.close()
    _check(out, whole(F, O, mix=eye, precision=srt.PREC_F16), "fp16 mode")


@pytest.mark.gpu
def test_pcm16_in_and_out(coeffs, host_pcm):
    F, O = 512, 16
    eng = _small(coeffs, F, 3)
    x = np.stack(host_pcm, 1)
    unpack = lambda q: (np.ascontiguousarray(q[:, 0].astype(np.float32) / np.float32(32768)), np.ascontiguousarray(q[:, 1].astype(np.float32) / np.float32(32768)))
    first, _ = eng.separate_host_overlap(unpack(rule(x)[0]), O)
    g = np.float32(1.0 / np.sort(np.abs(first).reshape(-1))[-3000])        # about three thousand samples of the float output pass full scale
    q = rule(x * g)[0]
    ref, c0 = eng.separate_host_overlap(unpack(q), O)
    assert c0.tolist() == [0, 0, 0]
    rq, rc = rule(ref)
    want, wclip = np.ascontiguousarray(rq.transpose(0, 2, 1)), [int(rc[s].sum()) for s in range(3)]
    buf = np.full(want.shape, 0x5A5A, np.int16)
    out, clipped = eng.separate_host_overlap(q, O, out_pcm16=True, out=buf)
    eng.close()
    print("clipped per stem:", clipped.tolist(), "expected", wclip)
    bad = np.argwhere(out != want)
    assert bad.size == 0, "first mismatch (stem, sample, channel) %s of %d" % (bad[0], len(bad))
    assert clipped.tolist() == wclip and sum(wclip) > 0


@pytest.mark.gpu
def test_the_engines_own_overlap_is_left_alone(oracle, coeffs, host_pcm, whole):
    import spleeterrt_amd as srt
    F, O = 512, 16
    eng = _small(coeffs, F, 3)
    before, _ = eng.separate_host_overlap(host_pcm, O)
    eng.set_overlap(8)
    out, _ = eng.separate_host_overlap(host_pcm, O, out=_nan_out(eng))
    assert np.array_equal(out.view(np.uint32), before.view(np.uint32))
    _check(out, whole(F, O), "engine overlap 8, call overlap 16")
    # still 8: 121 rows are three tiles at O = 8 (two at O = 0), and the chunked path still refuses
    Ls, Rs = _audio(oracle, 121 * 1024, 5)
    assert eng.stft(Ls, Rs)[1].shape[0] == 3
    with pytest.raises(srt.EngineError, match="overlap"):
        eng.separate_host_stream(*host_pcm)
    assert "srtSeparateHostStream:" in eng.L.srtLastError().decode()
    eng.close()


@pytest.mark.gpu
def test_refusals(coeffs, host_pcm, whole):
    import spleeterrt_amd as srt
    F, O = 512, 16
    eng = _small(coeffs, F, 3)
    Lh, Rh = host_pcm
    n = Lh.size
    out = _nan_out(eng)
    q = np.zeros((n, 2), np.int16)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda h, a, b, n_, ov, o, fl: eng.L.srtSeparateHostStreamOverlap(h, a, b, n_, ov, o, fl, None)
    cases = [("null engine", (None, vp(Lh), vp(Rh), n, O, vp(out), 0), ""),
             ("null input", (eng.h, None, vp(Rh), n, O, vp(out), 0), ""),
             ("null second channel", (eng.h, vp(Lh), None, n, O, vp(out), 0), ""),
             ("null output", (eng.h, vp(Lh), vp(Rh), n, O, None, 0), ""),
             ("unknown flag bits", (eng.h, vp(Lh), vp(Rh), n, O, vp(out), 8), "flag"),
             ("16-bit input with a second buffer", (eng.h, vp(q), vp(Rh), n, O, vp(out), srt.HOST_IN_PCM16), "h_in2"),
             ("short", (eng.h, vp(Lh), vp(Rh), 4095, O, vp(out), 0), "4096"),
             ("negative overlap", (eng.h, vp(Lh), vp(Rh), n, -1, vp(out), 0), "overlap_rows"),
             ("overlap above T/2", (eng.h, vp(Lh), vp(Rh), n, T_S // 2 + 1, vp(out), 0), "overlap_rows")]
    for name, args, word in cases:
        assert call(*args) == -1, name
        text = eng.L.srtLastError().decode()
        assert "srtSeparateHostStreamOverlap" in text and word in text, (name, text)
    eng.set_wiener(1)
    assert call(eng.h, vp(Lh), vp(Rh), n, O, vp(out), 0) == -1
    text = eng.L.srtLastError().decode()
    assert "srtSeparateHostStreamOverlap" in text and "Wiener" in text, text
    eng.set_wiener(0)
    bare = srt.Engine(F=F, T=T_S, stem_modes=(1, 0, 1), variant=srt.VARIANT_VST, max_tiles=3, batch_invariant=True)
    assert bare.L.srtSeparateHostStreamOverlap(bare.h, vp(Lh), vp(Rh), n, O, vp(out), 0, None) == -5
    assert "srtSeparateHostStreamOverlap" in bare.L.srtLastError().decode()
    bare.close()
    assert np.isnan(out).all()                                  # nothing was written by any of them
    # the Python layer refuses its argument errors before any library call
    for bad in (-1, T_S // 2 + 1, 1.5, "x", None):
        with pytest.raises(srt.EngineError, match="separate_host_overlap"):
            eng.separate_host_overlap(host_pcm, bad)
    # the call works, and again after the staging (the carry with it) has been released
    a, _ = eng.separate_host_overlap(host_pcm, O, out=out)
    _check(a, whole(F, O), "after the refusals")
    eng.release_staging()
    b, _ = eng.separate_host_overlap(host_pcm, O, out=_nan_out(eng))
    eng.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
