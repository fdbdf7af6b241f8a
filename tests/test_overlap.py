"""Overlapped network tiles with cross-faded masks (srtSetOverlap).

CPU: srtOverlapTiles against stream.overlap_tiles and a brute-force count; out-of-range overlaps refused.  GPU: O = 0 is the present path (bits and
launch list), the overlapped magnitude layout is pure data movement, the blend inside the inverse kernels against host-blended masks on the O = 0
kernels (both kernel families, with and without the ratio mask), srtSeparate = srtStft -> srtForward -> srtIstft, the CPU oracle end to end (fp32 with
and without ratio_mask, the fp16 mode at the bench shape), coverage of the output, graph mode across overlaps, capacity, and every refusal."""
import ctypes as C

import numpy as np
import pytest

T_S, F_S = 64, 512
MODES = (1, 0, 1, 0, 1, 0, 1, 0)


def _lib():
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


def _brute_tiles(rows, T, O):
    """tiles of stride T - O laid one after the other until every row is covered"""
    if rows == 0:
        return 0
    S, j = T - O, 0
    while j * S + T < rows:
        j += 1
    return j + 1


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_overlap_tiles_rule():
    from spleeterrt_amd import stream
    L = _lib()
    rng = np.random.default_rng(13)
    for T in (64, 128, 256):
        for O in (0, 1, T // 4, T // 2):
            S = T - O
            rows_set = [1, O, T, T + 1, S + T, S + T + 1] + [int(x) for x in rng.integers(1, 40 * T, size=40)]
            for rows in rows_set:
                nt = L.srtOverlapTiles(rows, T, O)
                assert nt == stream.overlap_tiles(rows, T, O) == _brute_tiles(rows, T, O), (rows, T, O, nt)
                if rows == 0:
                    assert nt == 0
                    continue
                # every row is covered, and each tile owns at least one row that no earlier tile covers
                assert (nt - 1) * S + T >= rows, (rows, T, O, nt)
                for j in range(1, nt):
                    assert (j - 1) * S + T < rows, (rows, T, O, nt, j)      # tile j's first new row, (j - 1) S + T, exists
                if O == 0:
                    assert nt == (rows + T - 1) // T
                if rows <= T:
                    assert nt == 1
                # a row lies in at most two tiles (O <= T / 2)
                r = min(rows - 1, S + O - 1)
                assert sum(1 for j in range(nt) if j * S <= r < j * S + T) <= 2


def test_overlap_out_of_range_is_refused():
    from spleeterrt_amd import stream
    L = _lib()
    for T, O in ((64, -1), (64, 33), (256, 129), (0, 0), (-64, 0)):
        assert L.srtOverlapTiles(1000, T, O) == 0 and b"srtOverlapTiles" in L.srtLastError(), (T, O)
        with pytest.raises(ValueError):
            stream.overlap_tiles(1000, T, O)
    assert L.srtOverlapTiles(1000, 64, 32) == 31 and L.srtOverlapTiles(1000, 256, 128) == 7
    L.srtSetOverlap.argtypes = [C.c_void_p, C.c_int]
    assert L.srtSetOverlap(None, 0) == -1 and b"srtSetOverlap" in L.srtLastError()


def test_rank_helpers_refuse_overlap():
    """the chunked / ranked helpers of stream.py cut at back-to-back tile boundaries: an engine with an overlap is refused before anything runs"""
    from spleeterrt_amd import stream

    class Stand:
        T, max_tiles, overlap, wiener = 64, 2, 16, 0

        def separate_ex(self, *a):
            raise AssertionError("must not run")

        separate_host_stream = separate_ex
    z = np.zeros(64 * 1024 * 3, np.float32)
    with pytest.raises(ValueError, match="overlap"):
        stream.separate_stream(Stand(), z, z)
    with pytest.raises(ValueError, match="overlap"):
        stream.separate_host_range(Stand(), z, z)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _engine(coeffs, S=2, **kw):
    import spleeterrt_amd as srt
    kw.setdefault("variant", srt.VARIANT_VST)
    kw.setdefault("F", F_S)
    kw.setdefault("T", T_S)
    eng = srt.Engine(stem_modes=MODES[:S], **kw)
    for s in range(S):
        eng.set_coeff(s, coeffs(s))
    return eng


def _audio(oracle, n, seed):
    import torch
    L, R = oracle.synth_audio(n, seed, True)
    return torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()


def _rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


def _blend_rows(masks, rows, T, O):
    """the rule of the issue on the host, fp32 step by step: masks [S][tiles][2][T][F] in the overlapped layout -> per-row masks [S][2][rows][F]"""
    from spleeterrt_amd import stream
    S_, nt = masks.shape[0], masks.shape[1]
    assert nt == stream.overlap_tiles(rows, T, O)
    st = T - O
    out = np.empty((S_, 2, rows, masks.shape[-1]), np.float32)
    for r in range(rows):
        j1 = min(r // st, nt - 1)
        k = r - j1 * st
        b = masks[:, j1, :, k]
        if j1 > 0 and k < O:
            a = masks[:, j1 - 1, :, k + st]
            w = np.float32(k + 0.5) / np.float32(O)
            out[:, :, r] = a + w * (b - a)
        else:
            out[:, :, r] = b
    return out


def _pack_rows(m, T):
    """per-row masks [S][2][rows][F] -> the O = 0 layout [S][ceil(rows / T)][2][T][F] (rows past the signal: zero)"""
    S_, _, rows, F = m.shape
    nt = (rows + T - 1) // T
    p = np.zeros((S_, nt, 2, T, F), np.float32)
    for r in range(rows):
        p[:, r // T, :, r % T] = m[:, :, r]
    return p


N_RAGGED = (4 * 48 + 64 + 21) * 1024 - 500            # 277 rows (273 transformed frames): six overlapped tiles at O = 16 (stride 48), eight at O = 32; four tiles + a tail at O = 0


@pytest.mark.gpu
def test_overlap_zero_is_the_present_path(oracle, coeffs):
    """srtSeparate after srtSetOverlap(e, 0) - and after an overlap was on and switched off again - equals a fresh engine that never called it, and launches the same kernels"""
    import torch
    L, R = _audio(oracle, N_RAGGED, 21)
    outs, lists = [], []
    for touch in (False, True):
        eng = _engine(coeffs, max_tiles=8, batch_invariant=True)
        if touch:
            eng.set_overlap(16)
            eng.separate(L, R)
            eng.set_overlap(0)
        eng.separate(L, R)
        eng.set_timing(True)
        outs.append(eng.separate(L, R).clone())
        lists.append(eng.get_timing_kernels())
        eng.set_timing(False)
        eng.close()
    assert torch.equal(outs[0], outs[1])
    assert lists[0] == lists[1]
    assert lists[0][0] == ("stft", "srt_stft_kernel") and lists[0][-1][0] == "istft" and lists[0][-1][1].startswith("srt_istft_ola3_kernel<4, false, false>"), (lists[0][0], lists[0][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_overlapped_magnitudes_are_pure_data_movement(oracle, coeffs, F):
    """tile j of the overlapped d_mag = rows [jS, jS + T) of the O = 0 magnitudes, zeros past the last row; the spectrum does not change"""
    import torch
    from spleeterrt_amd import stream
    eng = _engine(coeffs, S=1, F=F, max_tiles=12)
    L, R = _audio(oracle, N_RAGGED, 22)
    spec0, mag0 = eng.stft(L, R)
    rows = spec0.shape[1]
    assert rows == 277
    flat = mag0.permute(1, 0, 2, 3).reshape(2, -1, F)                 # [2][tiles * T][F]: row r of the signal at index r
    assert bool((flat[:, rows:] == 0).all())
    for O in (16, 32):
        eng.set_overlap(O)
        spec, mag = eng.stft(L, R)
        nt, st = stream.overlap_tiles(rows, T_S, O), T_S - O
        assert mag.shape == (nt, 2, T_S, F) and nt == eng.L.srtOverlapTiles(rows, T_S, O)
        assert torch.equal(spec, spec0)
        for j in range(nt):
            want = torch.zeros((2, T_S, F), device="cuda")
            hi = min(j * st + T_S, rows)
            want[:, :hi - j * st] = flat[:, j * st:hi]
            assert torch.equal(mag[j], want), (O, j)
        eng.set_timing(True)
        eng.stft(L, R)
        kn = eng.get_timing_kernels()
        eng.set_timing(False)
        assert kn == [("stft", "srt_stft_ov_kernel")], kn
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_blend_in_the_inverse_kernels(oracle, coeffs, F):
    """srtIstft with an overlap on masks in the overlapped layout against srtIstft at O = 0 on the host-blended masks: <= 2e-6 of the peak (the bound the
    project allows for association differences at seams).  Random masks, tiles that are one constant each, and all-ones (bit-equal to the O = 0 all-ones output)."""
    import torch
    from spleeterrt_amd import stream
    S = 3
    eng = _engine(coeffs, S=S, F=F, max_tiles=12)
    L, R = _audio(oracle, N_RAGGED, 23)
    spec, _ = eng.stft(L, R, want_mag=False)
    rows = spec.shape[1]
    rng = np.random.default_rng(31)
    ones0 = eng.istft(spec, torch.ones((S, (rows + T_S - 1) // T_S, 2, T_S, F), device="cuda"))
    for O in (16, 32):
        nt = stream.overlap_tiles(rows, T_S, O)
        cases = {"random": rng.random((S, nt, 2, T_S, F), dtype=np.float32),
                 "constant tiles": np.broadcast_to(rng.random((S, nt, 1, 1, 1), dtype=np.float32), (S, nt, 2, T_S, F)).copy()}
        for name, m in cases.items():
            eng.set_overlap(0)
            ref = eng.istft(spec, torch.from_numpy(_pack_rows(_blend_rows(m, rows, T_S, O), T_S)).cuda())
            eng.set_overlap(O)
            eng.set_timing(True)
            got = eng.istft(spec, torch.from_numpy(m).cuda())
            kn = eng.get_timing_kernels()
            eng.set_timing(False)
            assert kn[0][1].startswith("srt_istft_ola3_ov_kernel<4, false, false>" if F <= 1024 else "srt_istft_ola_ov_kernel<false>"), kn
            peak = float(ref.abs().max())
            err = float((got - ref).abs().max())
            print("blend F=%d O=%d %s: max-abs / peak = %.3g" % (F, O, name, err / peak))
            assert err <= 2e-6 * peak, (F, O, name, err / peak)
        eng.set_overlap(O)
        got1 = eng.istft(spec, torch.ones((S, nt, 2, T_S, F), device="cuda"))
        assert torch.equal(got1, ones0), (F, O)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_blend_then_ratio_in_the_inverse_kernels(oracle, coeffs, F):
    """The ratio case of the blend test.  The public srtIstft never normalises (srtRatioMask is its caller's business), so the kernels' blend-then-ratio
    prologue is reached through srtSeparate on a ratio_mask engine; its raw masks are the ones srtStft -> srtForward give under batch_invariant.  The host
    blends them, normalises the BLENDED masks (oracle.ratio_mask) and packs them in the O = 0 layout; a plain engine's srtIstft at O = 0 on those must
    agree with srtSeparate to <= 2e-6 of the peak."""
    import torch
    S = 3
    eng = _engine(coeffs, S=S, F=F, max_tiles=12, batch_invariant=True, ratio_mask=True)
    L, R = _audio(oracle, N_RAGGED, 24)
    for O in (16, 32):
        eng.set_overlap(O)
        eng.set_timing(True)
        got = eng.separate(L, R)
        kn = eng.get_timing_kernels()
        eng.set_timing(False)
        assert kn[-1][1].startswith("srt_istft_ola3_ov_kernel<4, true, false>" if F <= 1024 else "srt_istft_ola_ov_kernel<true>"), kn[-1]
        spec, mag = eng.stft(L, R)
        rows = spec.shape[1]
        raw = eng.forward(mag).cpu().numpy()
        m = oracle.ratio_mask(_blend_rows(raw, rows, T_S, O))
        eng.set_overlap(0)
        ref = eng.istft(spec, torch.from_numpy(_pack_rows(m, T_S)).cuda())       # (srtIstft applies masks as given, on a ratio_mask engine too)
        peak = float(ref.abs().max())
        err = float((got - ref).abs().max())
        print("blend + ratio F=%d O=%d: max-abs / peak = %.3g" % (F, O, err / peak))
        assert err <= 2e-6 * peak, (F, O, err / peak)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_separate_is_the_composition_of_its_stages(oracle, coeffs, F):
    """srtSeparate with an overlap = srtStft -> srtForward -> srtIstft with the same overlap, bit for bit (batch_invariant).  Without ratio_mask: a
    caller-side srtRatioMask would normalise the tiles' masks BEFORE the blend, which is not what srtSeparate computes (blend first), so the ratio case is
    left to the oracle comparison."""
    import torch
    eng = _engine(coeffs, S=2, F=F, max_tiles=12, batch_invariant=True)
    L, R = _audio(oracle, N_RAGGED, 25)
    for O in (16, 32):
        eng.set_overlap(O)
        whole = eng.separate(L, R)
        spec, mag = eng.stft(L, R)
        assert mag.shape[0] == eng.tiles(spec.shape[1])
        parts = eng.istft(spec, eng.forward(mag))
        assert torch.equal(whole, parts), (F, O, float((whole - parts).abs().max()))
    eng.close()


def _oracle_overlap(oracle, coeffs, L, R, T, F, O, S, ratio, oob=0.1):
    """the feature restated over the oracle's stages: stft; magnitudes of rows [jS, jS + T) per tile; the network per (stem, tile); blend; ratio; mask; istft"""
    from spleeterrt_amd import stream
    re, im = oracle.stft(L, R)
    rows = re.shape[1]
    nt, st = stream.overlap_tiles(rows, T, O), T - O
    masks = np.empty((S, nt, 2, T, F), np.float32)
    for j in range(nt):
        mag = oracle.magnitude_tile(re, im, j * st, T, F)
        for s in range(S):
            masks[s, j] = oracle.forward(coeffs(s), mag, MODES[s], oracle.VARIANT_VST)
    m = _blend_rows(masks, rows, T, O)
    if ratio:
        m = oracle.ratio_mask(m)
    out = []
    for s in range(S):
        r, i = re.copy(), im.copy()
        r[:, :, :F] *= m[s]
        i[:, :, :F] *= m[s]
        r[:, :, F:2049] *= np.float32(oob)
        i[:, :, F:2049] *= np.float32(oob)
        out.append(oracle.istft(r, i))
    return np.stack(out), m


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [False, True])
@pytest.mark.parametrize("O", [16, 32])
def test_end_to_end_against_the_oracle(oracle, coeffs, O, ratio):
    """4 stems fp32 on a clip of at least four overlapped tiles plus a tail, every output sample compared: stems rel-RMS <= 1e-4 and max-abs <= 1e-4 of
    the peak"""
    from spleeterrt_amd import stream
    S = 4
    eng = _engine(coeffs, S=S, max_tiles=12, ratio_mask=ratio, overlap=O)
    L, R = _audio(oracle, N_RAGGED, 26)
    got = eng.separate(L, R).cpu().numpy()
    eng.close()
    assert stream.overlap_tiles(277, T_S, O) >= 5
    ref, _ = _oracle_overlap(oracle, coeffs, L.cpu().numpy(), R.cpu().numpy(), T_S, F_S, O, S, ratio)
    assert got.shape == ref.shape and np.isfinite(got).all()
    for s in range(S):
        peak = float(np.abs(ref[s]).max())
        rr, ma = _rel_rms(got[s], ref[s]), float(np.abs(got[s] - ref[s]).max()) / peak
        print("oracle O=%d ratio=%d stem %d: rel-RMS %.3g, max-abs / peak %.3g" % (O, ratio, s, rr, ma))
        assert rr <= 1e-4, (O, ratio, s, rr)
        assert ma <= 1e-4, (O, ratio, s, ma)


@pytest.mark.gpu
def test_fp16_mode_at_the_bench_shape(oracle, coeffs):
    """the fp16 mode at F = 1024, T = 256, O = 64, five overlapped tiles (868 rows) x 4 stems: the half-mask inverse form runs with the overlap on, and every
    stem is within the fp16 tolerance class (rel-RMS <= 1e-2) of the fp32 oracle"""
    import spleeterrt_amd as srt
    T, F, O, S = 256, 1024, 64, 4
    n = 868 * 1024 - 77
    eng = _engine(coeffs, S=S, F=F, T=T, max_tiles=5, precision=srt.PREC_F16, overlap=O)
    assert eng.tiles(868) == 5
    L, R = _audio(oracle, n, 27)
    eng.separate(L, R)
    eng.set_timing(True)
    got = eng.separate(L, R).cpu().numpy()
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    eng.close()
    assert ks[0] == ("stft", "srt_stft_ov_kernel") and ks[-1] == ("istft", "srt_istft_ola3_ov_kernel<4, false, true>"), (ks[0], ks[-1])
    ref, _ = _oracle_overlap(oracle, coeffs, L.cpu().numpy(), R.cpu().numpy(), T, F, O, S, False)
    assert got.shape == ref.shape and np.isfinite(got).all()
    for s in range(S):
        rr = _rel_rms(got[s], ref[s])
        print("fp16 bench shape stem %d: rel-RMS %.3g" % (s, rr))
        assert rr <= 1e-2, (s, rr)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_overlap_writes_every_sample_and_nothing_past(oracle, coeffs, F):
    """the whole [n_stems][2][srtIstftLength(rows)] region is written, nothing behind it is touched"""
    import torch
    eng = _engine(coeffs, S=2, F=F, max_tiles=12, overlap=32)
    L, R = _audio(oracle, N_RAGGED, 28)
    need = 2 * 2 * eng.L.srtIstftLength(eng.L.srtStftRows(N_RAGGED))
    out = torch.full((need + 5000,), float("nan"), device="cuda")
    out[need:] = 12345.0
    eng.separate(L, R, out)
    h = out.cpu().numpy()
    assert np.isfinite(h[:need]).all(), int(np.isnan(h[:need]).sum())
    assert (h[need:] == 12345.0).all()
    eng.close()


@pytest.mark.gpu
def test_graph_mode_keys_on_the_overlap(oracle, coeffs):
    """graph mode: calls at O = 32, O = 0, O = 32 on the same buffers each equal their eager result; a graph captured at one overlap is never replayed at
    another, and a repeated call replays"""
    import torch
    L, R = _audio(oracle, N_RAGGED, 29)
    eager = {}
    eng = _engine(coeffs, S=2, max_tiles=12, batch_invariant=True)
    for O in (32, 0):
        eng.set_overlap(O)
        eager[O] = eng.separate(L, R).clone()
    eng.close()
    assert not torch.equal(eager[0], eager[32])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng = _engine(coeffs, S=2, max_tiles=12, batch_invariant=True)
        eng.set_graph_mode(True)
        out = torch.empty_like(eager[0])
        for O in (32, 0, 32, 32, 0):
            eng.set_overlap(O)
            out.fill_(float("nan"))
            eng.separate(L, R, out)
            s.synchronize()
            assert torch.equal(out, eager[O]), O
        eng.close()


@pytest.mark.gpu
def test_capacity_counts_overlapped_tiles(oracle, coeffs):
    """a signal with srtOverlapTiles(rows) > max_tiles is refused although ceil(rows / T) <= max_tiles; the largest signal that fits is accepted"""
    import torch
    from spleeterrt_amd import stream
    O, mt = 32, 4
    eng = _engine(coeffs, S=1, max_tiles=mt, overlap=O)
    fit_rows = (mt - 1) * (T_S - O) + T_S                              # 160 rows: exactly four overlapped tiles
    assert stream.overlap_tiles(fit_rows, T_S, O) == mt and stream.overlap_tiles(fit_rows + 1, T_S, O) == mt + 1 and (fit_rows + 1 + T_S - 1) // T_S <= mt
    Lb, Rb = _audio(oracle, (fit_rows + 1) * 1024, 30)
    out = torch.full((1, 2, eng.L.srtIstftLength(fit_rows + 1)), float("nan"), device="cuda")
    rc = eng.L.srtSeparate(eng.h, C.c_void_p(Lb.data_ptr()), C.c_void_p(Rb.data_ptr()), Lb.numel(), C.c_void_p(out.data_ptr()))
    assert rc == -1 and b"max_tiles" in eng.L.srtLastError()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    spec = torch.empty((2, fit_rows + 1, 2052, 2), device="cuda")
    mag = torch.empty((mt + 1, 2, T_S, F_S), device="cuda")
    assert eng.L.srtStft(eng.h, C.c_void_p(Lb.data_ptr()), C.c_void_p(Rb.data_ptr()), Lb.numel(), C.c_void_p(spec.data_ptr()), C.c_void_p(mag.data_ptr())) == -1
    Lf, Rf = Lb[:fit_rows * 1024], Rb[:fit_rows * 1024]
    got = eng.separate(Lf.contiguous(), Rf.contiguous())
    assert torch.isfinite(got).all()
    eng.set_overlap(0)                                                  # ... and the longer one fits the back-to-back cut
    assert torch.isfinite(eng.separate(Lb, Rb)).all()
    eng.close()


@pytest.mark.gpu
def test_set_overlap_range(oracle, coeffs):
    eng = _engine(coeffs, S=1, max_tiles=1)
    for bad in (-1, T_S // 2 + 1, T_S):
        assert eng.L.srtSetOverlap(eng.h, bad) == -1 and b"srtSetOverlap" in eng.L.srtLastError()
    for ok in (0, 1, T_S // 2):
        assert eng.L.srtSetOverlap(eng.h, ok) == 0
    eng.close()


@pytest.mark.gpu
def test_refusals(oracle, coeffs):
    """every entry point that does not take an overlap returns -1 with "overlap" in the text and leaves its NaN-filled output untouched; after
    srtSetOverlap(e, 0) the same call succeeds"""
    import torch
    import spleeterrt_amd as srt
    from spleeterrt_amd import capi
    eng = _engine(coeffs, S=2, max_tiles=8)
    Lq = eng.L
    n = 100 * 1024 + 300                                               # 101 rows: two tiles
    rows, frames = Lq.srtStftRows(n), Lq.srtStftFrames(n)
    ln = Lq.srtIstftLength(rows)
    Ld, Rd = _audio(oracle, n, 33)
    Lh, Rh = Ld.cpu().numpy(), Rd.cpu().numpy()
    vp = C.c_void_p
    spec, mag = eng.stft(Ld, Rd)
    masks = eng.forward(mag)

    d_out = torch.empty((3, 2, ln), device="cuda")
    h_out = np.empty((3, 2, ln), np.float32)
    P1 = vp * 1

    calls = {
        "srtSeparateHostStream": (lambda: Lq.srtSeparateHostStream(eng.h, vp(Lh.ctypes.data), vp(Rh.ctypes.data), n, frames, rows, vp(h_out.ctypes.data)), "h"),
        "srtSeparateHostStreamEx": (lambda: Lq.srtSeparateHostStreamEx(eng.h, vp(Lh.ctypes.data), vp(Rh.ctypes.data), n, frames, rows, vp(h_out.ctypes.data), 0), "h"),
        "srtSeparateCli": (lambda: Lq.srtSeparateCli(eng.h, vp(Ld.data_ptr()), vp(Rd.data_ptr()), n, 2, vp(d_out.data_ptr())), "d"),
        "srtSeparateCliHost": (lambda: Lq.srtSeparateCliHost(eng.h, vp(Lh.ctypes.data), vp(Rh.ctypes.data), n, 3, vp(h_out.ctypes.data)), "h"),
        "srtSeparateBatch": (lambda: Lq.srtSeparateBatch(eng.h, 1, P1(Ld.data_ptr()), P1(Rd.data_ptr()), (C.c_size_t * 1)(n), P1(d_out.data_ptr())), "d"),
        "srtIstftWiener": (lambda: Lq.srtIstftWiener(eng.h, vp(spec.data_ptr()), rows, vp(masks.data_ptr()), 1, vp(d_out.data_ptr())), "d"),
    }
    for name, (call, where) in calls.items():
        eng.set_overlap(16)
        d_out.fill_(float("nan"))
        h_out.fill(np.nan)
        assert call() == -1, name
        assert b"overlap" in Lq.srtLastError(), (name, Lq.srtLastError())
        torch.cuda.synchronize()
        assert bool(torch.isnan(d_out).all()) and np.isnan(h_out).all(), name
        eng.set_overlap(0)
        assert call() == 0, (name, Lq.srtLastError())
        torch.cuda.synchronize()
        written = h_out if where == "h" else d_out.cpu().numpy()
        assert np.isfinite(written[:2]).all(), name
    # srtSeparate with the Wiener filter on
    eng.set_wiener(1)
    eng.set_overlap(16)
    d_out.fill_(float("nan"))
    assert Lq.srtSeparate(eng.h, vp(Ld.data_ptr()), vp(Rd.data_ptr()), n, vp(d_out.data_ptr())) == -1 and b"overlap" in Lq.srtLastError()
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_out).all())
    eng.set_overlap(0)
    assert Lq.srtSeparate(eng.h, vp(Ld.data_ptr()), vp(Rd.data_ptr()), n, vp(d_out.data_ptr())) == 0
    eng.set_wiener(0)
    eng.release_staging()
    eng.close()

    # the multi-device driver: an overlap on one of its engines
    cfg = capi._Config()
    cfg.F, cfg.T, cfg.n_stems, cfg.variant, cfg.max_tiles = F_S, T_S, 2, srt.VARIANT_VST, 2
    for s in range(2):
        cfg.stem_mode[s], cfg.oob_weight[s] = MODES[s], 0.1
    m = vp()
    assert Lq.srtMultiCreate(C.byref(cfg), None, 1, C.byref(m)) == 0, Lq.srtLastError()
    for s in range(2):
        c = np.ascontiguousarray(coeffs(s), np.float32)
        assert Lq.srtMultiSetCoeffHost(m, s, vp(c.ctypes.data)) == 0
    e0 = Lq.srtMultiEngine(m, 0)
    multi = {
        "srtMultiSeparateHost": lambda: Lq.srtMultiSeparateHost(m, vp(Lh.ctypes.data), vp(Rh.ctypes.data), n, vp(h_out.ctypes.data), 0),
        "srtMultiSeparateCliHost": lambda: Lq.srtMultiSeparateCliHost(m, vp(Lh.ctypes.data), vp(Rh.ctypes.data), n, 2, vp(h_out.ctypes.data)),
    }
    for name, call in multi.items():
        assert Lq.srtSetOverlap(e0, 16) == 0
        h_out.fill(np.nan)
        assert call() == -1 and b"overlap" in Lq.srtLastError(), (name, Lq.srtLastError())
        assert np.isnan(h_out).all(), name
        assert Lq.srtSetOverlap(e0, 0) == 0
        assert call() == 0, (name, Lq.srtLastError())
        assert np.isfinite(h_out[:2]).all(), name
    Lq.srtMultiDestroy(m)
