"""Multichannel Wiener filter (srtSetWiener / srtIstftWiener, csrc/srt_wiener.hip): official Spleeter's `--mwf` post-processing,
norbert.wiener(v, x, n) with its defaults.  `wiener_np` below restates the specification in float64 numpy; the CPU tests check the
restatement itself, the GPU tests hold the kernels to it (through the oracle's inverse transform) and check the entry points around it."""
import ctypes as C

import numpy as np
import pytest

EPS = 2.0 ** -23            # fp32 machine epsilon: norbert's default eps for complex64
SPEC_LD = 2052


def wiener_np(spec, masks, T, F, iters, oob, stats_spec=None, stats_masks=None):
    """spec: complex [2, rows, >= 2049] in the engine's stored convention; masks [S, ntiles, 2, T, F].  Returns (out [S, 2, rows, 2049] complex,
    covs: per iteration (R [S, F, 2, 2], weight sums [S, F] in normalised units, a)).
    stats_spec / stats_masks: an iterable of (spec rows, mask rows [S, 2, rows, F]) chunks over which R and a are accumulated instead (the whole
    call), while only `spec` / `masks` are filtered."""
    S = masks.shape[0]
    rows = spec.shape[1]
    m = _mask_rows(masks, rows)

    def start(sp, mk):
        x = 4096.0 * sp[:, :, :F].astype(np.complex128)
        v = mk.astype(np.float64) * np.abs(x)[None]
        return x, v / (EPS + v.sum(0)) * x[None]

    chunks = [(spec, m)] if stats_spec is None else list(zip(stats_spec, stats_masks))
    a = max(1.0, max(float(np.abs(4096.0 * sp[:, :, :2049].astype(np.complex128)).max()) for sp, _ in chunks) / 10.0)
    covs = []
    for it in range(iters):
        Ryy = np.zeros((S, F, 2, 2), np.complex128)
        wsum = np.zeros((S, F))
        for sp, mk in chunks:
            x, y = start(sp, mk)
            xh, yh = x / a, y / a
            for R, _, _ in covs:
                yh = _em_step(yh, xh, R)
            Ryy += np.einsum("sctf,sdtf->sfcd", yh, yh.conj())
            wsum += (0.5 * (np.abs(yh) ** 2).sum(1)).sum(1)
        covs.append((Ryy / (EPS + wsum)[..., None, None], wsum, a))
    x, y = start(spec, m)
    xh, yh = x / a, y / a
    for R, _, _ in covs:
        yh = _em_step(yh, xh, R)
    out = np.empty((S, 2, rows, 2049), np.complex128)
    out[..., :F] = a * yh / 4096.0
    out[..., F:] = np.asarray(oob, np.float64)[:, None, None, None] * spec[None, :, :, F:2049]
    return out, covs


def _mask_rows(masks, rows):
    S, nt, _, T, F = masks.shape
    return masks.transpose(0, 2, 1, 3, 4).reshape(S, 2, nt * T, F)[:, :, :rows]


def _em_step(yh, xh, R):
    v = 0.5 * (np.abs(yh) ** 2).sum(1)                                  # [S, rows, F]
    Cm = np.einsum("stf,sfcd->tfcd", v, R) + np.sqrt(EPS) * np.eye(2)
    z = np.einsum("tfcd,dtf->ctf", np.linalg.inv(Cm), xh)              # C^-1 x
    return v[:, None] * np.einsum("sfcd,dtf->sctf", R, z)


def _gains(spec, masks, T, F, iters):
    """Sum over stems of W_j and sqrt(eps) C^-1 at every (row, bin), from the restatement's last iteration."""
    S = masks.shape[0]
    rows = spec.shape[1]
    _, covs = wiener_np(spec, masks, T, F, iters, np.ones(S))
    x = 4096.0 * spec[:, :, :F]
    v = _mask_rows(masks, rows) * np.abs(x)[None]
    a = covs[0][2]
    yh = v / (EPS + v.sum(0)) * x[None] / a
    for R, _, _ in covs[:-1]:
        yh = _em_step(yh, x / a, R)
    R = covs[-1][0]
    vv = 0.5 * (np.abs(yh) ** 2).sum(1)
    Cm = np.einsum("stf,sfcd->tfcd", vv, R) + np.sqrt(EPS) * np.eye(2)
    Ci = np.linalg.inv(Cm)
    W = np.einsum("stf,sfcd,tfde->tfce", vv, R, Ci)
    return W, np.sqrt(EPS) * Ci


def _rand_spec(rng, rows, scale=0.05):
    sp = np.zeros((2, rows, SPEC_LD), np.complex128)
    sp[:, :, :2049] = scale * (rng.standard_normal((2, rows, 2049)) + 1j * rng.standard_normal((2, rows, 2049)))
    return sp


# ------------------------------------------------------------------------------------------------------------ CPU: the restatement

def test_restatement_disjoint_masks_route_each_bin_to_its_owner():
    """0/1 masks, each bin owned by one stem, full-rank stereo sources: the owner's output is the mixture and the others are ~0, to O(sqrt(eps))."""
    rng = np.random.default_rng(1)
    S, T, F, rows = 3, 16, 64, 40
    spec = _rand_spec(rng, rows)
    owner = rng.integers(0, S, F)
    masks = np.zeros((S, 3, 2, T, F), np.float32)
    for j in range(S):
        masks[j, :, :, :, owner == j] = 1.0
    for iters in (1, 2):
        out, _ = wiener_np(spec, masks, T, F, iters, np.ones(S))
        x = spec[:, :, :F]
        peak = np.abs(x).max()
        for j in range(S):
            own = owner == j
            assert np.abs(out[j][:, :, :F][:, :, own] - x[:, :, own]).max() <= 1e-3 * peak
            assert np.abs(out[j][:, :, :F][:, :, ~own]).max() <= 1e-3 * peak


def test_restatement_stem_sum_is_identity_minus_regulariser():
    """sum_j W_j = I - sqrt(eps) C^-1, to rounding."""
    rng = np.random.default_rng(2)
    S, T, F, rows = 4, 16, 64, 32
    spec = _rand_spec(rng, rows)
    masks = rng.random((S, 2, 2, T, F)).astype(np.float32)
    for iters in (1, 3):
        W, reg = _gains(spec, masks, T, F, iters)                      # W: already summed over the stems
        assert np.abs(W - (np.eye(2) - reg)).max() <= 1e-9


def test_restatement_one_stem_passes_the_mixture():
    rng = np.random.default_rng(3)
    T, F, rows = 16, 128, 48
    spec = _rand_spec(rng, rows)
    masks = rng.random((1, 3, 2, T, F)).astype(np.float32) * 0.9 + 0.05
    out, _ = wiener_np(spec, masks, T, F, 2, [0.3])
    x = spec[:, :, :F]
    assert np.abs(out[0][:, :, :F] - x).max() <= 1e-3 * np.abs(x).max()
    assert np.allclose(out[0][:, :, F:], 0.3 * spec[:, :, F:2049])


def test_stream_helpers_refuse_a_wiener_engine_across_ranks():
    """stream.py's multi-rank helpers: a rank's share would be filtered with its own covariance."""
    from spleeterrt_amd import stream

    class Stub:
        T, max_tiles, S, wiener = 64, 4, 2, 1

        def separate_ex(self, *a):
            raise AssertionError("must refuse before separating")

        def separate_host_stream(self, *a, **k):
            raise AssertionError("must refuse before separating")
    L = np.zeros(4096 * 40, np.float32)
    for fn in (stream.separate_stream, stream.separate_host_range):
        with pytest.raises(ValueError, match="whole signal"):
            fn(Stub(), L, L, rank=0, world=2)


# ------------------------------------------------------------------------------------------------------------ GPU

def _stereo_clip(n, seed):
    """panned tones plus independent noise: the two channels differ"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    L = np.zeros(n)
    R = np.zeros(n)
    for f, pan in ((220.0, 0.1), (554.0, 0.8), (1760.0, 0.45), (4100.0, 0.95), (9000.0, 0.3)):
        s = 0.08 * np.sin(2 * np.pi * f * t + rng.random() * 6.0)
        L += (1 - pan) * s
        R += pan * s
    L += 0.01 * rng.standard_normal(n)
    R += 0.01 * rng.standard_normal(n)
    return L.astype(np.float32), R.astype(np.float32)


def _spec_tensor(re, im):
    import torch
    rows = re.shape[1]
    sp = np.zeros((2, rows, SPEC_LD, 2), np.float32)
    sp[:, :, :2049, 0] = re[:, :, :2049]
    sp[:, :, :2049, 1] = im[:, :, :2049]
    return torch.from_numpy(sp).cuda()


def _to_complex(spec_t):
    a = spec_t.cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def _istft_of(oracle, out):
    """oracle inverse of every stem of the restatement's filtered spectra"""
    S, _, rows, _ = out.shape
    res = []
    for j in range(S):
        re = np.zeros((2, rows, 4096), np.float32)
        im = np.zeros((2, rows, 4096), np.float32)
        re[:, :, :2049] = out[j].real
        im[:, :, :2049] = out[j].imag
        res.append(oracle.istft(re, im))
    return np.stack(res)


def _compare(got, ref, tag, rel_rms=1e-4, max_rel=1e-3):
    peak = float(np.abs(ref).max())
    worst = 0.0
    for j in range(ref.shape[0]):
        rr = float(np.sqrt(np.mean((got[j] - ref[j]) ** 2)) / np.sqrt(np.mean(ref[j] ** 2)))
        ma = float(np.abs(got[j] - ref[j]).max()) / peak
        worst = max(worst, rr)
        print("%s stem %d: rel-rms %.3g, max-abs %.3g of peak" % (tag, j, rr, ma))
        assert rr <= rel_rms and ma <= max_rel, (tag, j, rr, ma)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("F,T,rows,iters", [(1024, 256, 3 * 256 + 100, 1), (1024, 256, 3 * 256 + 100, 2), (1536, 256, 256 + 77, 1)])
def test_istft_wiener_against_numpy_and_oracle(oracle, F, T, rows, iters):
    """srtIstftWiener on an oracle spectrum with seeded random masks: the stems against oracle.istft of the restatement's spectra, and the R tables
    of every iteration (srtCopyTensor "wiener_cov") against the restatement's.  Measured on MI355X, stems: rel-RMS 2.5e-7 / max-abs 3.7e-7 of the
    peak at n = 1 (both F), 4.5e-5 / 5.5e-5 at n = 2; the bounds asserted are 1e-4 / 1e-3."""
    import torch
    import spleeterrt_amd as srt
    S = 4
    n = rows * 1024 - 300
    L, R = _stereo_clip(n, 7 + F + iters)
    re, im = oracle.stft(L, R)
    assert re.shape[1] == rows
    nt = (rows + T - 1) // T
    rng = np.random.default_rng(11 + iters)
    masks = rng.random((S, nt, 2, T, F)).astype(np.float32)
    oob = (0.1, 0.0, 0.25, 1.0)
    eng = srt.Engine(F=F, T=T, stem_modes=(1, 0, 1, 1), oob_weights=oob, max_tiles=nt)
    spec_t = _spec_tensor(re, im)
    eng.set_timing(True)
    got = eng.istft_wiener(spec_t, torch.from_numpy(masks).cuda(), iters).cpu().numpy()
    ks = [k for _, k in eng.get_timing_kernels()]
    eng.set_timing(False)
    assert sum(k.startswith("srt_wiener_stats_kernel") for k in ks) == iters and sum(k.startswith("srt_wiener_finalize_kernel") for k in ks) == iters
    assert any(k.startswith("srt_wiener_filter_kernel") for k in ks), ks
    out, covs = wiener_np(_to_complex(spec_t), masks, T, F, iters, oob)
    _compare(got, _istft_of(oracle, out), "istft_wiener F=%d n=%d" % (F, iters))
    for it, (Rn, wsum, a) in enumerate(covs, 1):
        for j in range(S):
            Rg, wg, ag = eng.wiener_cov(j, it)
            assert abs(ag - a) <= 1e-6 * a
            Rref = np.stack([Rn[j, :, 0, 0].real, Rn[j, :, 1, 1].real, Rn[j, :, 0, 1].real, Rn[j, :, 0, 1].imag], 1)
            d = np.abs(Rg - Rref).max() / np.abs(Rref).max()
            assert d <= 1e-4, (it, j, d)
            wref = wsum[j] * a * a / 4096.0 ** 2                   # spectrum units
            assert np.abs(wg - wref).max() <= 1e-4 * np.abs(wref).max()
    with pytest.raises(srt.EngineError, match="wiener_cov"):
        eng.wiener_cov(0, iters + 1)
    eng.close()


def _separate_engine(coeffs, S, T, F, nt, precision, oob=None):
    import spleeterrt_amd as srt
    eng = srt.Engine(F=F, T=T, stem_modes=(1, 0, 1, 1, 0)[:S], oob_weights=oob, variant=srt.VARIANT_VST, max_tiles=nt, precision=precision)
    for s in range(S):
        eng.set_coeff(s, coeffs(s))
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("prec,S", [(0, 4), (1, 5)])
def test_separate_with_wiener_against_its_own_stages(oracle, coeffs, prec, S):
    """srtSeparate with the filter on, fp32 and fp16 (configs[4]: 5 stems), 3 tiles + a tail: the engine's own stft + forward outputs through
    the restatement and oracle.istft.  The new kernels ran inside the separation."""
    import torch
    T, F = 256, 1024
    rows = 3 * T + 40
    n = rows * 1024 - 100
    L, R = _stereo_clip(n, 21 + S)
    nt = (rows + T - 1) // T
    eng = _separate_engine(coeffs, S, T, F, nt, prec)
    eng.set_wiener(1)
    Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    eng.set_timing(True)
    got = eng.separate(Ld, Rd).cpu().numpy()
    ks = [k for _, k in eng.get_timing_kernels()]
    eng.set_timing(False)
    for kn in ("srt_wiener_stats_kernel", "srt_wiener_finalize_kernel", "srt_wiener_filter_kernel"):
        assert any(k.startswith(kn) for k in ks), (kn, ks)
    spec, mag = eng.stft(Ld, Rd)
    masks = eng.forward(mag).cpu().numpy()
    out, _ = wiener_np(_to_complex(spec), masks, T, F, 1, [0.1] * S)
    _compare(got, _istft_of(oracle, out), "separate prec=%d" % prec)
    eng.close()


@pytest.mark.gpu
def test_separate_with_wiener_at_the_bench_shape(oracle, coeffs):
    """64 tiles x 4 stems (bench shape): R accumulated over all 16384 rows chunk-wise in numpy, then two tiles' rows filtered and compared."""
    import torch
    T, F, S, nt = 256, 1024, 4, 64
    n = nt * T * 1024
    g = torch.Generator(device="cuda").manual_seed(5)
    Ld = (torch.rand(n, device="cuda", generator=g) - 0.5) * 0.2
    Rd = 0.6 * Ld + (torch.rand(n, device="cuda", generator=g) - 0.5) * 0.08
    eng = _separate_engine(coeffs, S, T, F, nt, 0)
    eng.set_wiener(1)
    got = eng.separate(Ld, Rd)
    spec, mag = eng.stft(Ld, Rd)
    masks = eng.forward(mag)
    rows = spec.shape[1]
    step = 2048

    def chunks_spec():
        for r in range(0, rows, step):
            yield _to_complex(spec[:, r:r + step])

    def chunks_masks():
        for r in range(0, rows, step):
            t0 = r // T
            yield _mask_rows(masks[:, t0:t0 + step // T].cpu().numpy(), step)
    tiles = (10, 41)
    sp = np.concatenate([_to_complex(spec[:, t * T:(t + 1) * T]) for t in tiles], 1)           # the filter is row-local: two tiles side by side
    mk = np.concatenate([masks[:, t:t + 1].cpu().numpy() for t in tiles], 1)
    out, _ = wiener_np(sp, mk, T, F, 1, [0.1] * S, stats_spec=chunks_spec(), stats_masks=chunks_masks())
    for i, t in enumerate(tiles):
        # rows [t T, (t + 1) T) alone shape output samples [t T 1024 + 3072, (t + 1) T 1024): compare there
        ref = _istft_of(oracle, out[:, :, i * T:(i + 1) * T])[:, :, 3072:T * 1024]
        g_ = got[:, :, t * T * 1024 + 3072:(t + 1) * T * 1024].cpu().numpy()
        _compare(g_, ref, "bench shape tile %d" % t)
    eng.close()


@pytest.mark.gpu
def test_wiener_stems_add_up_to_the_mixture(coeffs):
    """oob_weight = 1/S: sum over stems of the outputs = the input PCM on the interior (sum_j W_j = I - sqrt(eps) C^-1); raw masks miss by O(1).
    The regulariser sqrt(eps) a^2 I of C removes what a bin holds below ~sqrt(eps) of (max |x| / 10)^2 in power, so the bound needs a spectrum
    without a wide dynamic range: correlated stereo noise (MI355X: 8.7e-5 at n = 1, 1.3e-4 at n = 2; raw masks 0.26).  The panned-tone clip of the
    other tests misses by 1.9e-2 with random masks in the restatement itself."""
    import torch
    T, F, S, nt = 64, 512, 4, 3
    n = nt * T * 1024
    rng = np.random.default_rng(99)
    L = (0.1 * rng.standard_normal(n)).astype(np.float32)
    R = (0.6 * L + 0.05 * rng.standard_normal(n)).astype(np.float32)
    Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    eng = _separate_engine(coeffs, S, T, F, nt, 0, oob=[1.0 / S] * S)
    x = np.stack([L, R])[:, 4096:n - 4096]
    raw = eng.separate(Ld, Rd).cpu().numpy().sum(0)[:, 4096:n - 4096]
    for iters in (1, 2):
        eng.set_wiener(iters)
        mix = eng.separate(Ld, Rd).cpu().numpy().sum(0)[:, 4096:n - 4096]
        rr = float(np.sqrt(np.mean((mix - x) ** 2) / np.mean(x ** 2)))
        print("mixture consistency n=%d: rel-rms %.3g" % (iters, rr))
        assert rr <= 1e-3
    rr_raw = float(np.sqrt(np.mean((raw - x) ** 2) / np.mean(x ** 2)))
    print("raw masks: rel-rms %.3g" % rr_raw)
    assert rr_raw > 0.1
    eng.close()


@pytest.mark.gpu
def test_wiener_deterministic_graph_replay_and_off(coeffs):
    """Two calls give the same bits; a graph replay equals the eager call; changing the iteration count re-captures; srtSetWiener(e, 0) equals an
    engine that never called it."""
    import torch
    T, F, S, nt = 64, 512, 4, 3
    n = nt * T * 1024 - 5000
    L, R = _stereo_clip(n, 5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        plain = _separate_engine(coeffs, S, T, F, nt, 0)
        ref_off = plain.separate(Ld, Rd).cpu().numpy()
        plain.close()
        eng = _separate_engine(coeffs, S, T, F, nt, 0)
        eng.set_wiener(2)
        eng.set_wiener(0)
        assert np.array_equal(eng.separate(Ld, Rd).cpu().numpy(), ref_off)
        eager = {}
        for it in (1, 2):
            eng.set_wiener(it)
            a = eng.separate(Ld, Rd).cpu().numpy()
            b = eng.separate(Ld, Rd).cpu().numpy()
            assert np.array_equal(a, b), it
            assert not np.array_equal(a, ref_off)
            eager[it] = a
        assert not np.array_equal(eager[1], eager[2])
        out = torch.empty((S, 2, eng.L.srtIstftLength(eng.L.srtStftRows(n))), device="cuda")
        eng.set_graph_mode(True)
        for it in (1, 2, 1, 0):
            eng.set_wiener(it)
            for _ in range(2):                                          # capture, then replay
                out.fill_(float("nan"))
                eng.separate(Ld, Rd, out)
                assert np.array_equal(out.cpu().numpy(), eager[it] if it else ref_off), it
        eng.set_graph_mode(False)
        eng.close()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_wiener_refusals(coeffs):
    import torch
    import spleeterrt_amd as srt
    from spleeterrt_amd.capi import _Config
    from spleeterrt_amd import stream
    T, F, S = 64, 512, 2
    with pytest.raises(srt.EngineError, match="ratio_mask"):
        srt.Engine(F=F, T=T, stem_modes=(1, 0), ratio_mask=True, wiener=1)
    eng = srt.Engine(F=F, T=T, stem_modes=(1, 0), max_tiles=2)
    for bad in (4, -1):
        with pytest.raises(srt.EngineError, match="iterations must be 0"):
            eng.set_wiener(bad)
    eng.set_wiener(1)
    n = 4096 * 20
    L, R = _stereo_clip(n, 3)
    with pytest.raises(srt.EngineError, match="whole signal"):
        eng.separate_host_stream(L, R)
    Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for fn in (lambda: eng.separate_cli(Ld, Rd, 2), lambda: eng.separate_cli_host(L, R, 3)):
        with pytest.raises(srt.EngineError, match="Wiener filter does not apply to the CLI"):
            fn()
    with pytest.raises(ValueError, match="whole signal"):
        stream.separate_host_range(eng, L, R, rank=0, world=2)
    rcs = eng.L.srtIstftWiener(eng.h, None, 10, None, 1, None)
    assert rcs == -1
    eng.close()
    lib = srt.load_library()
    cfg = _Config()
    cfg.F, cfg.T, cfg.n_stems, cfg.variant, cfg.max_tiles = F, T, S, srt.VARIANT_VST, 2
    h = C.c_void_p()
    assert lib.srtMultiCreate(C.byref(cfg), (C.c_int * 1)(0), 1, C.byref(h)) == 0, lib.srtLastError()
    assert lib.srtSetWiener(lib.srtMultiEngine(h, 0), 1) == 0
    out = np.zeros((S, 2, lib.srtIstftLength(lib.srtStftRows(n))), np.float32)
    assert lib.srtMultiSeparateHost(h, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), 0) == -1
    assert b"whole signal" in lib.srtLastError()
    assert lib.srtMultiSeparateCliHost(h, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), n, 2, out.ctypes.data_as(C.c_void_p)) == -1
    lib.srtMultiDestroy(h)
