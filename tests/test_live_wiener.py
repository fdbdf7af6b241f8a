"""The multichannel Wiener filter in the live hop path (srtLiveCreateWiener, srtLiveWiener, srtLiveCopyTensor; spleeterrt_amd.Live(wiener=n)).

The yardstick is `restate_wiener`: test_live_mix.py's float64 restatement of the hop with, per run, test_wiener.wiener_np over the run's network window (zero rows
for frames before 0) and, per frame, the filtered spectra of the frame's row of that window in place of mask x spectrum.  Bins >= F keep oob_weight (or the row mean
of the fp32 masks under the average extension) times the input, and an output of a mix is the matrix row applied to the stems' spectra and the input.

Bounds: the project's bounds for the offline filter against numpy, test_wiener._compare (rel-RMS 1e-4 per plane, max-abs 1e-3 of the peak); the CPU properties use
test_wiener.py's 1e-3 of the peak for "up to the regulariser".  Every GPU case prints what it measured."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_live import HOP, PLUGIN_OOB, _Masks, asymmetric_window, live_schedule, mask_run, rel_rms
from test_live import restate_segments as plain_restate_segments
from test_live_mix import analyse, timeline
from test_wiener import _compare, wiener_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFT = 4096
T, F = 64, 512
SPEC_LD = 2052
KERNELS = ("srt_live_wiener_inverse_kernel<false>", "srt_live_wiener_inverse_kernel<true>")


# ---------------------------------------------------------------- restatement
def restate_wiener(spec, F, T, K, L, oob, masks_fn, iters, G_of=None, ext=False, runs=None):
    """per-hop output segments [hops][2P][1024] (float64) of a live stream with the filter.  spec [hops][2][2049]: analyse()'s frames; masks_fn(h_r, window
    [2][T][F] fp32 magnitudes) -> fp32 masks [S][2][T][F]; G_of(h) -> [P][S + 1], the matrix in force at hop h (None: every stem); runs: the runs already
    evaluated, h_r -> (masks, wiener_np's filtered window [S][2][T][2049], its covariances), shared between restatements of one input and iteration count"""
    _, sy = asymmetric_window()
    hops = spec.shape[0]
    S = len(oob)
    D, _ = live_schedule(K, L)
    mag = (np.abs(spec[:, :, :F]) * 4096.0).astype(np.float32)
    runs = {} if runs is None else runs

    def run_of(hr):
        if hr not in runs:
            X = np.zeros((2, T, 2049), complex)
            win = np.zeros((2, T, F), np.float32)
            for i in range(T):
                gg = hr - T + 1 + i
                if gg >= 0:
                    X[:, i] = spec[gg]
                    win[:, i] = mag[gg]
            m = np.asarray(masks_fn(hr, win), np.float32)
            out, covs = wiener_np(X, m[:, None], T, F, iters, oob)
            runs[hr] = (m, out, covs)
        return runs[hr]
    G0 = np.eye(S, S + 1) if G_of is None else np.asarray(G_of(D), np.float64)
    P = G0.shape[0]
    segs = np.zeros((hops, 2 * P, HOP))
    ov = np.zeros((P, 2, HOP))
    k = np.arange(1, 2048)
    for h in range(D, hops):
        g = h - D
        hr = mask_run(g, K, L)
        p = T - 1 - (hr - g)
        m, out, _ = run_of(hr)
        Y = out[:, :, p].copy()                           # [S][2][2049]: y_j below F, oob_weight x the input above
        if ext:
            Y[:, :, F:] = m[:, :, p].astype(np.float64).mean(axis=2)[:, :, None] * spec[g][None, :, F:]
        G = G0 if G_of is None else np.asarray(G_of(h), np.float64)
        for o in range(P):
            A = np.tensordot(G[o, :S], Y, axes=1) + G[o, S] * spec[g]
            AL, AR = A[0], A[1]
            z = np.zeros(FFT, complex)
            z[0] = AR[0].real + 1j * AL[0].real
            z[2048] = (AR[2048].real - AR[2048].imag) + 1j * (AL[2048].real - AL[2048].imag)
            z[k] = AR[k] + 1j * AL[k]
            z[FFT - k] = np.conj(AR[k]) + 1j * np.conj(AL[k])
            y = np.fft.fft(z)
            yL, yR = y.imag, y.real
            segs[h, 2 * o] = ov[o, 0] + yL[2048:3072] * sy[:1024]
            segs[h, 2 * o + 1] = ov[o, 1] + yR[2048:3072] * sy[:1024]
            ov[o, 0] = yL[3072:] * sy[1024:2048]
            ov[o, 1] = yR[3072:] * sy[1024:2048]
    return segs, runs


# ---------------------------------------------------------------- CPU
def _lib():
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


def test_abi_and_refusals():
    """the three prototypes and the Python surface; every refusal of srtLiveCreateWiener, and those of srtLiveCopyTensor that need no instance: -1, the function's
    name in the text, before any device call (this runs on a machine without a GPU).  srtLiveCopyTensor's refusals on a live instance are in test_tables_bit_for_bit."""
    import spleeterrt_amd as srt
    from spleeterrt_amd import capi
    L = _lib()
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "spleeterrt_amd.h")).read())
    assert ("SRT_API int srtLiveCreateWiener(const srt_config *cfg, int hops_per_run, int lookahead, const srt_live_opts *opts /* may be NULL */, "
            "int iterations, const void *const *h_coeff, srt_live **out);") in flat
    assert "SRT_API int srtLiveWiener(const srt_live *s);" in flat
    assert ("SRT_API int srtLiveCopyTensor(srt_live *s, const char *name, int stem, int index, float *h_dst, size_t max_floats, long long *run_hop);") in flat
    assert "the Wiener filter is never on" not in flat
    so = os.path.join(ROOT, "spleeterrt_amd", "libspleeterrt_amd.so")
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines()}
    assert {"srtLiveCreateWiener", "srtLiveWiener", "srtLiveCopyTensor"} <= exported
    assert isinstance(capi.Live.wiener, property) and hasattr(capi.Live, "tensor") and srt.Live is capi.Live

    blob = np.zeros(capi.COEFF_FLOATS, np.float32)
    good = np.array([[1.0, 0.0, 0.0]], np.float32)

    def create(F=512, T=64, S=2, K=4, Lk=0, max_tiles=1, blobs=None, fs=0, max_block=0, n_out=0, gain=None, ext=0, iters=1, ratio=0, opts=True):
        cfg = capi._Config()
        cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles, cfg.variant, cfg.ratio_mask = F, T, S, max_tiles, capi.VARIANT_VST, ratio
        for i in range(S if 0 < S <= capi.MAX_STEMS else 0):
            cfg.stem_mode[i], cfg.oob_weight[i] = 1, 0.25
        blobs = [blob.ctypes.data] * max(S, 1) if blobs is None else blobs
        o = capi._LiveOpts()
        o.sample_rate, o.max_block, o.n_out, o.mask_extension = fs, max_block, n_out, ext
        if gain is not None:
            o.h_gain = gain.ctypes.data_as(C.POINTER(C.c_float))
        h = C.c_void_p()
        rc = L.srtLiveCreateWiener(C.byref(cfg), K, Lk, C.byref(o) if opts else None, iters, (C.c_void_p * len(blobs))(*blobs), C.byref(h))
        return rc, L.srtLastError().decode(), h
    nan = good.copy()
    nan[0, 2] = np.nan
    cases = (
        # everything srtLiveCreateEx refuses, with the filter on and off
        ({"K": 0}, "hops_per_run"), ({"K": 65}, "hops_per_run"), ({"K": 4, "Lk": 61}, "lookahead"), ({"K": 4, "Lk": -1}, "lookahead"),
        ({"max_tiles": 2}, "max_tiles"), ({"blobs": [blob.ctypes.data, None]}, "null coefficient"), ({"F": 500}, "multiples of 64"),
        ({"T": 100}, "multiples of 64"), ({"S": 0}, "n_stems"), ({"S": 9}, "n_stems"), ({"K": 0, "iters": 0}, "hops_per_run"), ({"K": 0, "opts": False}, "hops_per_run"),
        ({"fs": 7999, "max_block": 480}, "8000..384000"), ({"fs": 384001, "max_block": 480}, "8000..384000"), ({"fs": 48000, "max_block": 0}, "max_block"),
        ({"fs": 48000, "max_block": 65537}, "max_block"),
        ({"n_out": -1, "gain": good}, "n_out"), ({"n_out": 9, "gain": good}, "n_out"), ({"n_out": 1}, "h_gain"), ({"n_out": 1, "gain": nan}, "finite"),
        ({"ext": 2}, "mask_extension"), ({"ext": -1, "iters": 0}, "mask_extension"),
        # its own
        ({"iters": -1}, "iterations"), ({"iters": 4}, "iterations"), ({"iters": 1, "ratio": 1}, "ratio"), ({"iters": 3, "ratio": 1, "opts": False}, "ratio"))
    for kw, text in cases:
        rc, msg, h = create(**kw)
        assert rc == -1 and text in msg and "srtLiveCreateWiener" in msg and not h.value, (kw, rc, msg)
    assert L.srtLiveCreateWiener(None, 4, 0, None, 1, None, None) == -1 and "srtLiveCreateWiener: null argument" in L.srtLastError().decode()
    assert L.srtLiveWiener(None) == 0
    buf = np.zeros(16, np.float32)
    hr = C.c_longlong(7)
    assert L.srtLiveCopyTensor(None, b"masks", 0, 0, C.c_void_p(buf.ctypes.data), buf.size, C.byref(hr)) == -1
    assert "srtLiveCopyTensor" in L.srtLastError().decode() and hr.value == 7
    assert L.srtLiveCopyTensor(None, None, 0, 0, None, 0, None) == -1 and "srtLiveCopyTensor" in L.srtLastError().decode()


def _random_masks(S, lo=0.0, hi=1.0):
    def fn(hr, win):
        return np.random.default_rng(1000 + hr).uniform(lo, hi, (S, 2, T, F)).astype(np.float32)
    return fn


def _noise(hops, seed):
    rng = np.random.default_rng(seed)
    n = hops * HOP
    return rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)


@pytest.mark.parametrize("K,Lk,iters", [(1, 0, 1), (4, 4, 2)])
def test_restatement_one_stem_passes_the_mixture(K, Lk, iters):
    """one stem with oob_weight 1: the filter passes the mixture whatever the mask, so the output is the input delayed by live_schedule's latency, up to the
    regulariser (test_wiener.py: 1e-3 of the peak)"""
    D, lat = live_schedule(K, Lk)
    hops = D + 10
    L, R = _noise(hops, 3)
    spec, _ = analyse(L, R, hops, F)
    segs, _ = restate_wiener(spec, F, T, K, Lk, (1.0,), _random_masks(1, 0.05, 0.95), iters)
    tl = timeline(segs)
    assert np.all(tl[:, :D * HOP] == 0) and np.all(np.isfinite(tl))
    n = hops * HOP
    for c, x in enumerate((L, R)):
        d = np.abs(tl[c, lat:] - x[:n - lat]).max()
        assert d <= 1e-3 * np.abs(x).max(), (c, d)


@pytest.mark.parametrize("K,Lk,iters", [(4, 4, 1), (7, 5, 3)])
def test_restatement_stems_sum_to_the_in_band_mixture(K, Lk, iters):
    """sum_j W_j = I - sqrt(eps) C^-1: with oob_weight 0 the stems add up to the mixture's bins below F (the plain restatement under unit masks), up to the regulariser"""
    S = 4
    D, _ = live_schedule(K, Lk)
    hops = D + 10
    L, R = _noise(hops, 4)
    spec, _ = analyse(L, R, hops, F)
    segs, runs = restate_wiener(spec, F, T, K, Lk, (0.0,) * S, _random_masks(S), iters)
    band, _ = plain_restate_segments(L, R, hops, F, T, K, Lk, (0.0,), lambda hr, w: np.ones((1, 2, T, F)))
    total = segs.reshape(hops, S, 2, HOP).sum(axis=1)
    peak = np.abs(band).max()
    assert peak > 1e-2 and np.abs(total - band).max() <= 1e-3 * peak
    # the all-ones row of a mix is that sum
    mix, _ = restate_wiener(spec, F, T, K, Lk, (0.0,) * S, _random_masks(S), iters, lambda h: np.array([[1.0, 1.0, 1.0, 1.0, 0.0]]), runs=runs)
    assert np.abs(mix - total).max() <= 1e-12 * peak


def test_restatement_disjoint_masks_route_each_bin_to_its_owner():
    """0/1 masks, each bin owned by one stem: the owner's output is the mixture in its bins and the others ~0, which is mask x spectrum - the plain restatement
    under the same masks - to O(sqrt(eps)) (test_wiener.py: 1e-3 of the peak)"""
    S, K, Lk = 3, 4, 4
    D, _ = live_schedule(K, Lk)
    hops = D + 10
    L, R = _noise(hops, 1)
    owner = np.random.default_rng(1).integers(0, S, F)
    m01 = np.zeros((S, 2, T, F), np.float32)
    for j in range(S):
        m01[j][:, :, owner == j] = 1.0
    spec, _ = analyse(L, R, hops, F)
    ref, _ = plain_restate_segments(L, R, hops, F, T, K, Lk, (0.0,) * S, lambda hr, w: m01)
    peak = np.abs(ref).max()
    for iters in (1, 2):
        segs, _ = restate_wiener(spec, F, T, K, Lk, (0.0,) * S, lambda hr, w: m01, iters)
        assert np.abs(segs - ref).max() <= 1e-3 * peak, iters


def test_restatement_zero_rows_and_silence():
    """a window that still holds frames before 0, and an all-silent input: finite everywhere, exactly zero for silence"""
    hops = 12
    spec, _ = analyse(np.zeros(hops * HOP), np.zeros(hops * HOP), hops, F)
    segs, _ = restate_wiener(spec, F, T, 1, 0, (0.25, 0.0), _random_masks(2), 2)
    assert np.all(segs == 0)


def test_kernel_resources():
    """srt_dsp.hip compiled with the resource remarks (test_live_mix.py::test_kernel_resources' recipe): both instantiations of the filtering hop inverse exist,
    without scratch or spilled VGPRs, inside the hop kernels' LDS budget"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the resource check needs the compiler the library is built with")
    src = os.path.join(ROOT, "spleeterrt_amd", "csrc", "srt_dsp.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + ROOT + "/include", "-I" + ROOT + "/spleeterrt_amd/csrc",
           "-Wno-pass-failed", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur, names = {}, None, []
    for line in err.splitlines():
        m = re.search(r"remark:\s+([^:]+): (\S+) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            names.append(v)
            cur = rows.setdefault(v, {})
        elif cur is not None:
            cur[k] = v
    dm = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    res = {re.sub(r"\(.*", "", d).replace("void ", ""): rows[n] for n, d in zip(names, dm)}
    assert sorted(k for k in res if k.startswith("srt_live_wiener")) == sorted(KERNELS)
    assert "srt_live_spec_gather_kernel" in res
    old = res["srt_live_inverse_kernel"]
    for k in KERNELS:
        a = res[k]
        print("%-44s vgpr %s sgpr %s scratch %s spilled vgprs %s occupancy %s lds %s" % (
            k, a["VGPRs"], a["TotalSGPRs"], a["ScratchSize [bytes/lane]"], a["VGPRs Spill"], a["Occupancy [waves/SIMD]"], a["LDS Size [bytes/block]"]))
        assert int(a["ScratchSize [bytes/lane]"]) == 0 and int(a["VGPRs Spill"]) == 0, (k, a)
        assert int(a["LDS Size [bytes/block]"]) == int(old["LDS Size [bytes/block]"]) and 2 * int(a["LDS Size [bytes/block]"]) <= 160 * 1024, (k, a)


# ---------------------------------------------------------------- GPU
MODES4 = (1, 1, 1, 1)


class _Case:
    """One config, schedule and input: the analysed frames, the mask engine, the restated runs per iteration count and the outputs of the filter instances without
    a mix, each evaluated once and shared by the tests that name the same case"""

    def __init__(self, oracle, coeffs, K, Lk, S=4, oob=PLUGIN_OOB, modes=MODES4, seed=31):
        import spleeterrt_amd as srt
        self.K, self.Lk, self.S, self.oob, self.modes = K, Lk, S, oob, modes
        self.D, self.lat = live_schedule(K, Lk)
        self.hops = self.D + max(3 * K, 24)
        self.n = self.hops * HOP
        self.L, self.R = oracle.synth_audio(self.n, seed + K, True)
        self.cs = [np.ascontiguousarray(coeffs(k)) for k in range(S)]
        self.masks = _Masks(F, T, modes, oob, srt.VARIANT_VST, srt.PREC_F32, self.cs)
        self.spec, _ = analyse(self.L, self.R, self.hops, F)
        self.runs, self.plain = {}, {}

    def live(self, iters, **kw):
        import spleeterrt_amd as srt
        return srt.Live(F, T, self.modes, self.oob, srt.VARIANT_VST, srt.PREC_F32, self.K, self.Lk, self.cs, wiener=iters, **kw)

    def restate(self, iters, G_of=None, ext=False):
        segs, _ = restate_wiener(self.spec, F, T, self.K, self.Lk, self.oob, self.masks, iters, G_of, ext, self.runs.setdefault(iters, {}))
        return timeline(segs)

    def no_mix(self, iters):
        """the planes [2S][n] a filter instance without a mix writes for 1024-sample calls"""
        if iters not in self.plain:
            live = self.live(iters)
            assert live.wiener == iters and live.outputs == self.S and live.latency == self.lat
            w, got = live.process(self.L, self.R)
            live.close()
            assert w.shape == got.shape == (2 * self.S, self.n)
            self.plain[iters] = got
        return self.plain[iters]

    def check(self, tag, got, ref):
        """the first D hops exactly zero, hop D carries signal, the rest inside test_wiener._compare's bounds"""
        assert np.all(np.isfinite(got))
        assert np.all(got[:, :self.D * HOP] == 0), "the first D hops must be silence"
        assert np.abs(got[:, self.D * HOP:(self.D + 1) * HOP]).max() > 1e-4, "hop D must carry signal"
        return _compare(got[:, self.D * HOP:].astype(np.float64), ref[:, self.D * HOP:], tag)


@pytest.fixture(scope="module")
def case(oracle, coeffs):
    cache = {}

    def get(K, Lk, **kw):
        key = (K, Lk) + tuple(sorted(kw.items()))
        if key not in cache:
            cache[key] = _Case(oracle, coeffs, K, Lk, **kw)
        return cache[key]
    yield get
    for c in cache.values():
        c.masks.eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K,Lk,iters,hops_past", [(4, 4, 2, T + 9), (1, 0, 1, 24)])
def test_tables_bit_for_bit(oracle, coeffs, K, Lk, iters, hops_past):
    """the tables of the run launched last are srtIstftWiener's on the gathered window and the run's masks, bit for bit; the window is the analysed frames (rotated
    and full at T + D + 9 hops, still holding zero frames at D + 24); srtLiveCopyTensor's refusals on a live instance"""
    import torch
    import spleeterrt_amd as srt
    D, _ = live_schedule(K, Lk)
    hops = D + hops_past
    n = hops * HOP
    L, R = oracle.synth_audio(n, 77, True)
    cs = [np.ascontiguousarray(coeffs(k)) for k in range(4)]
    live = srt.Live(F, T, MODES4, PLUGIN_OOB, srt.VARIANT_VST, srt.PREC_F32, K, Lk, cs, wiener=iters)
    assert live.wiener == iters
    none, hr0 = live.tensor("wiener_spec")
    assert none is None and hr0 == -1
    live.process(L, R)
    spec, hr = live.tensor("wiener_spec")
    assert hr == max(h for h in range(hops) if h % K == K - 1)
    masks = np.stack([live.tensor("masks", j)[0] for j in range(4)])
    assert all(live.tensor("masks", j)[1] == hr for j in range(4)) and masks.min() >= 0.0 and masks.max() <= 1.0 and masks.std() > 1e-3
    # the window against the float64 analysis, at test_live._check's bound
    ref, _ = analyse(L, R, hops, F)
    win = np.zeros((2, T, 2049), complex)
    for i in range(T):
        g = hr - T + 1 + i
        if g >= 0:
            win[:, i] = ref[g]
        else:
            assert np.all(spec[:, i] == 0), "frames before 0 are zero rows"
    assert (hr - T + 1 < 0) == (hops_past == 24)
    got = spec[:, :, :2049].astype(np.complex128)
    err = max(rel_rms(np.concatenate([got[c].real.ravel(), got[c].imag.ravel()]), np.concatenate([win[c].real.ravel(), win[c].imag.ravel()])) for c in range(2))
    peak = float(np.abs(got - win).max() / np.abs(win).max())
    print("K=%d L=%d window: rel-rms %.3g max/peak %.3g" % (K, Lk, err, peak))
    assert err <= 1e-4 and peak <= 1e-4
    eng = srt.Engine(F=F, T=T, stem_modes=MODES4, oob_weights=PLUGIN_OOB, variant=srt.VARIANT_VST, max_tiles=1)
    spec_t = torch.from_numpy(np.ascontiguousarray(spec).view(np.float32).reshape(2, T, SPEC_LD, 2)).cuda()
    eng.istft_wiener(spec_t, torch.from_numpy(np.ascontiguousarray(masks[:, None])).cuda(), iterations=iters)
    for it in range(1, iters + 1):
        for j in range(4):
            Rg, wg, ag = eng.wiener_cov(j, it)
            a, h2 = live.tensor("wiener_cov", j, it)
            assert h2 == hr and np.abs(Rg).max() > 0
            assert np.array_equal(a[:4 * F].reshape(F, 4), Rg) and np.array_equal(a[4 * F:5 * F], wg) and float(a[5 * F]) == ag, (it, j)
    eng.close()
    buf = np.zeros(5 * F + 1, np.float32)
    for name, stem, index, size in ((b"wiener_mean", 0, 1, buf.size), (b"wiener_cov", 0, 0, buf.size), (b"wiener_cov", 0, iters + 1, buf.size),
                                    (b"wiener_cov", 4, 1, buf.size), (b"wiener_cov", 0, 1, 5 * F), (b"masks", -1, 0, buf.size), (b"masks", 0, 0, buf.size),
                                    (b"wiener_spec", 0, 0, buf.size)):
        assert live.L.srtLiveCopyTensor(live.h, name, stem, index, C.c_void_p(buf.ctypes.data), size, None) == -1, (name, stem, index, size)
        assert b"srtLiveCopyTensor" in live.L.srtLastError()
    assert live.L.srtLiveCopyTensor(live.h, b"masks", 0, 0, None, 1 << 20, None) == -1 and b"srtLiveCopyTensor" in live.L.srtLastError()
    live.close()
    off = srt.Live(F, T, MODES4, PLUGIN_OOB, srt.VARIANT_VST, srt.PREC_F32, K, Lk, cs)
    assert off.wiener == 0
    with pytest.raises(srt.EngineError, match="srtLiveCopyTensor"):
        off.tensor("wiener_cov", 0, 1)
    with pytest.raises(srt.EngineError, match="srtLiveCopyTensor"):
        off.tensor("wiener_spec")
    off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K,Lk,iters", [(1, 0, 1), (4, 4, 1), (7, 5, 1), (64, 0, 1), (4, 4, 3)])
def test_samples_against_the_restatement(case, K, Lk, iters):
    """every stem of a filter instance against restate_wiener with the masks of a separate engine, max(3K, 24) hops past D.
    Measured on MI355X (worst plane: rel-RMS / max-abs of the peak): see DESIGN.md §18"""
    c = case(K, Lk)
    worst = c.check("live wiener K=%d L=%d n=%d" % (K, Lk, iters), c.no_mix(iters), c.restate(iters))
    print("K=%d L=%d n=%d worst rel-rms %.3g" % (K, Lk, iters, worst))


@pytest.mark.gpu
def test_two_stems_distinct_weights(case):
    c = case(4, 4, S=2, oob=(0.1, 0.3), modes=(0, 1))
    c.check("live wiener 2 stems", c.no_mix(1), c.restate(1))


class _RawLive:
    """a handle made through ctypes, driven through spleeterrt_amd.Live's methods"""

    def __new__(cls, handle, S):
        from spleeterrt_amd import capi
        live = object.__new__(capi.Live)
        live.L, live.h, live.S, live.F, live.T = _lib(), handle, S, F, T
        return live


@pytest.mark.gpu
def test_zero_iterations_is_live_create_ex(case):
    """iterations = 0 equals srtLiveCreateEx with the same options - none, and a mix with the average extension - bit for bit"""
    import spleeterrt_amd as srt
    from spleeterrt_amd import capi
    c = case(4, 4)
    G = np.array([[-1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.5, 2.0, -1.0, 0.0]], np.float32)
    for kw in ({"create_ex": True}, {"mix": G, "mask_extension": "average"}):
        ex = srt.Live(F, T, c.modes, c.oob, srt.VARIANT_VST, srt.PREC_F32, c.K, c.Lk, c.cs, **kw)
        _, a = ex.process(c.L, c.R, (300, 724, 1024, 512, 17))
        ex.close()
        cfg = capi._Config()
        cfg.F, cfg.T, cfg.n_stems, cfg.variant, cfg.max_tiles, cfg.impl, cfg.precision = F, T, 4, srt.VARIANT_VST, 1, capi.IMPL_MFMA, srt.PREC_F32
        for i in range(4):
            cfg.stem_mode[i], cfg.oob_weight[i] = 1, c.oob[i]
        o = capi._LiveOpts()
        if "mix" in kw:
            o.n_out, o.h_gain, o.mask_extension = 2, G.ctypes.data_as(C.POINTER(C.c_float)), capi.MASK_EXT_AVERAGE
        h = C.c_void_p()
        L = _lib()
        rc = L.srtLiveCreateWiener(C.byref(cfg), c.K, c.Lk, C.byref(o) if "mix" in kw else None, 0, (C.c_void_p * 4)(*[b.ctypes.data for b in c.cs]), C.byref(h))
        assert rc == 0, L.srtLastError()
        zero = _RawLive(h, 4)
        assert zero.wiener == 0 and zero.outputs == (2 if "mix" in kw else 4)
        _, b = zero.process(c.L, c.R, (300, 724, 1024, 512, 17))
        zero.close()
        assert np.abs(a).max() > 1e-3 and np.array_equal(a, b)


MIX3 = np.array([[-1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0]], np.float32)      # karaoke, one-hot (stem 2), dry


@pytest.mark.gpu
def test_mix_rows(case):
    """karaoke, one-hot and dry rows in one instance against the restatement; the one-hot row is that stem of the instance without a mix, bit for bit; the dry row
    is the delayed input"""
    c = case(4, 4)
    live = c.live(1, mix=MIX3)
    assert live.outputs == 3 and live.wiener == 1
    _, got = live.process(c.L, c.R)
    live.close()
    assert got.shape == (6, c.n)
    c.check("mix rows", got, c.restate(1, lambda h: MIX3))
    assert np.array_equal(got[2:4], c.no_mix(1)[4:6]), "a one-hot row must equal the stem of the no-mix instance"
    delayed = np.zeros((2, c.n))
    delayed[0, c.lat:], delayed[1, c.lat:] = c.L[:c.n - c.lat], c.R[:c.n - c.lat]
    _compare(got[4:, c.D * HOP:].astype(np.float64), delayed[:, c.D * HOP:], "dry row against the delayed input")


@pytest.mark.gpu
def test_set_mix_mid_stream(case):
    """1024-sample calls, the matrix replaced before call D + 6: the restatement with the matrix per hop"""
    c = case(4, 4)
    G0 = np.array([[-1.0, 0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    G1 = np.array([[0.0, 0.5, 2.0, -1.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0]], np.float32)
    sw = c.D + 6
    live = c.live(1, mix=G0)
    parts = [live.process(c.L[:sw * HOP], c.R[:sw * HOP])[1]]
    live.set_mix(G1)
    parts.append(live.process(c.L[sw * HOP:], c.R[sw * HOP:])[1])
    live.close()
    got = np.concatenate(parts, axis=1)
    ref = c.restate(1, lambda h: G0 if h < sw else G1)
    assert np.abs(ref[:, sw * HOP:] - c.restate(1, lambda h: G0)[:, sw * HOP:]).max() > 1e-3, "the change must be audible in the restatement"
    c.check("set_mix before call D+6", got, ref)


@pytest.mark.gpu
def test_average_extension(case):
    """mask_extension = "average" under the filter: bins >= F follow the masks' row means, not the filter"""
    c = case(4, 4)
    ref = c.restate(1, ext=True)
    assert np.abs(ref - c.restate(1)).max() > 1e-4 * np.abs(ref).max(), "the extension must change the stems on this input"
    live = c.live(1, mask_extension="average")
    assert live.outputs == 4
    _, got = live.process(c.L, c.R)
    live.close()
    c.check("average extension", got, ref)


@pytest.mark.gpu
def test_chunking_and_determinism(case):
    """the samples written do not depend on how the input is cut into calls, two instances agree bit for bit, and silence in gives finite silence out"""
    c = case(4, 4)
    outs = []
    for chunks in ((1024,), (17, 300, 724, 1024)):
        live = c.live(2)
        w, _ = live.process(c.L, c.R, chunks)
        live.close()
        outs.append(w)
    m = min(outs[0].shape[1], outs[1].shape[1])
    assert m > c.n - 2 * HOP and np.abs(outs[0]).max() > 1e-3 and np.array_equal(outs[0][:, :m], outs[1][:, :m])
    assert np.array_equal(outs[0], c.no_mix(2)), "two instances fed the same input must give the same bits"
    live = c.live(2)
    z = np.zeros(c.n, np.float32)
    _, got = live.process(z, z)
    live.close()
    assert np.all(np.isfinite(got)) and np.all(got == 0)


@pytest.mark.gpu
def test_rate_instance(case):
    """fs = 48000 with the filter: every call writes its n samples, and the bits do not depend on the call sizes"""
    c = case(4, 4)
    outs = []
    for chunks in ((480,), (1, 100, 379)):
        live = c.live(1, sample_rate=48000, max_block=480)
        assert live.outputs == 4 and live.wiener == 1
        w, tl = live.process(c.L, c.R, chunks)
        live.close()
        assert w.shape == (8, c.n) and np.array_equal(w, tl)
        outs.append(tl)
    assert np.all(np.isfinite(outs[0])) and np.abs(outs[0]).max() > 1e-3 and np.array_equal(outs[0], outs[1])
