"""The stem remix and the average mask extension in the live hop (srtLiveCreateEx, srtLiveSetMix, srtLiveOutputs; spleeterrt_amd.Live(mix=...,
mask_extension=...)).

The yardstick is test_live.py's float64 restatement of the hop with the gain of output m formed as the kernel forms it: h = G[m][S], then
h = fl32(G[m][s] * g_s + h) for s ascending on the fp32 gains (test_mix.chain32), g_s = the fp32 mask value below F and oob_weight[s] above it, or under
the average extension the float64 mean of the row's fp32 gains.  Everything after the gain (the product with the spectrum, the transform, the window, the
overlap-add) is float64.

Bound, none of it taken from what the new kernel gives.  Every GPU case has a mix-off, constant-rule Live of the same config and input (the kernel the
project had before: srt_live_inverse_kernel) held against the restatement first:
    b_off = max over stems s of max|err_s| / peak_s        (peak_s: peak of the restated stem)
Output m of the code under test is an inverse transform of the same kind on a spectrum scaled by |G|, so its error must stay within
    MARGIN x b_off x scale_m,   scale_m = sum_s |G[m][s]| peak_s + |G[m][S]| peak_dry,   MARGIN = 4
(the project's MARGIN: the same fp32 transform with other contraction choices), peaks of the restated stem and dry streams, and - the outer cap -
within test_live._check's 1e-4 of that same scale.  Both figures are printed by every case."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_live import HOP, _Masks, account, asymmetric_window, live_schedule, mask_run, rel_rms
from test_live import restate_segments as plain_restate_segments
from test_mix import chain32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFT = 4096
T, F = 64, 512
MARGIN = 4.0
CAP = 1e-4
OOB4 = (0.25, 0.0, 0.25, 0.25)
OOB3 = (1.0, 0.0, 0.25)                                # distinct weights for the mixes
KERNELS = ("srt_live_combine_inverse_kernel<false>", "srt_live_combine_inverse_kernel<true>")


# ---------------------------------------------------------------- restatement
def analyse(L_in, R_in, hops, F):
    """spectra [hops][2][2049] (float64) and network magnitudes [hops][2][F] (fp32) of the hop frames, as test_live.restate_segments forms them"""
    an, _ = asymmetric_window()
    x = np.zeros((2, hops * HOP + FFT))
    nin = min(L_in.size, hops * HOP)
    x[0, FFT - HOP:FFT - HOP + nin] = L_in[:nin]
    x[1, FFT - HOP:FFT - HOP + nin] = R_in[:nin]
    spec = np.empty((hops, 2, 2049), complex)
    for g in range(hops):
        spec[g] = 2.0 * np.conj(np.fft.fft(x[:, g * HOP:g * HOP + FFT] * an, axis=1)[:, :2049])
    return spec, (np.abs(spec[:, :, :F]) * 4096.0).astype(np.float32)


def restate_mix(spec, mag, F, T, K, Lk, oob, masks_fn, G_of, ext=False, runs=None):
    """per-hop output segments [hops][2P][1024]: test_live.restate_segments with a matrix per hop.  G_of(h) -> [P][S + 1], the matrix in force at hop h;
    masks_fn(h_r, window [2][T][F] fp32) -> fp32 masks [S][2][T][F]; runs: the masks of the runs already evaluated (shared between restatements)"""
    _, sy = asymmetric_window()
    hops = spec.shape[0]
    S = len(oob)
    D, _ = live_schedule(K, Lk)
    runs = {} if runs is None else runs

    def masks_of(hr):
        if hr not in runs:
            win = np.zeros((2, T, F), np.float32)
            for i in range(T):
                gg = hr - T + 1 + i
                if gg >= 0:
                    win[:, i] = mag[gg]
            runs[hr] = np.asarray(masks_fn(hr, win), np.float32)
        return runs[hr]
    P = np.asarray(G_of(D)).shape[0]
    segs = np.zeros((hops, 2 * P, HOP))
    ov = np.zeros((P, 2, HOP))
    k = np.arange(1, 2048)
    for h in range(D, hops):
        g = h - D
        hr = mask_run(g, K, Lk)
        m = masks_of(hr)[:, :, T - 1 - (hr - g)]      # [S][2][F] fp32
        gains = np.empty((S, 2, 2049), np.float32)
        gains[:, :, :F] = m
        if ext:
            gains[:, :, F:] = m.astype(np.float64).mean(axis=2)[:, :, None]
        else:
            gains[:, :, F:] = np.asarray(oob, np.float32)[:, None, None]
        G = np.asarray(G_of(h), np.float32)
        for o in range(P):
            A = spec[g] * chain32(G[o], gains).astype(np.float64)
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


def stems_and_dry(S):
    """the matrix whose outputs are the S stems and then the unmasked input"""
    return np.eye(S + 1, dtype=np.float32)


def timeline(segs):
    """1024-sample calls: [2P][hops * 1024]"""
    return segs.transpose(1, 0, 2).reshape(segs.shape[1], -1)


# ---------------------------------------------------------------- CPU
def _lib():
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


def test_abi_and_refusals():
    """the three prototypes, srt_live_opts' layout, the Python surface and every refusal that needs no instance: -1, the function's name in the text, before
    any device call (this runs on a machine without a GPU).  srtLiveSetMix's refusals on a live instance are in test_set_mix_mid_stream."""
    import spleeterrt_amd as srt
    from spleeterrt_amd import capi
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "spleeterrt_amd.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("SRT_API int srtLiveCreateEx(const srt_config *cfg, int hops_per_run, int lookahead, const srt_live_opts *opts, "
            "const void *const *h_coeff, srt_live **out);") in flat
    assert "SRT_API int srtLiveSetMix(srt_live *s, const float *h_gain);" in flat
    assert "SRT_API int srtLiveOutputs(const srt_live *s);" in flat
    so = os.path.join(ROOT, "spleeterrt_amd", "libspleeterrt_amd.so")
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines()}
    assert {"srtLiveCreateEx", "srtLiveSetMix", "srtLiveOutputs"} <= exported
    body = re.search(r"typedef struct srt_live_opts \{(.*?)\} srt_live_opts;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(int|const float \*)\s*(\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in capi._LiveOpts._fields_] == ["sample_rate", "max_block", "n_out", "h_gain", "mask_extension"]
    for (ct, n), (_, pt) in zip(fields, capi._LiveOpts._fields_):
        assert (pt is C.c_int) == (ct == "int") and (pt is C.c_int or pt is C.POINTER(C.c_float)), n
    assert C.sizeof(capi._LiveOpts) == 32 and capi._LiveOpts.h_gain.offset == 16 and capi._LiveOpts.mask_extension.offset == 24
    assert hasattr(capi.Live, "set_mix") and isinstance(capi.Live.outputs, property) and srt.Live is capi.Live

    blob = np.zeros(capi.COEFF_FLOATS, np.float32)
    good = np.array([[1.0, 0.0, 0.0]], np.float32)

    def create(F=512, T=64, S=2, K=4, Lk=0, max_tiles=1, blobs=None, fs=0, max_block=0, n_out=0, gain=None, ext=0):
        cfg = capi._Config()
        cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles, cfg.variant = F, T, S, max_tiles, capi.VARIANT_VST
        for i in range(S if 0 < S <= capi.MAX_STEMS else 0):
            cfg.stem_mode[i], cfg.oob_weight[i] = 1, 0.25
        blobs = [blob.ctypes.data] * max(S, 1) if blobs is None else blobs
        o = capi._LiveOpts()
        o.sample_rate, o.max_block, o.n_out, o.mask_extension = fs, max_block, n_out, ext
        if gain is not None:
            o.h_gain = gain.ctypes.data_as(C.POINTER(C.c_float))
        h = C.c_void_p()
        rc = L.srtLiveCreateEx(C.byref(cfg), K, Lk, C.byref(o), (C.c_void_p * len(blobs))(*blobs), C.byref(h))
        return rc, L.srtLastError().decode(), h
    nan, inf = good.copy(), np.tile(good, (2, 1))
    nan[0, 2] = np.nan
    inf[1, 0] = np.inf
    cases = (
        # everything srtLiveCreate refuses
        ({"K": 0}, "hops_per_run"), ({"K": 65}, "hops_per_run"), ({"K": 4, "Lk": 61}, "lookahead"), ({"K": 4, "Lk": -1}, "lookahead"),
        ({"max_tiles": 2}, "max_tiles"), ({"blobs": [blob.ctypes.data, None]}, "null coefficient"), ({"F": 500}, "multiples of 64"),
        ({"T": 100}, "multiples of 64"), ({"S": 0}, "n_stems"), ({"S": 9}, "n_stems"),
        # ... and srtLiveCreateRate
        ({"fs": 7999, "max_block": 480}, "8000..384000"), ({"fs": 384001, "max_block": 480}, "8000..384000"), ({"fs": 48000, "max_block": 0}, "max_block"),
        ({"fs": 48000, "max_block": 65537}, "max_block"), ({"fs": 48000, "max_block": 480, "K": 0}, "hops_per_run"),
        # the options
        ({"n_out": -1, "gain": good}, "n_out"), ({"n_out": 9, "gain": good}, "n_out"), ({"n_out": 1}, "h_gain"), ({"n_out": 1, "gain": nan}, "finite"),
        ({"n_out": 2, "gain": inf}, "finite"), ({"ext": 2}, "mask_extension"), ({"ext": -1}, "mask_extension"),
        ({"n_out": 1, "gain": good, "ext": 7, "fs": 48000, "max_block": 480}, "mask_extension"))
    for kw, text in cases:
        rc, msg, h = create(**kw)
        assert rc == -1 and text in msg and "srtLiveCreateEx" in msg and not h.value, (kw, rc, msg)
    assert L.srtLiveCreateEx(None, 4, 0, None, None, None) == -1 and "srtLiveCreateEx: null argument" in L.srtLastError().decode()
    assert L.srtLiveSetMix(None, C.c_void_p(good.ctypes.data)) == -1 and "srtLiveSetMix" in L.srtLastError().decode()
    assert L.srtLiveSetMix(None, None) == -1 and "srtLiveSetMix" in L.srtLastError().decode()
    assert L.srtLiveOutputs(None) == 0


def _random_masks(S):
    def fn(hr, win):
        return np.random.default_rng(1000 + hr).uniform(0.0, 1.0, (S, 2, T, F)).astype(np.float32)
    return fn


@pytest.mark.parametrize("K,Lk", [(1, 0), (4, 4), (7, 5)])
def test_restatement_properties(K, Lk):
    """one-hot rows reproduce test_live.restate_segments' stems (the chain gives g_s exactly); the row (0, .., 0, 1) is the input delayed by
    live_schedule's latency to 1e-9; the average extension of constant masks is that constant"""
    S, oob = 3, (0.5, 0.0, 0.25)                        # weights that are fp32 values
    D, lat = live_schedule(K, Lk)
    hops = D + 10
    n = hops * HOP
    rng = np.random.default_rng(3)
    L, R = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    spec, mag = analyse(L, R, hops, F)
    fn = _random_masks(S)
    segs, runs = restate_mix(spec, mag, F, T, K, Lk, oob, fn, lambda h: stems_and_dry(S))
    ref, _ = plain_restate_segments(L, R, hops, F, T, K, Lk, oob, fn)
    assert np.abs(ref).max() > 1e-2
    assert np.abs(segs[:, :2 * S] - ref).max() <= 1e-12 * np.abs(ref).max()
    tl = timeline(segs)
    assert np.all(tl[:, :D * HOP] == 0)
    for c, x in enumerate((L, R)):
        assert np.abs(tl[2 * S + c, lat:] - x[:n - lat]).max() <= 1e-9
    # a matrix that changes mid-stream: hops before the change are those of the old matrix, hops after the cross-fade hop those of the new one
    G0, G1 = np.array([[1.0, 0.0, 0.0, 0.0]]), np.array([[0.0, 0.0, 0.0, 1.0]])
    sw, _ = restate_mix(spec, mag, F, T, K, Lk, oob, fn, lambda h: G0 if h < D + 4 else G1, runs=runs)
    assert np.array_equal(sw[:D + 4, :2], segs[:D + 4, :2]) and np.abs(sw[D + 5:, :2] - segs[D + 5:, 2 * S:]).max() <= 1e-12
    assert not np.array_equal(sw[D + 4, :2], segs[D + 4, :2]) and not np.array_equal(sw[D + 4, :2], segs[D + 4, 2 * S:])
    half, _ = restate_mix(spec, mag, F, T, K, Lk, (0.9, 0.9), lambda hr, w: np.full((2, 2, T, F), 0.5, np.float32), lambda h: stems_and_dry(2), ext=True)
    th = timeline(half)
    for j in range(4):
        assert np.abs(th[j, lat:] - 0.5 * (L, R)[j % 2][:n - lat]).max() <= 1e-9


def test_kernel_resources():
    """srt_dsp.hip compiled with the resource remarks (tests/test_mix.py::test_mix_kernels_resources' recipe): both instantiations of the combining hop
    inverse exist, without scratch or spilled VGPRs, at two waves per SIMD or more, inside the hop kernels' LDS budget (two workgroups per CU)"""
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
    assert sorted(k for k in res if k.startswith("srt_live_combine")) == sorted(KERNELS)
    old = res["srt_live_inverse_kernel"]
    for k in KERNELS:
        a = res[k]
        print("%-44s vgpr %s sgpr %s scratch %s spilled vgprs %s occupancy %s lds %s" % (
            k, a["VGPRs"], a["TotalSGPRs"], a["ScratchSize [bytes/lane]"], a["VGPRs Spill"], a["Occupancy [waves/SIMD]"], a["LDS Size [bytes/block]"]))
        assert int(a["ScratchSize [bytes/lane]"]) == 0 and int(a["VGPRs Spill"]) == 0, (k, a)
        assert int(a["Occupancy [waves/SIMD]"]) >= 2, (k, a)
        assert int(a["LDS Size [bytes/block]"]) == int(old["LDS Size [bytes/block]"]) and 2 * int(a["LDS Size [bytes/block]"]) <= 160 * 1024, (k, a)


# ---------------------------------------------------------------- GPU
class _Case:
    """One config and input: the mix-off, constant-rule Live held against the restatement (b_off), and what the cases under test share with it - the
    analysed frames, the evaluated runs' masks, the restated stem and dry streams with their peaks"""

    def __init__(self, oracle, coeffs, S, oob, K, Lk, ratio=False, seed=7, noise=False):
        import spleeterrt_amd as srt
        self.S, self.oob, self.K, self.Lk, self.ratio = S, oob, K, Lk, ratio
        self.modes = (1,) * S
        self.D, self.lat = live_schedule(K, Lk)
        self.hops = self.D + 16
        self.n = self.hops * HOP
        if noise:
            rng = np.random.default_rng(seed)
            self.L, self.R = (rng.uniform(-0.5, 0.5, self.n).astype(np.float32) for _ in range(2))
        else:
            self.L, self.R = oracle.synth_audio(self.n, seed, True)
        self.cs = [np.ascontiguousarray(coeffs(k)) for k in range(S)]
        self.masks = _Masks(F, T, self.modes, oob, srt.VARIANT_VST, srt.PREC_F32, self.cs, ratio)
        self.spec, self.mag = analyse(self.L, self.R, self.hops, F)
        segs, self.runs = restate_mix(self.spec, self.mag, F, T, K, Lk, oob, self.masks, lambda h: stems_and_dry(S))
        self.ref = timeline(segs)                      # [2S + 2][n]: the stems, then the dry stream
        self.peaks = self.peaks_of(self.ref)
        live = self.live()
        assert live.outputs == S
        _, got = live.process(self.L, self.R)
        live.close()
        self.off = got
        self.b_off = max(float(np.abs(got[2 * s:2 * s + 2] - self.ref[2 * s:2 * s + 2]).max()) / self.peaks[s] for s in range(S))
        print("mix off: b_off %.3g, worst rel-rms %.3g" % (self.b_off, max(rel_rms(got[j], self.ref[j]) for j in range(2 * S))))
        assert 0.0 < self.b_off <= CAP

    @staticmethod
    def peaks_of(ref):
        return [float(np.abs(ref[2 * s:2 * s + 2]).max()) for s in range(ref.shape[0] // 2)]

    def live(self, **kw):
        import spleeterrt_amd as srt
        return srt.Live(F, T, self.modes, self.oob, srt.VARIANT_VST, srt.PREC_F32, self.K, self.Lk, self.cs, ratio_mask=self.ratio, **kw)

    def restate(self, G_of, ext=False):
        segs, _ = restate_mix(self.spec, self.mag, F, T, self.K, self.Lk, self.oob, self.masks, G_of, ext, self.runs)
        return timeline(segs)

    def within(self, tag, got, ref, Gabs, peaks=None):
        """every output m of got [2P][n] within MARGIN x b_off x scale_m (and the cap) of ref; Gabs [P][S + 1]: |G|, its largest value per entry when it changes"""
        peaks = self.peaks if peaks is None else peaks
        worst = 0.0
        for m in range(got.shape[0] // 2):
            scale = float(np.dot(np.abs(Gabs[m]), peaks))
            err = float(np.abs(got[2 * m:2 * m + 2] - ref[2 * m:2 * m + 2]).max())
            worst = max(worst, err / (MARGIN * self.b_off * scale))
            print("%s output %d: err %.3g, MARGIN x b_off x scale %.3g (b_off %.3g, scale %.3g), ratio %.3g" % (
                tag, m, err, MARGIN * self.b_off * scale, self.b_off, scale, err / (MARGIN * self.b_off * scale)))
            assert err <= MARGIN * self.b_off * scale and err <= CAP * scale, (tag, m, err, self.b_off, scale)
        print("%s: b_off %.3g worst ratio to the bound %.3g" % (tag, self.b_off, worst))
        return worst


@pytest.fixture(scope="module")
def case(oracle, coeffs):
    """the cases of this module, each built once (its mix-off run, its restatement, its mask engine) and shared by the tests that name the same config"""
    cache = {}

    def get(S, oob, K, Lk, ratio=False, seed=7, noise=False):
        key = (S, oob, K, Lk, ratio, seed, noise)
        if key not in cache:
            cache[key] = _Case(oracle, coeffs, S, oob, K, Lk, ratio, seed, noise)
        return cache[key]
    yield get
    for c in cache.values():
        c.masks.eng.close()


@pytest.mark.gpu
def test_zero_options_are_the_old_calls(oracle, coeffs):
    """srtLiveCreateEx with all-zero options is srtLiveCreate, and with only sample_rate / max_block srtLiveCreateRate, bit for bit"""
    import spleeterrt_amd as srt
    K, Lk = 4, 4
    D, _ = live_schedule(K, Lk)
    n = (D + 16) * HOP
    L, R = oracle.synth_audio(n, 21, True)
    cs = [np.ascontiguousarray(coeffs(k)) for k in range(4)]
    outs = []
    for kw in ({}, {"create_ex": True}):
        live = srt.Live(F, T, (1, 1, 1, 1), OOB4, srt.VARIANT_VST, srt.PREC_F32, K, Lk, cs, **kw)
        assert live.outputs == 4
        outs.append(live.process(L, R, (300, 724, 1024, 512, 17)))
        live.close()
    assert np.abs(outs[0][0]).max() > 1e-3
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    outs = []
    for kw in ({}, {"create_ex": True}):
        live = srt.Live(F, T, (1, 1, 1, 1), OOB4, srt.VARIANT_VST, srt.PREC_F32, K, Lk, cs, sample_rate=48000, max_block=480, **kw)
        assert live.outputs == 4
        outs.append((live.latency, live.process(L, R, (480,))[1]))
        live.close()
    assert outs[0][0] == outs[1][0] and np.abs(outs[0][1]).max() > 1e-3 and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("K,Lk", [(1, 0), (4, 4), (7, 5)])
def test_identity(case, K, Lk):
    """n_out = S = 4 with the identity: every stem within the bound; the first D hops are silence and hop D carries signal"""
    c = case(4, OOB4, K, Lk)
    G = np.eye(4, 5, dtype=np.float32)
    live = c.live(mix=G)
    assert live.outputs == 4 and live.latency == c.lat
    w, got = live.process(c.L, c.R)
    live.close()
    assert w.shape == got.shape == (8, c.n)
    assert np.all(got[:, :c.D * HOP] == 0), "the first D hops must be silence"
    assert np.abs(got[:, c.D * HOP:(c.D + 1) * HOP]).max() > 1e-4, "hop D must carry signal"
    c.within("identity K=%d L=%d" % (K, Lk), got, c.ref[:8], G)


MIXES3 = np.array([[-1.0, 0.0, 0.0, 1.0], [0.5, 2.0, -1.0, 0.0], [0.0, 0.0, 0.0, 1.0]], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [False, True])
def test_mixes(case, ratio):
    """three stems with distinct weights above F, three outputs in one instance: karaoke, a general row, and the dry row (= the delayed input)"""
    c = case(3, OOB3, 4, 4, ratio=ratio)
    live = c.live(mix=MIXES3)
    assert live.outputs == 3
    _, got = live.process(c.L, c.R)
    live.close()
    assert got.shape == (6, c.n) and np.abs(got[:2]).max() > 1e-3
    c.within("mixes ratio=%d" % ratio, got, c.restate(lambda h: MIXES3), MIXES3)
    delayed = np.zeros((2, c.n))
    delayed[0, c.lat:], delayed[1, c.lat:] = c.L[:c.n - c.lat], c.R[:c.n - c.lat]
    c.within("dry row against the delayed input", got[4:], delayed, MIXES3[2:])


@pytest.mark.gpu
def test_average_extension_of_constant_masks():
    """all-zero weights (VST: every mask exactly 0.5), mix off, oob_weight 0.9, the average extension: e = 0.5, so every stem is 0.5 x the input delayed by
    srtLiveLatency() to 1e-5 of the peak (test_live.test_live_latency_measured's form) - 0.9 x above F would miss it by far"""
    import spleeterrt_amd as srt
    from spleeterrt_amd import capi
    K, Lk = 4, 4
    zero = np.zeros(capi.COEFF_FLOATS, np.float32)
    live = srt.Live(F, T, (1, 0), (0.9, 0.9), srt.VARIANT_VST, srt.PREC_F32, K, Lk, [zero, zero], mask_extension="average")
    assert live.outputs == 2
    lat = live.latency
    D, _ = live_schedule(K, Lk)
    n = (D + 16) * HOP
    rng = np.random.default_rng(404)
    L = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    R = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    _, got = live.process(L, R)
    live.close()
    peak = max(np.abs(L).max(), np.abs(R).max()) * 0.5
    for j in range(4):
        d = float(np.abs(got[j, lat:] - 0.5 * (L, R)[j % 2][:n - lat]).max())
        print("plane %d: max |got - 0.5 x| = %.3g (peak %.3g)" % (j, d, peak))
        assert d <= 1e-5 * peak, (j, d)
    assert np.all(got[:, :lat - HOP] == 0) and lat == (Lk + 2 * K) * HOP + HOP


def _energy_above(x, F):
    X = np.abs(np.fft.rfft(np.asarray(x, np.float64))) ** 2
    edge = int(round(F * x.size / FFT))                 # bin F of the 4096-point transform on this length's grid
    return float(X[edge:].sum() / X.sum())


@pytest.mark.gpu
def test_average_extension_real_weights(case):
    """mix off with the average extension on noise that has most of its energy above F: every stem within the bound of the restatement"""
    c = case(4, OOB4, 4, 4, seed=11, noise=True)
    assert min(_energy_above(c.L, F), _energy_above(c.R, F)) >= 0.10
    ref = c.restate(lambda h: stems_and_dry(4), ext=True)
    assert np.abs(ref[:8] - c.ref[:8]).max() > 1e-2 * max(c.peaks), "the extension must change the stems on this input"
    live = c.live(mask_extension="average")
    assert live.outputs == 4
    _, got = live.process(c.L, c.R)
    live.close()
    assert np.all(got[:, :c.D * HOP] == 0) and np.abs(got[:, c.D * HOP:(c.D + 1) * HOP]).max() > 1e-4
    c.within("average extension", got, ref[:8], np.eye(4, 5), c.peaks_of(ref))


@pytest.mark.gpu
def test_average_extension_ratio_stems_sum_to_the_input(case):
    """ratio_mask + the average extension: the gains sum to 1 in every bin of the whole band, so the row (-1, -1, -1 | 1) is silence within the bound"""
    c = case(3, OOB3, 4, 4, ratio=True, seed=11, noise=True)
    G = np.array([[-1.0, -1.0, -1.0, 1.0]], np.float32)
    ref = c.restate(lambda h: stems_and_dry(3), ext=True)
    live = c.live(mix=G, mask_extension="average")
    _, got = live.process(c.L, c.R)
    live.close()
    assert got.shape == (2, c.n)
    c.within("input minus the stems", got, np.zeros_like(got, np.float64), G, c.peaks_of(ref))
    # the same instance without the extension keeps oob_weight (1 + 0 + 0.25) x the band above F: far from silence
    live = c.live(mix=G)
    _, con = live.process(c.L, c.R)
    live.close()
    assert np.abs(con).max() > 1e-2 * c.peaks[3]


@pytest.mark.gpu
def test_set_mix_mid_stream(case):
    """1024-sample calls, the matrix replaced before call D + 6: the restatement with the matrix per hop (the overlap-add cross-fades the two); a refused
    srtLiveSetMix leaves the matrix in force; srtLiveSetMix's refusals on a live instance"""
    import spleeterrt_amd as srt
    c = case(4, OOB4, 4, 4)
    G0 = np.array([[-1.0, 0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    G1 = np.array([[0.0, 0.5, 2.0, -1.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0]], np.float32)
    sw = c.D + 6
    live = c.live(mix=G0)
    assert live.outputs == 2
    parts = [live.process(c.L[:sw * HOP], c.R[:sw * HOP])[1]]
    live.set_mix(G1)
    mid = (sw + 4) * HOP
    parts.append(live.process(c.L[sw * HOP:mid], c.R[sw * HOP:mid])[1])
    bad = G0.copy()
    bad[1, 2] = np.nan
    with pytest.raises(srt.EngineError, match="srtLiveSetMix"):
        live.set_mix(bad)
    assert live.L.srtLiveSetMix(live.h, None) == -1 and b"srtLiveSetMix" in live.L.srtLastError()
    with pytest.raises(ValueError):
        live.set_mix(G0[:1])
    parts.append(live.process(c.L[mid:], c.R[mid:])[1])
    live.close()
    got = np.concatenate(parts, axis=1)
    ref = c.restate(lambda h: G0 if h < sw else G1)
    assert np.abs(ref[:, sw * HOP:] - c.restate(lambda h: G0)[:, sw * HOP:]).max() > 1e-3, "the change must be audible in the restatement"
    c.within("set_mix before call D+6", got, ref, np.maximum(np.abs(G0), np.abs(G1)))
    off = c.live()
    with pytest.raises(srt.EngineError, match="srtLiveSetMix"):
        off.set_mix(np.eye(4, 5, dtype=np.float32))
    off.close()


@pytest.mark.gpu
def test_chunking(case):
    """n_out = 1: the samples written do not depend on how the input is cut into calls, and start where the reference's accounting says"""
    c = case(4, OOB4, 4, 4)
    G = np.array([[-1.0, 0.0, 0.0, 0.0, 1.0]], np.float32)
    outs = []
    for chunks, start in (((1024,), 0), ((17, 300, 724, 1024, 1), 317)):
        live = c.live(mix=G)
        w, tl = live.process(c.L, c.R, chunks)
        live.close()
        wr, _, first = account(np.ones((c.hops + 1, 2, HOP)), c.n, chunks)
        assert first == start and w.shape == wr.shape and w.shape[0] == 2, (chunks, first, w.shape, wr.shape)
        assert np.all(tl[:, :start] == 0)
        outs.append(w)
    m = min(outs[0].shape[1], outs[1].shape[1])
    assert np.abs(outs[0]).max() > 1e-3 and np.array_equal(outs[0][:, :m], outs[1][:, :m])


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [48000, 44100])
def test_rate_instances(case, fs):
    """a rate instance with one output: every call returns n and writes 2 planes, the bits do not depend on the call sizes, and the output is the G-weighted
    sum (float64) of a mix-off rate instance's planes within the bound (both converters are linear); b_off from the 44.1 kHz case of the same config"""
    c = case(4, OOB4, 4, 4)
    G = np.array([[1.0, 0.0, 1.0, 1.0, 0.0]], np.float32)
    off = c.live(sample_rate=fs, max_block=480)
    lat = off.latency
    w, planes = off.process(c.L, c.R, (480,))
    off.close()
    assert w.shape == planes.shape == (8, c.n)
    outs = []
    for chunks in ((480,), (1, 100, 379)):
        live = c.live(mix=G, sample_rate=fs, max_block=480)
        assert live.outputs == 1 and live.latency == lat
        w, tl = live.process(c.L, c.R, chunks)
        live.close()
        assert w.shape == (2, c.n) and np.array_equal(w, tl)            # every call wrote all of its n samples
        outs.append(tl)
    assert np.array_equal(outs[0], outs[1])
    ref = sum(float(G[0, s]) * planes[2 * s:2 * s + 2].astype(np.float64) for s in range(4))
    assert np.abs(ref).max() > 1e-3
    c.within("rate instance %d Hz" % fs, outs[0], ref, G, c.peaks_of(planes) + [0.0])
