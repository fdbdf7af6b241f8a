"""Stem remix inside the inverse transform (srtSetMix): output m is the inverse transform of X * h_m with
    h = G[m][S];  for s = 0 .. S-1 ascending:  h = fmaf(G[m][s], g_s, h)
g_s = the gain the inverse transform applies for stem s with the mix off (mask, cross-faded, normalised across the stems in band; oob_weight or the average
table above F).  The srt_istft_ola3_mix_kernel (F <= 1024) and srt_istft_ola_mix_kernel (F > 1024) forms of csrc/srt_dsp.hip.

Bounds, none of them taken from what the kernels give:
  identity       a one-hot matrix reproduces the stems bit for bit (fmaf(0, g, h) = h for finite g, fmaf(1, g, 0) = g)
  float64        tests/test_dsp_float64.py's own: every output hop within MARGIN x e_cpu (+ MARGIN x the window term for F <= 1024) of the float64 inverse
                 under the host's fp32 restatement of the chain, e_cpu from the fp32 oracle on the same gains; CAP as the outer cap
  linearity      the mix against sum_s G[m][s] stem_s + G[m][S] dry (float64 sum of the mix-off results): each of those is one inverse transform of the
                 project's CAP = 2e-6 of its own peak, so CAP x (peak_m + sum_s |G[m][s]| peak_s + |G[m][S]| peak_dry)
  host stream    2e-6 of the peak against the whole signal in one call (the seam-association figure README.md states for the chunked path)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_dsp_float64 as D

T_S, S3 = 64, 3
MODES = (1, 0, 1, 0, 1, 0, 1, 0)
OOB3 = (1.0, 0.0, 0.25)
ROWS = 2 * T_S + 17                                     # 145 rows: three back-to-back tiles, the last one ragged
N_PLAIN = (ROWS - 1) * 1024 + 900
N_RAGGED = (4 * 48 + 64 + 21) * 1024 - 500            # 277 rows: six overlapped tiles at O = 16, five back-to-back ones
OV = 16
FS = (576, 1088)                                       # three-per-CU family with the band edge inside a thread's bins / table family
CAP = D.CAP
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX_KERNELS = sorted(["srt_istft_ola3_mix_kernel<4, %s, %s>" % (o, e) for o in ("false", "true") for e in ("false", "true")] +
                     ["srt_istft_ola_mix_kernel<%s, %s>" % (o, e) for o in ("false", "true") for e in ("false", "true")])


def _lib():
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


def _mix_kernel(F, ov=False, ext=False):
    b = lambda x: "true" if x else "false"                                   # noqa: E731
    return ("srt_istft_ola3_mix_kernel<4, %s, %s>" if F <= 1024 else "srt_istft_ola_mix_kernel<%s, %s>") % (b(ov), b(ext))


def chain32(G_row, g):
    """the kernel's chain on the host: h = G[S], then h = fl32(G[s] * g_s + h) for s ascending (product and sum in float64, rounded to fp32 per step).
    g: [S][...] fp32 gains (or S scalars) -> fp32 [...]"""
    G_row = np.asarray(G_row, np.float32)
    g = np.asarray(g, np.float32)
    h = np.full(g.shape[1:], G_row[-1], np.float32)
    for s in range(g.shape[0]):
        h = (np.float64(G_row[s]) * g[s].astype(np.float64) + h.astype(np.float64)).astype(np.float32)
    return h


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_abi():
    import spleeterrt_amd as srt
    from spleeterrt_amd import capi
    L = _lib()
    assert L.srtSetMix is not None and L.srtMixOutputs is not None
    hdr = open(os.path.join(ROOT, "include", "spleeterrt_amd.h")).read()
    assert "SRT_API int srtSetMix(srt_engine *e, int n_out, const float *h_gain);" in hdr
    assert "SRT_API int srtMixOutputs(const srt_engine *e);" in hdr
    assert hasattr(capi.Engine, "set_mix") and isinstance(capi.Engine.mix_outputs, property) and srt.Engine is capi.Engine
    L.srtSetMix.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.srtMixOutputs.argtypes = [C.c_void_p]
    g = (C.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    nan = (C.c_float * 4)(float("nan"), 0.0, 0.0, 0.0)
    for n_out, gain in ((0, None), (1, g), (1, None), (-1, g), (9, g), (1, nan)):       # a null engine is refused first, whatever the other arguments
        assert L.srtSetMix(None, n_out, gain) == -1 and b"srtSetMix" in L.srtLastError(), (n_out, L.srtLastError())
    assert L.srtMixOutputs(None) == 0


def test_mix_kernels_resources():
    """srt_dsp.hip compiled with the resource remarks (the recipe of test_mask_extension.py): exactly the eight mix kernels exist, each without scratch or
    spilled VGPRs and with at least two waves per SIMD (two workgroups of four waves per CU); the counts that file holds (15 inverse kernels with the
    extension in their name, 6 srt_mask_ext_kernel instantiations) have not moved"""
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
    mix = sorted(k for k in res if "mix" in k)
    assert mix == MIX_KERNELS, mix
    for k in mix:
        a = res[k]
        print("%-48s vgpr %s sgpr %s scratch %s spilled vgprs %s occupancy %s" % (
            k, a["VGPRs"], a["TotalSGPRs"], a["ScratchSize [bytes/lane]"], a["VGPRs Spill"], a["Occupancy [waves/SIMD]"]))
        assert int(a["ScratchSize [bytes/lane]"]) == 0 and int(a["VGPRs Spill"]) == 0, (k, a)
        assert int(a["Occupancy [waves/SIMD]"]) >= 2, (k, a)
    assert len([k for k in res if k.startswith("srt_istft_") and "_ext_kernel" in k]) == 15
    assert sum(1 for k in res if k.startswith("srt_mask_ext_kernel")) == 6


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _engine(coeffs, S=S3, **kw):
    import spleeterrt_amd as srt
    kw.setdefault("variant", srt.VARIANT_VST)
    kw.setdefault("T", T_S)
    kw.setdefault("oob_weights", OOB3[:S] if S <= 3 else None)
    eng = srt.Engine(stem_modes=MODES[:S], **kw)
    if coeffs is not None:
        for s in range(S):
            eng.set_coeff(s, coeffs(s))
    return eng


_AUDIO = {}


def _noisy_host(oracle, n, seed, F):
    """oracle.synth_audio plus seeded white noise of twice its RMS, scaled to a peak of 0.5; asserts on the CPU (oracle.stft) that >= 10 % of the spectral
    energy lies in bins >= F"""
    if (n, seed) not in _AUDIO:
        L, R = oracle.synth_audio(n, seed, True)
        rng = np.random.default_rng(1000 + seed)
        a = 2.0 * np.sqrt(0.5 * (np.mean(L.astype(np.float64) ** 2) + np.mean(R.astype(np.float64) ** 2)))
        L = L + a * rng.standard_normal(n)
        R = R + a * rng.standard_normal(n)
        k = 0.5 / max(np.abs(L).max(), np.abs(R).max())
        L, R = (k * L).astype(np.float32), (k * R).astype(np.float32)
        re_, im_ = oracle.stft(L, R)
        p = (re_[:, :, :2049].astype(np.float64) ** 2 + im_[:, :, :2049].astype(np.float64) ** 2).sum(axis=(0, 1))
        _AUDIO[(n, seed)] = (L, R, p)
    L, R, p = _AUDIO[(n, seed)]
    frac = float(p[F:].sum() / p.sum())
    assert frac >= 0.1, (F, frac)
    return L, R


def _noisy(oracle, n, seed, F):
    import torch
    L, R = _noisy_host(oracle, n, seed, F)
    return torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()


def _timed(eng, call):
    eng.set_timing(True)
    out = call()
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    return out, ks


IDENT_CASES = {"plain": dict(), "ratio": dict(ratio_mask=True), "overlap": dict(overlap=OV),
               "overlap+ratio+average": dict(overlap=OV, ratio_mask=True, mask_extension="average")}


@pytest.mark.gpu
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("case", list(IDENT_CASES))
def test_identity_is_bit_exact(oracle, coeffs, F, case):
    """the S one-hot rows reproduce separate() with the mix off bit for bit, on the mix kernel of the case; set_mix(None) brings the old bits and the
    old kernel list back"""
    import torch
    kw = IDENT_CASES[case]
    ov = "overlap" in kw
    L, R = _noisy(oracle, N_RAGGED if ov else N_PLAIN, 61, F)
    eng = _engine(coeffs, F=F, max_tiles=8, **kw)
    assert eng.mix_outputs == 0
    off, ks_off = _timed(eng, lambda: eng.separate(L, R).clone())
    assert off.shape[0] == S3 and "mix" not in ks_off[-1][1], ks_off[-1]
    eye = np.concatenate([np.eye(S3, dtype=np.float32), np.zeros((S3, 1), np.float32)], axis=1)
    eng.set_mix(eye)
    assert eng.mix_outputs == S3
    on, ks_on = _timed(eng, lambda: eng.separate(L, R).clone())
    assert ks_on[-1] == ("istft", _mix_kernel(F, ov, "mask_extension" in kw)), ks_on[-1]
    assert ks_on[:-1] == ks_off[:-1]
    bad = torch.nonzero(on != off)
    assert bad.numel() == 0, "%s F=%d: %d samples differ, first at %r" % (case, F, bad.shape[0], tuple(bad[0].tolist()))
    # one row alone: stem 1 as the only output
    eng.set_mix(eye[1:2])
    one = eng.separate(L, R)
    assert one.shape[0] == 1 and torch.equal(one[0], off[1])
    eng.set_mix(None)
    assert eng.mix_outputs == 0
    again, ks_again = _timed(eng, lambda: eng.separate(L, R).clone())
    assert torch.equal(again, off) and ks_again == ks_off
    eng.close()


NOCANCEL = np.array([(0.5, 0.25, 1.0, 0.0), (-0.5, 0.0, 0.0, 1.0), (0.25, 0.5, 0.125, 0.25), (1.0, 1.0, 1.0, 0.5)], np.float32)      # no row's terms cancel: every h >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("n_out", [1, 2, S3 + 1])
def test_mix_against_float64(oracle, F, n_out):
    """istft(spec, masks) with the mix on, on an arbitrary spectrum under random masks and under no masks: the M outputs as M "stems" of
    test_dsp_float64's istft_case, whose gains are the chain restated on the host in fp32 (chain32); that file's bound, hop by hop"""
    import torch
    G = NOCANCEL[:n_out]
    spec = D.spectrum_input(ROWS, 900 + F)
    masks = D.mask_input(S3, 3, T_S, F, 950 + F)
    eng = _engine(None, F=F, max_tiles=3)
    eng.set_mix(G)
    sd = torch.from_numpy(spec).cuda()
    oob = tuple(float(chain32(G[m], np.asarray(OOB3, np.float32))) for m in range(n_out))
    for with_masks in (True, False):
        got, ks = _timed(eng, lambda: eng.istft(sd, torch.from_numpy(masks).cuda() if with_masks else None).cpu().numpy())
        assert ks == [("istft", _mix_kernel(F))], ks
        g = masks if with_masks else np.ones_like(masks)
        h32 = np.stack([chain32(G[m], g) for m in range(n_out)])                  # [M][ntiles][2][T][F]
        assert np.isfinite(h32).all() and h32.min() >= 0
        D._inverse_check(oracle, "mix n_out %d" % n_out, eng, spec, h32, oob, T_S, F, masks64=h32.astype(np.float64), got=got)
    eng.close()


def _linearity(tag, mix, G, stems, dry):
    """mix [M][2][len] against sum_s G[m][s] stems[s] + G[m][S] dry in float64, bound CAP x (peak_m + sum_s |G[m][s]| peak_s + |G[m][S]| peak_dry)"""
    S = stems.shape[0]
    st, dr = stems.astype(np.float64), dry.astype(np.float64)
    pk = [float(np.abs(st[s]).max()) for s in range(S)] + [float(np.abs(dr).max())]
    bounds = []
    for m in range(G.shape[0]):
        ref = sum(float(G[m][s]) * st[s] for s in range(S)) + float(G[m][S]) * dr
        err = float(np.abs(mix[m] - ref).max())
        bound = CAP * (float(np.abs(mix[m]).max()) + sum(abs(float(G[m][s])) * pk[s] for s in range(S + 1)))
        print("%s row %d %r: max |mix - sum| = %.3g, bound %.3g (ratio %.2f)" % (tag, m, G[m].tolist(), err, bound, err / bound))
        assert np.isfinite(mix[m]).all() and err <= bound, (tag, m, err, bound)
        bounds.append(bound)
    return bounds


def _dry(L, R, F):
    """istft(stft(x), None) of a one-stem engine at oob_weight = 1: the unmasked input through the same transforms"""
    eng = _engine(None, S=1, F=F, max_tiles=8, oob_weights=(1.0,))
    spec, _ = eng.stft(L, R, want_mag=False)
    out = eng.istft(spec, None)[0].cpu().numpy()
    eng.close()
    return out


CANCEL = np.array([(0.0, -1.0, 0.0, 1.0), (1.0, 0.0, 1.0, 0.0), (0.5, 0.25, 1.0, 0.0)], np.float32)      # karaoke (input minus stem 1), an accompaniment, a remix


@pytest.mark.gpu
@pytest.mark.parametrize("F", FS)
def test_linearity_end_to_end(oracle, coeffs, F):
    import torch                                                             # noqa: F401
    L, R = _noisy(oracle, N_PLAIN, 62, F)
    eng = _engine(coeffs, F=F, max_tiles=3)
    stems = eng.separate(L, R).cpu().numpy()
    eng.set_mix(CANCEL)
    mix = eng.separate(L, R).cpu().numpy()
    eng.close()
    assert mix.shape == (3, 2, stems.shape[2])
    _linearity("plain F=%d" % F, mix, CANCEL, stems, _dry(L, R, F))


@pytest.mark.gpu
@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("F", FS)
def test_linearity_with_ratio(oracle, coeffs, F, ext):
    """ratio_mask: the chain runs over the normalised gains.  With the average extension the stems' gains sum to 1 over the whole band, so the rows
    (1,1,1 | 0) and (0,0,0 | 1) must agree - within row (1,1,1 | 0)'s bound (dry in the place of the stems' sum)"""
    L, R = _noisy(oracle, N_PLAIN, 63, F)
    eng = _engine(coeffs, F=F, max_tiles=3, ratio_mask=True, mask_extension="average" if ext else "constant")
    stems = eng.separate(L, R).cpu().numpy()
    G = np.concatenate([CANCEL, np.array([(1, 1, 1, 0), (0, 0, 0, 1)], np.float32)])
    eng.set_mix(G)
    mix, ks = _timed(eng, lambda: eng.separate(L, R).cpu().numpy())
    eng.close()
    assert ks[-1] == ("istft", _mix_kernel(F, False, ext)), ks[-1]
    dry = _dry(L, R, F)
    bounds = _linearity("ratio%s F=%d" % (" + average" if ext else "", F), mix, G, stems, dry)
    if ext:
        err = float(np.abs(mix[3].astype(np.float64) - mix[4]).max())
        print("ratio + average F=%d: rows (1,1,1|0) and (0,0,0|1) differ by %.3g, bound %.3g" % (F, err, bounds[3]))
        assert err <= bounds[3], (err, bounds[3])


@pytest.mark.gpu
def test_linearity_in_the_fp16_mode(oracle, coeffs):
    """fp16 mode (F = 512: the fp16 storage needs F % 256 == 0, which neither 576 nor 1088 is): while the mix is on the engine's own masks stay floats, so
    separate() equals istft(spec, forward(mag)) bit for bit - forward hands out fp32 masks - and the mix is linear in the mix-off stems of the same mode"""
    import torch
    import spleeterrt_amd as srt
    F = 512
    L, R = _noisy(oracle, N_PLAIN, 64, F)
    eng = _engine(coeffs, F=F, max_tiles=3, precision=srt.PREC_F16)
    eng.set_mix(CANCEL)
    mix, ks = _timed(eng, lambda: eng.separate(L, R).clone())
    assert ks[-1] == ("istft", _mix_kernel(F)), ks[-1]
    spec, mag = eng.stft(L, R)
    chain = eng.istft(spec, eng.forward(mag))
    assert torch.equal(mix, chain)
    # the mix-off stems by the same route, on fp32 masks (the half masks of the mix-off separate() would add their own 2^-11 rounding to the comparison)
    eng.set_mix(None)
    stems = eng.istft(spec, eng.forward(mag)).cpu().numpy()
    eng.close()
    _linearity("fp16 mode", mix.cpu().numpy(), CANCEL, stems, _dry(L, R, F))


@pytest.mark.gpu
@pytest.mark.parametrize("F", FS)
def test_host_stream(oracle, coeffs, F):
    """max_tiles = 1: the 277-row signal takes five chunks, so staging, seam carry, download and the 16-bit pack all run over n_out planes"""
    import torch
    from spleeterrt_amd import capi
    Lh, Rh = _noisy_host(oracle, N_RAGGED, 65, F)
    eng = _engine(coeffs, F=F, max_tiles=1, batch_invariant=True)
    off = eng.separate_host_stream(Lh, Rh)
    eye = np.concatenate([np.eye(S3, dtype=np.float32), np.zeros((S3, 1), np.float32)], axis=1)
    eng.set_mix(eye)
    on = eng.separate_host_stream(Lh, Rh)
    assert on.shape == off.shape and np.array_equal(on, off)
    loud = np.array((3.0, 1.0, 3.0), np.float32)
    loud *= np.float32(1.5 / np.abs(np.tensordot(loud.astype(np.float64), off, 1)).max())       # the second output peaks near 1.5: it clips (the mix is linear)
    G = np.array([(0.0, -1.0, 0.0, 1.0), tuple(loud) + (0.0,)], np.float32)
    eng.set_mix(G)
    two = eng.separate_host_stream(Lh, Rh)
    assert two.shape == (2, 2, off.shape[2])
    whole = _engine(coeffs, F=F, max_tiles=5, batch_invariant=True)
    whole.set_mix(G)
    Ld, Rd = torch.from_numpy(Lh).cuda(), torch.from_numpy(Rh).cuda()
    rows = whole.L.srtStftRows(Lh.size)
    ref = whole.separate_ex(Ld, Rd, whole.L.srtStftFrames(Lh.size), rows).cpu().numpy()
    whole.close()
    peak = float(np.abs(ref).max())
    err = float(np.abs(two - ref).max())
    print("host stream F=%d: five chunks against one call, max-abs / peak = %.3g" % (F, err / peak))
    assert ref.shape == two.shape and err <= 2e-6 * peak, err / peak
    # 16-bit output: the planes the float call gave, packed by the same rule, and one clipped-sample count per OUTPUT
    two_io, clip0 = eng.separate_host_stream_io((Lh, Rh))
    assert np.array_equal(two_io, two) and clip0.shape == (2,) and not clip0.any()
    q, clipped = eng.separate_host_stream_io((Lh, Rh), out_pcm16=True)
    want, wclip = capi.pcm16_pack(torch.from_numpy(two).cuda())
    print("host stream F=%d: clipped %r" % (F, clipped.tolist()))
    assert q.shape == (2, off.shape[2], 2) and q.dtype == np.int16 and np.array_equal(q, want.cpu().numpy())
    assert clipped.shape == (2,) and np.array_equal(clipped.astype(np.int64), wclip.cpu().numpy()) and clipped[1] > 0
    eng.release_staging()
    eng.close()


@pytest.mark.gpu
def test_graph_mode_never_replays_an_old_matrix(oracle, coeffs):
    import torch
    F = 576
    L, R = _noisy(oracle, N_PLAIN, 66, F)
    A, B = CANCEL[:2], CANCEL[1:3]
    eager = {}
    eng = _engine(coeffs, F=F, max_tiles=3, batch_invariant=True)
    for name, G in (("A", A), ("B", B)):
        eng.set_mix(G)
        eager[name] = eng.separate(L, R).clone()
    eng.close()
    assert not torch.equal(eager["A"], eager["B"])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng = _engine(coeffs, F=F, max_tiles=3, batch_invariant=True)
        eng.set_graph_mode(True)
        out = torch.empty_like(eager["A"])
        for name, G in (("A", A), ("A", None), ("B", B), ("B", None), ("A", A)):     # capture, replay, a new matrix, its replay, the first matrix set again
            if G is not None:
                eng.set_mix(G)
            out.fill_(float("nan"))
            eng.separate(L, R, out)
            s.synchronize()
            assert torch.equal(out, eager[name]), name
        eng.close()


@pytest.mark.gpu
def test_refusals(oracle, coeffs):
    """srtSetMix's argument checks on a live engine; every entry point without a mix returns -1 with "mix" in the text and leaves its NaN-filled output
    untouched, and runs again after set_mix(None)"""
    import torch
    import spleeterrt_amd as srt
    from spleeterrt_amd import capi
    F = 576
    eng = _engine(coeffs, S=2, F=F, max_tiles=4, oob_weights=(0.1, 0.1))
    Lq = eng.L
    vp = C.c_void_p
    one = np.array([(1.0, -1.0, 0.0)], np.float32)
    for n_out, gain, why in ((-1, one, "n_out"), (9, one, "n_out"), (1, None, "null"), (1, np.array([(1.0, np.inf, 0.0)], np.float32), "finite"),
                             (1, np.array([(np.nan, 0.0, 0.0)], np.float32), "finite")):
        assert Lq.srtSetMix(eng.h, n_out, None if gain is None else vp(gain.ctypes.data)) == -1 and b"srtSetMix" in Lq.srtLastError(), (why, Lq.srtLastError())
        assert eng.mix_outputs == 0
    with pytest.raises(srt.EngineError):
        eng.set_mix(np.ones((1, 4), np.float32))                             # the wrong row length for two stems
    eng.set_wiener(1)
    assert Lq.srtSetMix(eng.h, 1, vp(one.ctypes.data)) == -1 and b"srtSetMix" in Lq.srtLastError() and b"Wiener" in Lq.srtLastError()
    assert Lq.srtSetMix(eng.h, 0, None) == 0                                 # switching off is always possible
    eng.set_wiener(0)
    eng.set_mix(one)
    assert Lq.srtSetWiener(eng.h, 1) == -1 and b"mix" in Lq.srtLastError()
    assert Lq.srtSetWiener(eng.h, 0) == 0

    n = 100 * 1024 + 300                                                     # 101 rows: two tiles
    rows = Lq.srtStftRows(n)
    ln = Lq.srtIstftLength(rows)
    Lh, Rh = _noisy_host(oracle, n, 67, F)
    Ld, Rd = torch.from_numpy(Lh).cuda(), torch.from_numpy(Rh).cuda()
    eng.set_mix(None)
    spec, mag = eng.stft(Ld, Rd)
    masks = eng.forward(mag)
    d_out = torch.empty((3, 2, ln), device="cuda")
    h_out = np.empty((3, 2, ln), np.float32)
    h16 = np.empty((3, ln, 2), np.int16)
    clip = np.zeros(3, np.uint64)
    P1 = vp * 1
    calls = {
        "srtSeparateCli": (lambda: Lq.srtSeparateCli(eng.h, vp(Ld.data_ptr()), vp(Rd.data_ptr()), n, 2, vp(d_out.data_ptr())), "d"),
        "srtSeparateCliHost": (lambda: Lq.srtSeparateCliHost(eng.h, vp(Lh.ctypes.data), vp(Rh.ctypes.data), n, 3, vp(h_out.ctypes.data)), "h"),
        "srtSeparateCliHostIo": (lambda: Lq.srtSeparateCliHostIo(eng.h, vp(Lh.ctypes.data), vp(Rh.ctypes.data), n, 2, vp(h16.ctypes.data), capi.HOST_OUT_PCM16, vp(clip.ctypes.data)), "q"),
        "srtSeparateBatch": (lambda: Lq.srtSeparateBatch(eng.h, 1, P1(Ld.data_ptr()), P1(Rd.data_ptr()), (C.c_size_t * 1)(n), P1(d_out.data_ptr())), "d"),
        "srtSeparateBatchWiener": (lambda: Lq.srtSeparateBatchWiener(eng.h, 1, P1(Ld.data_ptr()), P1(Rd.data_ptr()), (C.c_size_t * 1)(n), P1(d_out.data_ptr()), 1), "d"),
        "srtIstftWiener": (lambda: Lq.srtIstftWiener(eng.h, vp(spec.data_ptr()), rows, vp(masks.data_ptr()), 1, vp(d_out.data_ptr())), "d"),
    }
    SENT = 0x5A5A
    for name, (call, where) in calls.items():
        eng.set_mix(one)
        d_out.fill_(float("nan"))
        h_out.fill(np.nan)
        h16.fill(SENT)
        assert call() == -1, name
        assert b"mix" in Lq.srtLastError(), (name, Lq.srtLastError())
        torch.cuda.synchronize()
        assert bool(torch.isnan(d_out).all()) and np.isnan(h_out).all() and (h16 == SENT).all(), name
        eng.set_mix(None)
        assert call() == 0, (name, Lq.srtLastError())
        torch.cuda.synchronize()
        if where == "q":
            assert (h16[:2] != SENT).any(), name
        else:
            assert np.isfinite((h_out if where == "h" else d_out.cpu().numpy())[:2]).all(), name
    eng.release_staging()
    eng.close()

    # the multi-device driver: the mix on one of its engines (two engines on device 0)
    cfg = capi._Config()
    cfg.F, cfg.T, cfg.n_stems, cfg.variant, cfg.max_tiles = F, T_S, 2, srt.VARIANT_VST, 2
    for s in range(2):
        cfg.stem_mode[s], cfg.oob_weight[s] = MODES[s], 0.1
    m = vp()
    assert Lq.srtMultiCreate(C.byref(cfg), (C.c_int * 2)(0, 0), 2, C.byref(m)) == 0, Lq.srtLastError()
    for s in range(2):
        c = np.ascontiguousarray(coeffs(s), np.float32)
        assert Lq.srtMultiSetCoeffHost(m, s, vp(c.ctypes.data)) == 0
    Lq.srtMultiEngine.restype, Lq.srtMultiEngine.argtypes = vp, [vp, C.c_int]
    e2 = Lq.srtMultiEngine(m, 1)
    multi = {
        "srtMultiSeparateHost": lambda: Lq.srtMultiSeparateHost(m, vp(Lh.ctypes.data), vp(Rh.ctypes.data), n, vp(h_out.ctypes.data), 0),
        "srtMultiSeparateCliHost": lambda: Lq.srtMultiSeparateCliHost(m, vp(Lh.ctypes.data), vp(Rh.ctypes.data), n, 2, vp(h_out.ctypes.data)),
    }
    for name, call in multi.items():
        assert Lq.srtSetMix(e2, 1, vp(one.ctypes.data)) == 0 and Lq.srtMixOutputs(e2) == 1
        h_out.fill(np.nan)
        assert call() == -1 and b"mix" in Lq.srtLastError(), (name, Lq.srtLastError())
        assert np.isnan(h_out).all(), name
        assert Lq.srtSetMix(e2, 0, None) == 0 and Lq.srtMixOutputs(e2) == 0
        assert call() == 0, (name, Lq.srtLastError())
        assert np.isfinite(h_out[:2]).all(), name
    Lq.srtMultiDestroy(m)
