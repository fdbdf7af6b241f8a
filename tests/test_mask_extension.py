"""Average mask extension for the bins above the analysed band (srtSetMaskExtension).

CPU: the ABI, and the register / scratch / occupancy figures of every EXT inverse instantiation against its sibling.  GPU: the mode switched off is the
present path (bits and launch list); the gain table against a float64 mean and exact on constant rows; the EXT inverse kernels (both families, plain and
overlapped masks) against the constant-rule kernels on a host-scaled spectrum; srtSeparate = its stages (plain, ratio, overlap + ratio); the CPU oracle end
to end; the stems of a ratio engine sum to the input over the whole band; batch, host stream, graph mode, the fp16 mode's half masks, coverage of the
output, and every refusal.  The signals carry seeded white noise so that at least 10 % of their energy lies in the bins the mode governs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

T_S = 64
MODES = (1, 0, 1, 0, 1, 0, 1, 0)
N_RAGGED = (4 * 48 + 64 + 21) * 1024 - 500            # 277 rows (273 transformed frames): four tiles + a tail; six overlapped tiles at O = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                                        # fp32 unit roundoff


def _chain(F):
    """additions in the longest chain of the kernel's sum: a lane adds its F / 64 values in ascending k, then six butterfly steps over the 64 lanes"""
    return F // 64 + 6


def _lib():
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_abi():
    import spleeterrt_amd as srt
    from spleeterrt_amd import capi
    L = _lib()
    assert L.srtSetMaskExtension is not None
    hdr = open(os.path.join(ROOT, "include", "spleeterrt_amd.h")).read()
    assert re.search(r"#define\s+SRT_MASK_EXT_CONSTANT\s+0\b", hdr) and re.search(r"#define\s+SRT_MASK_EXT_AVERAGE\s+1\b", hdr)
    assert "srtSetMaskExtension(srt_engine *e, int mode)" in hdr
    assert (capi.MASK_EXT_CONSTANT, capi.MASK_EXT_AVERAGE) == (0, 1) == (srt.MASK_EXT_CONSTANT, srt.MASK_EXT_AVERAGE)
    assert hasattr(capi.Engine, "set_mask_extension")
    L.srtSetMaskExtension.argtypes = [C.c_void_p, C.c_int]
    for mode in (0, 1, 7):
        assert L.srtSetMaskExtension(None, mode) == -1 and b"srtSetMaskExtension" in L.srtLastError()


def test_ext_inverse_kernels_keep_their_siblings_resources():
    """srt_dsp.hip compiled with the resource remarks (as scripts/kernel_resources.py does): every inverse instantiation with the extension has no scratch
    and at least the occupancy of the same instantiation without it (the ratio forms of the three-per-CU family come out at 168 VGPRs / occupancy 3 where
    their siblings take 170 / 2: more resident waves than the sibling, never fewer)"""
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
    ext = sorted(k for k in res if k.startswith("srt_istft_") and "_ext_kernel" in k)
    # ola3 plain / ratio / half, ola plain / ratio, their overlap forms, the five batch forms
    assert len(ext) == 15, ext
    for k in ext:
        sib = k.replace("_ext_kernel", "_kernel")
        assert sib in res, (k, sib)
        a, b = res[k], res[sib]
        print("%-52s vgpr %s sgpr %s scratch %s occ %s | sibling vgpr %s sgpr %s scratch %s occ %s" % (
            k, a["VGPRs"], a["TotalSGPRs"], a["ScratchSize [bytes/lane]"], a["Occupancy [waves/SIMD]"],
            b["VGPRs"], b["TotalSGPRs"], b["ScratchSize [bytes/lane]"], b["Occupancy [waves/SIMD]"]))
        assert int(a["ScratchSize [bytes/lane]"]) == 0 and int(a["VGPRs Spill"]) == 0, (k, a)
        assert int(a["Occupancy [waves/SIMD]"]) >= int(b["Occupancy [waves/SIMD]"]), (k, a, b)
    for k in res:
        if k.startswith("srt_mask_ext_kernel"):
            assert int(res[k]["ScratchSize [bytes/lane]"]) == 0 and int(res[k]["LDS Size [bytes/block]"]) == 0, (k, res[k])
    assert sum(1 for k in res if k.startswith("srt_mask_ext_kernel")) == 6


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _engine(coeffs, S=2, **kw):
    import spleeterrt_amd as srt
    kw.setdefault("variant", srt.VARIANT_VST)
    kw.setdefault("F", 512)
    kw.setdefault("T", T_S)
    eng = srt.Engine(stem_modes=MODES[:S], **kw)
    for s in range(S):
        eng.set_coeff(s, coeffs(s))
    return eng


_AUDIO = {}


def _noisy_host(oracle, n, seed, F):
    """oracle.synth_audio plus seeded white noise of twice its RMS; asserts on the CPU (oracle.stft) that >= 10 % of the spectral energy lies in bins >= F"""
    if (n, seed) not in _AUDIO:
        L, R = oracle.synth_audio(n, seed, True)
        rng = np.random.default_rng(1000 + seed)
        a = 2.0 * np.sqrt(0.5 * (np.mean(L.astype(np.float64) ** 2) + np.mean(R.astype(np.float64) ** 2)))
        L = (L + a * rng.standard_normal(n)).astype(np.float32)
        R = (R + a * rng.standard_normal(n)).astype(np.float32)
        re_, im_ = oracle.stft(L, R)
        p = (re_[:, :, :2049].astype(np.float64) ** 2 + im_[:, :, :2049].astype(np.float64) ** 2).sum(axis=(0, 1))
        _AUDIO[(n, seed)] = (L, R, p, re_, im_)
    L, R, p, _, _ = _AUDIO[(n, seed)]
    frac = float(p[F:].sum() / p.sum())
    assert frac >= 0.1, (F, frac)
    return L, R


def _noisy(oracle, n, seed, F):
    import torch
    L, R = _noisy_host(oracle, n, seed, F)
    return torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()


def _rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


def _blend_rows(masks, rows, T, O):
    """the overlap rule on the host, fp32 step by step (as tests/test_overlap.py): masks [S][tiles][2][T][F] in the overlapped layout -> per-row masks
    [S][2][rows][F]; row r: primary tile j1 = min(r / S, tiles - 1), offset k = r - j1 S; inside an overlap a + w (b - a), w = (k + 1/2) / O"""
    from spleeterrt_amd import stream
    S_, nt = masks.shape[0], masks.shape[1]
    assert nt == stream.overlap_tiles(rows, T, O)
    st = T - O
    out = np.empty((S_, 2, rows, masks.shape[-1]), np.float32)
    for r in range(rows):
        j1 = min(r // st, nt - 1)
        k = r - j1 * st
        b = masks[:, j1, :, k]
        if O and j1 > 0 and k < O:
            a = masks[:, j1 - 1, :, k + st]
            w = np.float32(k + 0.5) / np.float32(O)
            out[:, :, r] = a + w * (b - a)
        else:
            out[:, :, r] = b
    return out


def _pack_rows(m, T):
    """per-row masks [S][2][rows][F] -> the back-to-back layout [S][ceil(rows / T)][2][T][F] (rows past the signal: zero)"""
    S_, _, rows, F = m.shape
    nt = (rows + T - 1) // T
    p = np.zeros((S_, nt, 2, T, F), np.float32)
    for r in range(rows):
        p[:, r // T, :, r % T] = m[:, :, r]
    return p


def _table(eng, rows):
    """[S][rows][2]"""
    return np.stack([eng.mask_ext(s, rows) for s in range(eng.S)])


def _timed(eng, call):
    eng.set_timing(True)
    out = call()
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    return out, ks


def _ext_names(F, ratio=False, ov=False, m16=False):
    b = lambda x: "true" if x else "false"                                   # noqa: E731
    me = ("mask_ext", "srt_mask_ext_kernel<%s, %s, %s>" % (b(m16), b(ratio), b(ov)))
    if F <= 1024:
        inv = "srt_istft_ola3%s_ext_kernel<4, %s, %s>" % ("_ov" if ov else "", b(ratio), b(m16))
    else:
        inv = "srt_istft_ola%s_ext_kernel<%s>" % ("_ov" if ov else "", b(ratio))
    return me, ("istft", inv)


@pytest.mark.gpu
def test_off_is_the_present_path(oracle, coeffs):
    """srtSeparate on an engine that switched the extension on, ran, and switched it off again equals a fresh engine, and launches the same kernels"""
    import torch
    L, R = _noisy(oracle, N_RAGGED, 41, 512)
    outs, lists = [], []
    for touch in (False, True):
        eng = _engine(coeffs, max_tiles=8, batch_invariant=True)
        if touch:
            eng.set_mask_extension("average")
            eng.separate(L, R)
            eng.set_mask_extension("constant")
        eng.separate(L, R)
        out, ks = _timed(eng, lambda: eng.separate(L, R).clone())
        outs.append(out)
        lists.append(ks)
        eng.close()
    assert torch.equal(outs[0], outs[1])
    assert lists[0] == lists[1]
    assert all(n != "mask_ext" for n, _ in lists[1])
    assert lists[0][0] == ("stft", "srt_stft_kernel") and lists[0][-1] == ("istft", "srt_istft_ola3_kernel<4, false, false>"), (lists[0][0], lists[0][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_the_table(oracle, coeffs, F):
    """srtIstft on random fp32 masks, S = 3: the table is within (n + 1) 2^-24 of the float64 mean, n = F / 64 + 6 the additions of the kernel's longest
    chain (each rounds a partial sum <= F by at most 2^-24 of it, i.e. 2^-24 of the mean's scale after the division, which rounds once more; masks in [0, 1]).
    Rows of one constant j / 256 come back exactly: every partial sum is a multiple of 1/256 below 2^24 / 256, and the division is a true one."""
    import torch
    S = 3
    eng = _engine(coeffs, S=S, F=F, max_tiles=8, mask_extension="average")
    L, R = _noisy(oracle, N_RAGGED, 42, F)
    spec, _ = eng.stft(L, R, want_mag=False)
    rows = spec.shape[1]
    nt = (rows + T_S - 1) // T_S
    rng = np.random.default_rng(51)
    m = rng.random((S, nt, 2, T_S, F), dtype=np.float32)
    _, ks = _timed(eng, lambda: eng.istft(spec, torch.from_numpy(m).cuda()))
    assert ks == list(_ext_names(F)), ks
    got = _table(eng, rows)                                                 # [S][rows][2]
    want = m.astype(np.float64).mean(axis=-1).transpose(0, 2, 1, 3).reshape(S, 2, nt * T_S)[:, :, :rows].transpose(0, 2, 1)
    err = float(np.abs(got - want).max())
    print("table F=%d: max |e - mean64| = %.3g (bound %.3g)" % (F, err, (_chain(F) + 1) * U))
    assert err <= (_chain(F) + 1) * U, (F, err)
    j = rng.integers(0, 257, size=(S, nt, 2, T_S, 1))
    mc = np.broadcast_to((j / 256.0).astype(np.float32), (S, nt, 2, T_S, F)).copy()
    eng.istft(spec, torch.from_numpy(mc).cuda())
    got = _table(eng, rows)
    want = mc[..., 0].transpose(0, 2, 1, 3).reshape(S, 2, nt * T_S)[:, :, :rows].transpose(0, 2, 1)
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    # no masks: all-ones, e = 1 exactly and no table kernel - the output is the constant rule's at oob_weight = 1
    out1, ks = _timed(eng, lambda: eng.istft(spec, None))
    assert [n for n, _ in ks] == ["istft"] and "_ext_" not in ks[0][1], ks
    one = _engine(coeffs, S=S, F=F, max_tiles=8, oob_weights=(1.0,) * S)
    assert torch.equal(out1, one.istft(spec, None))
    one.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O", [0, 16])
@pytest.mark.parametrize("F", [512, 1536])
def test_ext_inverse_kernels_against_the_constant_path(oracle, coeffs, F, O):
    """For every stem the host builds spec' = spec x (mask in band, the table's row gain above), fp32 products, and an S = 1, oob_weight = 1 engine without
    masks transforms it (constant rule: every bin as it is).  The AVERAGE output must agree to 2e-6 of the peak (the project's bound for the inverse kernels,
    tests/test_overlap.py).  O = 16: masks in the overlapped layout, blended on the host by _blend_rows; the table is then also held to the float64 mean of
    the host-blended rows.  All-0.5 masks against a constant-mode engine at oob_weight = 0.5: the same bound, equality expected."""
    import torch
    from spleeterrt_amd import stream
    S = 3
    eng = _engine(coeffs, S=S, F=F, max_tiles=12, mask_extension="average", overlap=O)
    one = _engine(coeffs, S=1, F=F, max_tiles=12, oob_weights=(1.0,))
    L, R = _noisy(oracle, N_RAGGED, 43, F)
    spec, _ = eng.stft(L, R, want_mag=False)
    rows = spec.shape[1]
    nt = stream.overlap_tiles(rows, T_S, O)
    rng = np.random.default_rng(52 + O)
    m = rng.random((S, nt, 2, T_S, F), dtype=np.float32)
    got, ks = _timed(eng, lambda: eng.istft(spec, torch.from_numpy(m).cuda()))
    assert ks == list(_ext_names(F, ov=O > 0)), ks
    tab = _table(eng, rows)
    mr = _blend_rows(m, rows, T_S, O)                                       # [S][2][rows][F]
    terr = float(np.abs(tab - mr.astype(np.float64).mean(axis=-1).transpose(0, 2, 1)).max())
    print("F=%d O=%d: table against the host rows' float64 mean %.3g" % (F, O, terr))
    assert terr <= (_chain(F) + 1) * U, (F, O, terr)
    sp = spec.cpu().numpy()
    for s in range(S):
        x = sp.copy()
        x[:, :, :F, :] *= mr[s][:, :, :, None]
        x[:, :, F:2049, :] *= tab[s].T[:, :, None, None]
        ref = one.istft(torch.from_numpy(x).cuda(), None)[0]
        peak = float(ref.abs().max())
        err = float((got[s] - ref).abs().max())
        print("F=%d O=%d stem %d: max-abs / peak = %.3g" % (F, O, s, err / peak))
        assert err <= 2e-6 * peak, (F, O, s, err / peak)
    half = torch.full((S, nt, 2, T_S, F), 0.5, device="cuda")
    got = eng.istft(spec, half)
    assert np.array_equal(_table(eng, rows), np.full((S, rows, 2), 0.5, np.float32))
    con = _engine(coeffs, S=S, F=F, max_tiles=12, oob_weights=(0.5,) * S, overlap=O)
    ref = con.istft(spec, half)
    peak = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print("F=%d O=%d all-0.5 masks against oob_weight 0.5: max-abs / peak = %.3g" % (F, O, err / peak))
    assert err <= 2e-6 * peak, (F, O, err / peak)
    for e in (eng, one, con):
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_separate_is_the_composition_of_its_stages(oracle, coeffs, F):
    """mode on, batch_invariant: srtSeparate is bit for bit stft -> forward -> istft; with ratio_mask it is within 2e-6 of the peak of stft -> forward ->
    srtRatioMask on a copy -> istft; with O = 16 and the ratio, of istft (O = 0) on the host-blended, host-normalised masks"""
    import torch
    L, R = _noisy(oracle, N_RAGGED, 44, F)
    eng = _engine(coeffs, S=2, F=F, max_tiles=12, batch_invariant=True, mask_extension="average")
    whole, ks = _timed(eng, lambda: eng.separate(L, R))
    assert tuple(ks[-2:]) == _ext_names(F), ks[-2:]
    spec, mag = eng.stft(L, R)
    assert torch.equal(whole, eng.istft(spec, eng.forward(mag)))
    eng.close()

    eng = _engine(coeffs, S=3, F=F, max_tiles=12, batch_invariant=True, ratio_mask=True, mask_extension="average")
    whole, ks = _timed(eng, lambda: eng.separate(L, R))
    assert tuple(ks[-2:]) == _ext_names(F, ratio=True), ks[-2:]
    spec, mag = eng.stft(L, R)
    rows = spec.shape[1]
    raw = eng.forward(mag)
    ref = eng.istft(spec, eng.ratio_mask(raw.clone()))
    peak = float(ref.abs().max())
    err = float((whole - ref).abs().max())
    print("ratio F=%d: max-abs / peak = %.3g" % (F, err / peak))
    assert err <= 2e-6 * peak, (F, err / peak)

    eng.set_overlap(16)
    whole, ks = _timed(eng, lambda: eng.separate(L, R))
    assert tuple(ks[-2:]) == _ext_names(F, ratio=True, ov=True), ks[-2:]
    tab_whole = _table(eng, rows)
    spec, mag = eng.stft(L, R)
    raw = eng.forward(mag).cpu().numpy()
    m = oracle.ratio_mask(_blend_rows(raw, rows, T_S, 16))
    eng.set_overlap(0)
    ref = eng.istft(spec, torch.from_numpy(_pack_rows(m, T_S)).cuda())       # (srtIstft applies masks as given, on a ratio_mask engine too)
    peak = float(ref.abs().max())
    err = float((whole - ref).abs().max())
    terr = float(np.abs(tab_whole - _table(eng, rows)).max())
    print("overlap + ratio F=%d: max-abs / peak = %.3g, tables differ by %.3g" % (F, err / peak, terr))
    assert err <= 2e-6 * peak, (F, err / peak)
    eng.close()


N_STEMS_E2E = 4
_ORACLE = {}


def _oracle_masks(oracle, coeffs):
    """the oracle's stft and per-row masks [S][2][rows][F] of the shared end-to-end signal (4 stems, F = 512, back-to-back tiles), computed once"""
    if not _ORACLE:
        F, S = 512, N_STEMS_E2E
        L, R = _noisy_host(oracle, N_RAGGED, 45, F)
        _, _, _, re_, im_ = _AUDIO[(N_RAGGED, 45)]
        rows = re_.shape[1]
        nt = (rows + T_S - 1) // T_S
        masks = np.empty((S, nt, 2, T_S, F), np.float32)
        for j in range(nt):
            mag = oracle.magnitude_tile(re_, im_, j * T_S, T_S, F)
            for s in range(S):
                masks[s, j] = oracle.forward(coeffs(s), mag, MODES[s], oracle.VARIANT_VST)
        _ORACLE.update(L=L, R=R, re=re_, im=im_, m=_blend_rows(masks, rows, T_S, 0))
    return _ORACLE


def _apply_average(oracle, re_, im_, m, F):
    """the issue's rule over the oracle's stages: gains m [S][2][rows][F] in band, their fp32 mean per row and channel above, then the oracle's istft"""
    out = []
    for s in range(m.shape[0]):
        e = m[s].mean(axis=-1, dtype=np.float32)[:, :, None]
        r, i = re_.copy(), im_.copy()
        r[:, :, :F] *= m[s]
        i[:, :, :F] *= m[s]
        r[:, :, F:2049] *= e
        i[:, :, F:2049] *= e
        out.append(oracle.istft(r, i))
    return np.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [False, True])
def test_end_to_end_against_the_oracle(oracle, coeffs, ratio):
    """4 stems, fp32, F = 512: oracle.stft, oracle.forward per tile, oracle.ratio_mask when on, the fp32 mean per row and channel, oracle.istft (the reference
    program has no extension: these are the oracle's masks under the rule).  Every output sample: rel-RMS <= 1e-4 and max-abs <= 1e-4 of the peak."""
    import torch
    o = _oracle_masks(oracle, coeffs)
    S, F = N_STEMS_E2E, 512
    eng = _engine(coeffs, S=S, F=F, max_tiles=8, ratio_mask=ratio, mask_extension="average")
    got = eng.separate(torch.from_numpy(o["L"]).cuda(), torch.from_numpy(o["R"]).cuda()).cpu().numpy()
    eng.close()
    ref = _apply_average(oracle, o["re"], o["im"], oracle.ratio_mask(o["m"]) if ratio else o["m"], F)
    assert got.shape == ref.shape and np.isfinite(got).all()
    for s in range(S):
        peak = float(np.abs(ref[s]).max())
        rr, ma = _rel_rms(got[s], ref[s]), float(np.abs(got[s] - ref[s]).max()) / peak
        print("oracle ratio=%d stem %d: rel-RMS %.3g, max-abs / peak %.3g" % (ratio, s, rr, ma))
        assert rr <= 1e-4, (ratio, s, rr)
        assert ma <= 1e-4, (ratio, s, ma)


@pytest.mark.gpu
def test_stems_sum_to_the_input(oracle, coeffs):
    """ratio_mask + AVERAGE: the four stems sum to oracle.istft(oracle.stft(x)) over the whole band, rel-RMS <= 1e-4; the table's gains sum to 1 over the
    stems up to rounding (each mean is within (n + 1) 2^-24 of the exact mean of gains that sum to 1 within a few roundings each: S (n + 1) 2^-24 + 16 2^-24).
    The same engine under the constant rule at oob_weight = 0.1 misses by more than 0.1 rel-RMS: the upper band then sums to 0.4 x the input."""
    S, F = 4, 512
    L, R = _noisy(oracle, N_RAGGED, 45, F)
    _, _, _, re_, im_ = _AUDIO[(N_RAGGED, 45)]
    ref = oracle.istft(re_, im_)
    eng = _engine(coeffs, S=S, F=F, max_tiles=8, ratio_mask=True, mask_extension="average")
    got = eng.separate(L, R).cpu().numpy().sum(axis=0)
    rows = re_.shape[1]
    tsum = _table(eng, rows).astype(np.float64).sum(axis=0)
    terr = float(np.abs(tsum - 1.0).max())
    rr = _rel_rms(got, ref)
    print("sum of stems, average: rel-RMS %.3g; |sum of gains - 1| <= %.3g" % (rr, terr))
    assert rr <= 1e-4, rr
    assert terr <= (S * (_chain(F) + 1) + 16) * U, terr
    eng.set_mask_extension("constant")
    miss = _rel_rms(eng.separate(L, R).cpu().numpy().sum(axis=0), ref)
    print("sum of stems, constant 0.1: rel-RMS %.3g" % miss)
    assert miss > 0.1, miss
    eng.close()


@pytest.mark.gpu
def test_batch(oracle, coeffs):
    """three tracks - shorter than a tile, one tile plus a tail, exactly two tiles - in one srtSeparateBatch with the mode on: each bit for bit srtSeparate of
    that track (batch_invariant), through the batched EXT kernel"""
    import torch
    F = 512
    ns = (40 * 1024 - 100, (64 + 21) * 1024 - 300, 128 * 1024)
    eng = _engine(coeffs, S=2, F=F, max_tiles=8, batch_invariant=True, mask_extension="average")
    tr = [_noisy(oracle, n, 60 + k, F) for k, n in enumerate(ns)]
    got, ks = _timed(eng, lambda: eng.separate_batch(tr))
    assert ks[-2:] == [("mask_ext", "srt_mask_ext_kernel<false, false, false>"), ("istft_batch", "srt_istft_batch_ext_kernel<true, false, false>")], ks[-2:]
    for k, (L, R) in enumerate(tr):
        ref = eng.separate(L, R)
        assert got[k].shape == ref.shape
        assert torch.equal(got[k], ref), (k, float((got[k] - ref).abs().max()))
    eng.close()


@pytest.mark.gpu
def test_host_stream(oracle, coeffs):
    """separate_host_stream on a max_tiles = 2 engine (three chunks) against srtSeparate of the whole signal on a larger engine, mode on: 2e-6 of the peak,
    the bound of the existing stream tests for chunk seams (the gain is row-local, so the seams need nothing)"""
    F = 512
    Lh, Rh = _noisy_host(oracle, N_RAGGED, 46, F)
    L, R = _noisy(oracle, N_RAGGED, 46, F)
    big = _engine(coeffs, S=2, F=F, max_tiles=8, batch_invariant=True, mask_extension="average")
    ref = big.separate(L, R).cpu().numpy()
    big.close()
    eng = _engine(coeffs, S=2, F=F, max_tiles=2, batch_invariant=True, mask_extension="average")
    got = eng.separate_host_stream(Lh, Rh)
    eng.close()
    assert got.shape == ref.shape
    peak = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("host stream: max-abs / peak = %.3g" % (err / peak))
    assert err <= 2e-6 * peak, err / peak


@pytest.mark.gpu
def test_graph_mode_keys_on_the_mode(oracle, coeffs):
    """graph mode: calls with the mode on, off, on, on, off on the same buffers each equal their eager result"""
    import torch
    L, R = _noisy(oracle, N_RAGGED, 47, 512)
    eager = {}
    eng = _engine(coeffs, S=2, max_tiles=8, batch_invariant=True)
    for mode in ("average", "constant"):
        eng.set_mask_extension(mode)
        eager[mode] = eng.separate(L, R).clone()
    eng.close()
    assert not torch.equal(eager["average"], eager["constant"])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng = _engine(coeffs, S=2, max_tiles=8, batch_invariant=True)
        eng.set_mask_extension("average")                                  # (allocates the table before anything is captured)
        eng.set_graph_mode(True)
        out = torch.empty_like(eager["average"])
        for mode in ("average", "constant", "average", "average", "constant"):
            eng.set_mask_extension(mode)
            out.fill_(float("nan"))
            eng.separate(L, R, out)
            s.synchronize()
            assert torch.equal(out, eager[mode]), mode
        eng.close()


@pytest.mark.gpu
def test_half_masks(oracle, coeffs):
    """the fp16 mode at T = 256, F = 1024, 4 tiles x 4 stems (the smallest shape at which the engine keeps its masks as halves): the half forms of both
    kernels run, the table is within 2e-2 (the project's fp16 mask tolerance; a mean cannot be further off than its terms) of the float64 mean of the
    oracle's fp32 masks, and every stem is within rel-RMS 1e-2 of the oracle under the rule"""
    import torch
    import spleeterrt_amd as srt
    T, F, S = 256, 1024, 4
    n = 4 * T * 1024 - 77
    Lh, Rh = _noisy_host(oracle, n, 48, F)
    eng = _engine(coeffs, S=S, F=F, T=T, max_tiles=4, precision=srt.PREC_F16, mask_extension="average")
    L, R = torch.from_numpy(Lh).cuda(), torch.from_numpy(Rh).cuda()
    eng.separate(L, R)
    got, ks = _timed(eng, lambda: eng.separate(L, R).cpu().numpy())
    assert tuple(ks[-2:]) == _ext_names(F, m16=True), ks[-2:]
    _, _, _, re_, im_ = _AUDIO[(n, 48)]
    rows = re_.shape[1]
    assert rows == 4 * T
    tab = _table(eng, rows)
    eng.close()
    masks = np.empty((S, 4, 2, T, F), np.float32)
    for j in range(4):
        mag = oracle.magnitude_tile(re_, im_, j * T, T, F)
        for s in range(S):
            masks[s, j] = oracle.forward(coeffs(s), mag, MODES[s], oracle.VARIANT_VST)
    m = _blend_rows(masks, rows, T, 0)
    terr = float(np.abs(tab - m.astype(np.float64).mean(axis=-1).transpose(0, 2, 1)).max())
    print("half masks: table against the oracle masks' float64 mean %.3g" % terr)
    assert terr <= 2e-2, terr
    ref = _apply_average(oracle, re_, im_, m, F)
    assert got.shape == ref.shape and np.isfinite(got).all()
    for s in range(S):
        rr = _rel_rms(got[s], ref[s])
        print("half masks stem %d: rel-RMS %.3g" % (s, rr))
        assert rr <= 1e-2, (s, rr)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_writes_every_sample_and_nothing_past(oracle, coeffs, F):
    """mode on: the whole [n_stems][2][srtIstftLength(rows)] region is written, nothing behind it is touched"""
    import torch
    eng = _engine(coeffs, S=2, F=F, max_tiles=8, mask_extension="average")
    L, R = _noisy(oracle, N_RAGGED, 49, F)
    need = 2 * 2 * eng.L.srtIstftLength(eng.L.srtStftRows(N_RAGGED))
    out = torch.full((need + 5000,), float("nan"), device="cuda")
    out[need:] = 12345.0
    eng.separate(L, R, out)
    h = out.cpu().numpy()
    assert np.isfinite(h[:need]).all(), int(np.isnan(h[:need]).sum())
    assert (h[need:] == 12345.0).all()
    eng.close()


@pytest.mark.gpu
def test_refusals(oracle, coeffs):
    """srtSeparateCli, srtIstftWiener and srtSetWiener(1) with the mode on, srtSetMaskExtension(AVERAGE) with the Wiener filter on and an unknown mode all
    return -1 with a message, write nothing, and leave an engine that still works"""
    import torch
    import spleeterrt_amd as srt
    eng = _engine(coeffs, S=2, max_tiles=8, batch_invariant=True)
    Lq, vp = eng.L, C.c_void_p
    n = 100 * 1024 + 300
    rows = Lq.srtStftRows(n)
    ln = Lq.srtIstftLength(rows)
    Ld, Rd = _noisy(oracle, n, 50, 512)
    spec, mag = eng.stft(Ld, Rd)
    masks = eng.forward(mag)
    before = eng.separate(Ld, Rd).clone()
    d_out = torch.empty((3, 2, ln), device="cuda")
    eng.set_mask_extension("average")
    calls = {
        "srtSeparateCli": lambda: Lq.srtSeparateCli(eng.h, vp(Ld.data_ptr()), vp(Rd.data_ptr()), n, 2, vp(d_out.data_ptr())),
        "srtIstftWiener": lambda: Lq.srtIstftWiener(eng.h, vp(spec.data_ptr()), rows, vp(masks.data_ptr()), 1, vp(d_out.data_ptr())),
        "srtSetWiener": lambda: Lq.srtSetWiener(eng.h, 1),
    }
    for name, call in calls.items():
        d_out.fill_(float("nan"))
        assert call() == -1, name
        msg = Lq.srtLastError()
        assert name.encode() in msg and b"mask extension" in msg and b"srtSetMaskExtension" in msg, (name, msg)
        torch.cuda.synchronize()
        assert bool(torch.isnan(d_out).all()), name
    with pytest.raises(srt.EngineError, match="mask extension"):
        eng.separate_cli(Ld, Rd, 3)
    for bad in (-1, 2, 99):
        assert Lq.srtSetMaskExtension(eng.h, bad) == -1 and b"srtSetMaskExtension" in Lq.srtLastError(), bad
    with pytest.raises(srt.EngineError):
        eng.set_mask_extension("zeros")
    assert eng.mask_extension == srt.MASK_EXT_AVERAGE
    on = eng.separate(Ld, Rd)
    assert torch.isfinite(on).all() and not torch.equal(on, before)
    eng.set_mask_extension("constant")
    eng.set_wiener(1)
    assert Lq.srtSetMaskExtension(eng.h, srt.MASK_EXT_AVERAGE) == -1 and b"Wiener" in Lq.srtLastError()
    assert Lq.srtSetMaskExtension(eng.h, srt.MASK_EXT_CONSTANT) == 0
    assert torch.isfinite(eng.separate(Ld, Rd)).all()
    eng.set_wiener(0)
    assert torch.equal(eng.separate(Ld, Rd), before)
    assert Lq.srtSeparateCli(eng.h, vp(Ld.data_ptr()), vp(Rd.data_ptr()), n, 2, vp(d_out.data_ptr())) == 0
    eng.close()
