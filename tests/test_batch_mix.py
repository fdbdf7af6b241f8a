"""srtSeparateBatchMix: the stem remix of srtSetMix per track of a packed batch (§10.3) - one matrix per track, an argument of the call.

CPU: the declaration and the symbol, the null-engine call, the eight srt_istft_batch_bus_kernel forms and their resources against the single-signal mix kernels
whose bodies they run.  GPU: every track of one call against srtSeparate of that track alone after srtSetOverlap(O) and srtSetMix(G_k) (bit for bit under
batch_invariant; both kernel families; overlap, ratio_mask, the average extension; the fp16 mode), one-hot rows against srtSeparateBatchOverlap's stems,
n_out = 0, gain_stride = 0, isolation of one track's matrix, linearity against a float64 sum of the mix-off results, the default mode, coverage, the slot
ring, the engine's own settings, every refusal, and the Python grouping.

Bounds, none taken from what the kernels give: bit equality wherever the arithmetic is the same; linearity at tests/test_mix.py's
CAP x (peak_m + sum_s |G[m][s]| peak_s + |G[m][S]| peak_dry); the default mode at tests/test_batch_overlap.py's 1e-5 of the peak."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_batch_overlap as B
import test_mix as M

T_S, S3 = M.T_S, M.S3
FS = M.FS                                                # 576: three-per-CU family, the band edge inside a thread's bins; 1088: the table family
TRACKS = B.TRACKS_OV                                     # rows 160, 4, 65, 64, 137: 10 / 12 packed tiles at O = 16 / 32
MAX_TILES = B.MAX_TILES
N_OUT = 2
# one matrix per track [n_out][S + 1]: one-hot rows, the cancelling row (1, 1, 1 | -1), the dry row (0, 0, 0 | 1), karaoke, fractional gains
GS = np.array([[(1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0)],
               [(1.0, 1.0, 1.0, -1.0), (0.0, 0.0, 0.0, 1.0)],
               [(0.5, 0.25, 1.0, 0.0), (-0.5, 0.0, 0.125, 0.75)],
               [(0.0, 1.0, 0.0, 0.0), (0.25, 0.5, 0.125, 0.25)],
               [(0.0, -1.0, 0.0, 1.0), (1.0, 0.0, 1.0, 0.0)]], np.float32)
GW = N_OUT * (S3 + 1)
BUS_KERNELS = sorted("srt_istft_batch_bus_kernel<%s, %s, %s>" % (a, b, c) for a in ("false", "true") for b in ("false", "true") for c in ("false", "true"))
DECL = ("SRT_API int  srtSeparateBatchMix(srt_engine *e, int ntracks, const float *const *d_L, const float *const *d_R,\n"
        "                                 const size_t *n, float *const *d_out, int overlap_rows,\n"
        "                                 int n_out, const float *h_gain, size_t gain_stride);")


def _bus_kernel(F, O, ext=False):
    return "srt_istft_batch_bus_kernel<%s>" % ", ".join("true" if x else "false" for x in (F <= 1024, O > 0, ext))


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_abi():
    from spleeterrt_amd import capi
    L = M._lib()
    assert L.srtSeparateBatchMix is not None
    hdr = open(os.path.join(M.ROOT, "include", "spleeterrt_amd.h")).read()
    assert re.sub(r"\s+", " ", DECL) in re.sub(r"\s+", " ", hdr)
    assert "mix" in capi.Engine.separate_batch.__code__.co_varnames
    assert GS.shape == (len(TRACKS), N_OUT, S3 + 1)


def test_null_engine():
    L = M._lib()
    P1 = C.c_void_p * 1
    g = (C.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    for n_out, gain in ((1, g), (0, None), (1, None), (9, g)):               # a null engine is refused first, whatever the other arguments
        assert L.srtSeparateBatchMix(None, 1, P1(None), P1(None), (C.c_size_t * 1)(4096), P1(None), 16, n_out, gain, 0) == -1
        assert b"srtSeparateBatchMix" in L.srtLastError()


def test_bus_kernels_resources():
    """srt_dsp.hip compiled with the resource remarks (the recipe of test_mix.py::test_mix_kernels_resources): exactly the eight batch forms exist, each without
    scratch or spilled VGPRs and with at least the occupancy of the single-signal mix kernel whose body it runs.  (The F > 1024 siblings sit at 227-247 VGPRs: a
    track look-up or a matrix row held in vector registers would spill there.)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the resource check needs the compiler the library is built with")
    src = os.path.join(M.ROOT, "spleeterrt_amd", "csrc", "srt_dsp.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + M.ROOT + "/include", "-I" + M.ROOT + "/spleeterrt_amd/csrc",
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
    bus = sorted(k for k in res if "batch_bus" in k)
    assert bus == BUS_KERNELS, bus
    for k in bus:
        ola3, ov, ext = re.match(r"srt_istft_batch_bus_kernel<(\w+), (\w+), (\w+)>$", k).groups()
        sib = "srt_istft_ola3_mix_kernel<4, %s, %s>" % (ov, ext) if ola3 == "true" else "srt_istft_ola_mix_kernel<%s, %s>" % (ov, ext)
        a, b = res[k], res[sib]
        print("%-52s vgpr %s sgpr %s scratch %s spilled vgprs %s occupancy %s | %s vgpr %s occupancy %s" % (
            k, a["VGPRs"], a["TotalSGPRs"], a["ScratchSize [bytes/lane]"], a["VGPRs Spill"], a["Occupancy [waves/SIMD]"], sib, b["VGPRs"], b["Occupancy [waves/SIMD]"]))
        assert int(a["ScratchSize [bytes/lane]"]) == 0 and int(a["VGPRs Spill"]) == 0, (k, a)
        assert int(a["Occupancy [waves/SIMD]"]) >= int(b["Occupancy [waves/SIMD]"]) >= 2, (k, a, b)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _engine(coeffs, **kw):
    kw.setdefault("max_tiles", MAX_TILES)
    return M._engine(coeffs, **kw)


def _tracks(oracle, F, seed=3100):
    """the five tracks as seeded noisy audio with >= 10 % of the energy above F (asserted on the CPU by test_mix._noisy_host)"""
    return [M._noisy(oracle, n, seed + k, F) for k, n in enumerate(TRACKS)]


def _gptr(G):
    G = np.array(G, np.float32, order="C")                              # (a copy: callers overwrite it)
    return G, G.ctypes.data_as(C.POINTER(C.c_float))


def _mix_call(eng, tr, outs, O, G, n_out=N_OUT, stride=None):
    """one raw srtSeparateBatchMix; G [ntracks][n_out][S + 1] (or one matrix with stride = 0)"""
    G, p = _gptr(G)
    return B._raw_call(eng, eng.L.srtSeparateBatchMix, tr, outs, O, n_out, p, GW if stride is None else stride)


def _outs(eng, tr, planes=N_OUT, fill=float("nan")):
    import torch
    L = eng.L
    return [torch.full((planes, 2, L.srtIstftLength(L.srtStftRows(int(a.numel())))), fill, device="cuda") for a, _ in tr]


def _singles(eng, tr, O, G):
    """separate() per track after set_overlap(O) and set_mix(G[k]); the overlap is put back and the mix switched off"""
    own = eng.overlap
    eng.set_overlap(O)
    out = []
    for k, (L, R) in enumerate(tr):
        eng.set_mix(G[k])
        out.append(eng.separate(L, R).clone())
    eng.set_mix(None)
    eng.set_overlap(own)
    return out


CASES = {"plain": (0, False, "constant"), "overlap": (16, False, "constant"), "ratio": (0, True, "constant"),
         "overlap+ratio+average": (16, True, "average"), "overlap32+average": (32, False, "average")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("F", FS)
def test_bit_identical_to_single_tracks(oracle, coeffs, F, case):
    """batch_invariant: every track's outputs from ONE call are bit for bit separate() of that track alone after set_overlap(O) and set_mix(G_k); one
    istft_batch launch, the form for this F, overlap and extension"""
    import torch
    O, ratio, ext = CASES[case]
    eng = _engine(coeffs, F=F, batch_invariant=True, ratio_mask=ratio, mask_extension=ext)
    tr = _tracks(oracle, F)
    got, ks = M._timed(eng, lambda: eng.separate_batch(tr, overlap=O, mix=GS))
    names = [n for n, _ in ks]
    assert names.count("stft_batch") == 1 and names.count("istft_batch") == 1, names
    assert ks[-1] == ("istft_batch", _bus_kernel(F, O, ext == "average")), ks[-1]
    assert eng.mix_outputs == 0 and eng.overlap == 0
    ref = _singles(eng, tr, O, GS)
    for k in range(len(tr)):
        assert got[k].shape == ref[k].shape and got[k].shape[0] == N_OUT
        assert torch.equal(got[k], ref[k]), (case, k, float((got[k] - ref[k]).abs().max()))
    eng.close()


@pytest.mark.gpu
def test_bit_identical_in_the_fp16_mode(oracle, coeffs):
    """the fp16 mode at F = 512 (its storage needs F % 256 == 0): the masks of this call are floats, as under set_mix, so the comparison is bits again"""
    import torch
    import spleeterrt_amd as srt
    F, O = 512, 16
    eng = _engine(coeffs, F=F, batch_invariant=True, precision=srt.PREC_F16)
    tr = _tracks(oracle, F)
    got, ks = M._timed(eng, lambda: eng.separate_batch(tr, overlap=O, mix=GS))
    assert ks[-1] == ("istft_batch", _bus_kernel(F, O)), ks[-1]
    ref = _singles(eng, tr, O, GS)
    for k in range(len(tr)):
        assert torch.equal(got[k], ref[k]), (k, float((got[k] - ref[k]).abs().max()))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", FS)
def test_one_hot_rows_are_the_batch_stems(oracle, coeffs, F):
    """fp32: a row that is 1 on stem s gives stem s of srtSeparateBatchOverlap bit for bit (fmaf(0, g, h) = h, fmaf(1, g, 0) = g)"""
    import torch
    O = 16
    eng = _engine(coeffs, F=F, batch_invariant=True)
    tr = _tracks(oracle, F)
    stems = [o.clone() for o in eng.separate_batch(tr, overlap=O)]
    pick = [(k % S3, (k + 1) % S3) for k in range(len(tr))]
    G = np.zeros((len(tr), N_OUT, S3 + 1), np.float32)
    for k, (a, b) in enumerate(pick):
        G[k, 0, a] = 1.0
        G[k, 1, b] = 1.0
    got = eng.separate_batch(tr, overlap=O, mix=G)
    for k, (a, b) in enumerate(pick):
        assert torch.equal(got[k][0], stems[k][a]) and torch.equal(got[k][1], stems[k][b]), k
    eng.close()


@pytest.mark.gpu
def test_n_out_zero_is_separate_batch_overlap(oracle, coeffs):
    """n_out = 0: srtSeparateBatchOverlap's kernel list and bits; h_gain and gain_stride are ignored"""
    import torch
    F, O = FS[0], 16
    eng = _engine(coeffs, F=F, batch_invariant=True)
    tr = _tracks(oracle, F)
    eng.separate_batch(tr, overlap=O)                                    # (first call allocates the table)
    want = _outs(eng, tr, S3)
    rc, ks0 = M._timed(eng, lambda: B._raw_call(eng, eng.L.srtSeparateBatchOverlap, tr, want, O))
    assert rc == 0, eng.L.srtLastError()
    outs = _outs(eng, tr, S3)
    rc, ks1 = M._timed(eng, lambda: B._raw_call(eng, eng.L.srtSeparateBatchMix, tr, outs, O, 0, None, 3))
    assert rc == 0, eng.L.srtLastError()
    assert ks0 == ks1 and ks1[-1][1].startswith("srt_istft_batch_ov_kernel"), ks1[-1]
    for k in range(len(tr)):
        assert torch.isfinite(outs[k]).all() and torch.equal(outs[k], want[k]), k
    eng.close()


@pytest.mark.gpu
def test_gain_stride_zero_and_isolation(oracle, coeffs):
    """gain_stride = 0 equals the same matrix repeated per track (also at a stride wider than the matrix); changing only track 2's matrix changes track 2's
    outputs and no other track's bits"""
    import torch
    F, O = FS[1], 16
    eng = _engine(coeffs, F=F, batch_invariant=True)
    tr = _tracks(oracle, F)
    one = GS[2]
    a, b, c = _outs(eng, tr), _outs(eng, tr), _outs(eng, tr)
    assert _mix_call(eng, tr, a, O, one, stride=0) == 0, eng.L.srtLastError()
    assert _mix_call(eng, tr, b, O, np.stack([one] * len(tr))) == 0, eng.L.srtLastError()
    wide = np.full((len(tr), GW + 3), 7.0, np.float32)                   # (the three floats between the matrices are never read as gains)
    wide[:, :GW] = one.reshape(-1)
    assert _mix_call(eng, tr, c, O, wide, stride=GW + 3) == 0, eng.L.srtLastError()
    for k in range(len(tr)):
        assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    base, moved = _outs(eng, tr), _outs(eng, tr)
    G2 = GS.copy()
    G2[2] = GS[4]
    assert _mix_call(eng, tr, base, O, GS) == 0 and _mix_call(eng, tr, moved, O, G2) == 0, eng.L.srtLastError()
    for k in range(len(tr)):
        assert torch.equal(base[k], moved[k]) == (k != 2), k
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [False, True])
@pytest.mark.parametrize("F", FS)
def test_linearity_against_float64(oracle, coeffs, F, ratio):
    """output m of track k against sum_s G_k[m][s] stem_s + G_k[m][S] dry, formed in float64 from the mix-off batch stems and the mask-free round trip; the bound
    of tests/test_mix.py::test_linearity_end_to_end (its _linearity)"""
    O = 16
    tr = _tracks(oracle, F)
    eng = _engine(coeffs, F=F, ratio_mask=ratio)
    stems = [o.cpu().numpy() for o in eng.separate_batch(tr, overlap=O)]
    mix = [o.cpu().numpy() for o in eng.separate_batch(tr, overlap=O, mix=GS)]
    eng.close()
    dry_eng = M._engine(None, S=1, F=F, max_tiles=3, oob_weights=(1.0,))
    for k, (L, R) in enumerate(tr):
        spec, _ = dry_eng.stft(L, R, want_mag=False)
        dry = dry_eng.istft(spec, None)[0].cpu().numpy()
        assert mix[k].shape == (N_OUT, 2, stems[k].shape[2])
        M._linearity("F=%d ratio=%d track %d" % (F, ratio, k), mix[k], GS[k], stems[k], dry)
    dry_eng.close()


@pytest.mark.gpu
def test_default_mode_matches_single_tracks(oracle, coeffs):
    """not batch_invariant: max-abs <= 1e-5 of the peak against the single calls, the bound of tests/test_batch_overlap.py's default-mode case.  (Where a row
    cancels, the peak is that of the track's largest output: the error of a sum does not shrink with the sum.)"""
    F, O = FS[0], 16
    eng = _engine(coeffs, F=F)
    tr = _tracks(oracle, F)
    got = [o.cpu().numpy() for o in eng.separate_batch(tr, overlap=O, mix=GS)]
    ref = [o.cpu().numpy() for o in _singles(eng, tr, O, GS)]
    eng.close()
    for k in range(len(tr)):
        assert got[k].shape == ref[k].shape
        peak = float(np.abs(ref[k]).max())
        err = float(np.abs(got[k] - ref[k]).max())
        print("default mode track %d: max-abs / peak = %.3g" % (k, err / peak))
        assert err <= 1e-5 * peak, (k, err / peak)


@pytest.mark.gpu
@pytest.mark.parametrize("F", FS)
def test_writes_every_plane_and_nothing_past(oracle, coeffs, F):
    """outputs pre-filled with NaN and one guard plane behind each: all n_out planes are finite afterwards, the guard keeps its pattern"""
    import torch
    eng = _engine(coeffs, F=F)
    tr = _tracks(oracle, F)
    L = eng.L
    plane = [L.srtIstftLength(L.srtStftRows(n)) for n in TRACKS]
    for O in (0, 32):
        outs = [torch.full(((N_OUT * 2 + 1) * p,), float("nan"), device="cuda") for p in plane]
        for o, p in zip(outs, plane):
            o[N_OUT * 2 * p:] = 12345.0
        eng.separate_batch(tr, outs, overlap=O, mix=GS)
        for k, (o, p) in enumerate(zip(outs, plane)):
            h = o.cpu().numpy()
            assert np.isfinite(h[:N_OUT * 2 * p]).all(), (O, k, int(np.isnan(h[:N_OUT * 2 * p]).sum()))
            assert (h[N_OUT * 2 * p:] == 12345.0).all(), (O, k)
    eng.close()


@pytest.mark.gpu
def test_slot_ring(oracle, coeffs):
    """six back-to-back calls with six matrix sets and no synchronisation in between (the ring has four pinned slots): each call gives its own matrices'
    result, which is the result of the same call issued alone"""
    import torch
    F, O = FS[0], 16
    eng = _engine(coeffs, F=F, batch_invariant=True)
    tr = _tracks(oracle, F)
    sets = [np.ascontiguousarray(np.roll(GS, i, axis=0) * np.float32(1.0 - 0.125 * i)) for i in range(6)]
    alone = []
    for G in sets:
        o = _outs(eng, tr)
        assert _mix_call(eng, tr, o, O, G) == 0, eng.L.srtLastError()
        torch.cuda.synchronize()
        alone.append(o)
    torch.cuda.synchronize()
    ring = [_outs(eng, tr) for _ in sets]
    torch.cuda.synchronize()
    for G, o in zip(sets, ring):
        G, p = _gptr(G)
        assert B._raw_call(eng, eng.L.srtSeparateBatchMix, tr, o, O, N_OUT, p, GW) == 0, eng.L.srtLastError()
        G[:] = np.nan                                                   # (h_gain is copied by the call: the caller's memory is free at once)
    torch.cuda.synchronize()
    for i in range(len(sets)):
        for k in range(len(tr)):
            assert torch.equal(ring[i][k], alone[i][k]), (i, k)
        if i:
            assert not torch.equal(ring[i][0], ring[i - 1][0]), i
    eng.close()


@pytest.mark.gpu
def test_engine_state_is_neither_read_nor_changed(oracle, coeffs):
    """with the engine's own set_mix and set_overlap on, the call succeeds and uses its arguments only; mix_outputs and overlap are unchanged afterwards and a
    following separate() gives the bits it gave before"""
    import torch
    F = FS[0]
    eng = _engine(coeffs, F=F, batch_invariant=True)
    tr = _tracks(oracle, F)
    own = np.array([(0.25, 0.0, 0.5, 0.125)], np.float32)
    ref = _singles(eng, tr, 32, GS)
    eng.set_overlap(16)
    eng.set_mix(own)
    before = eng.separate(*tr[0]).clone()
    outs = _outs(eng, tr)
    assert _mix_call(eng, tr, outs, 32, GS) == 0, eng.L.srtLastError()
    assert eng.mix_outputs == 1 and eng.overlap == 16
    after = eng.separate(*tr[0])
    assert after.shape[0] == 1 and torch.equal(after, before)
    for k in range(len(tr)):
        assert torch.equal(outs[k], ref[k]), k
    # the calls without a mix argument keep refusing while the engine's mix is on
    assert B._raw_call(eng, eng.L.srtSeparateBatchOverlap, tr, outs, 16) == -1 and b"mix" in eng.L.srtLastError()
    eng.close()


@pytest.mark.gpu
def test_refusals(oracle, coeffs):
    """every refusal: -1 with text that names the entry point and sentinel-filled outputs left untouched; -5 for unset weights.  All of them are host-side
    argument checks"""
    import torch
    import spleeterrt_amd as srt
    F = FS[0]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                   # (a non-default stream, so that the capture case below can capture it)
        eng = _engine(coeffs, F=F)
    L = eng.L
    fn = L.srtSeparateBatchMix
    tr = _tracks(oracle, F)
    outs = _outs(eng, tr, S3)                                       # (room for S planes: the n_out = 0 refusals would write the stems)
    torch.cuda.synchronize()
    G, gp = _gptr(GS)
    k = len(tr)
    P = C.c_void_p * k
    Lp, Rp, Op = [a.data_ptr() for a, _ in tr], [b.data_ptr() for _, b in tr], [o.data_ptr() for o in outs]
    ns = (C.c_size_t * k)(*TRACKS)

    def refused(rc, *words):
        msg = L.srtLastError()
        assert rc == -1 and b"srtSeparateBatchMix" in msg and all(w in msg for w in words), (rc, msg)

    for bad in (-1, T_S // 2 + 1, T_S):
        refused(B._raw_call(eng, fn, tr, outs, bad, N_OUT, gp, GW), b"overlap")
    for bad in (-1, srt.capi.MAX_STEMS + 1):
        refused(B._raw_call(eng, fn, tr, outs, 16, bad, gp, GW), b"n_out")
    refused(B._raw_call(eng, fn, tr, outs, 16, N_OUT, None, GW), b"null")
    refused(B._raw_call(eng, fn, tr, outs, 16, N_OUT, gp, GW - 1), b"gain_stride")
    for val in (float("nan"), float("inf")):
        Gb, gb = _gptr(GS)
        Gb[3, 1, 2] = val
        refused(B._raw_call(eng, fn, tr, outs, 16, N_OUT, gb, GW), b"track 3", b"finite")
    eng.set_wiener(1)
    refused(B._raw_call(eng, fn, tr, outs, 16, N_OUT, gp, GW), b"Wiener")
    refused(B._raw_call(eng, fn, tr, outs, 0, 0, None, 0), b"Wiener")
    eng.set_wiener(0)
    # what srtSeparateBatchOverlap refuses
    refused(fn(eng.h, k, P(*([Lp[0], None] + Lp[2:])), P(*Rp), ns, P(*Op), 16, N_OUT, gp, GW), b"null")
    refused(fn(eng.h, k, P(*Lp), P(*Rp), ns, P(*(Op[:4] + [None])), 16, N_OUT, gp, GW), b"null")
    refused(fn(eng.h, k, None, P(*Rp), ns, P(*Op), 16, N_OUT, gp, GW), b"arrays")
    refused(fn(eng.h, k, P(*Lp), P(*Rp), (C.c_size_t * k)(TRACKS[0], 4095, *TRACKS[2:]), P(*Op), 16, N_OUT, gp, GW), b"4096")
    refused(fn(eng.h, 0, P(*Lp), P(*Rp), ns, P(*Op), 16, N_OUT, gp, GW))
    small = _engine(coeffs, F=F, max_tiles=9)                       # the list takes 10 overlapped tiles at O = 16
    refused(B._raw_call(small, fn, tr, outs, 16, N_OUT, gp, GW), b"max_tiles")
    small.close()
    bare = srt.Engine(F=F, T=T_S, stem_modes=M.MODES[:S3], variant=srt.VARIANT_VST, max_tiles=MAX_TILES)
    assert B._raw_call(bare, fn, tr, outs, 16, N_OUT, gp, GW) == -5 and b"weights" in L.srtLastError() and b"srtSeparateBatchMix" in L.srtLastError()
    bare.close()
    torch.cuda.synchronize()
    dummy = torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                      # the engine's stream is capturing: refused before anything is enqueued
        dummy += 1.0                                                # (so that the captured graph is not empty)
        rc = B._raw_call(eng, fn, tr, outs, 16, N_OUT, gp, GW)
        msg = L.srtLastError()
    assert rc == -1 and b"capture" in msg and b"srtSeparateBatchMix" in msg, (rc, msg)
    del graph
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)
    with torch.cuda.stream(side):                                   # ... and the same arguments without a fault in them run
        assert B._raw_call(eng, fn, tr, outs, 16, N_OUT, gp, GW) == 0, L.srtLastError()
        side.synchronize()
    assert all(bool(torch.isfinite(o[:N_OUT]).all()) for o in outs)
    eng.close()


@pytest.mark.gpu
def test_python_splits_into_calls(oracle, coeffs):
    """max_tiles = 4 at O = 16 cuts the list into three srtSeparateBatchMix calls: per-track matrices follow their tracks; one matrix serves every track; mix
    with wiener raises before any call; mix=None returns [S, 2, len] as before"""
    import torch
    import spleeterrt_amd as srt
    from spleeterrt_amd import stream
    F, O = FS[0], 16
    groups = stream.pack_tracks(TRACKS, T_S, 4, overlap=O)
    assert [g.tracks for g in groups] == [[0, 1], [2, 3], [4]]
    eng = _engine(coeffs, F=F, max_tiles=4, batch_invariant=True)
    tr = _tracks(oracle, F)
    got, ks = M._timed(eng, lambda: eng.separate_batch(tr, overlap=O, mix=[GS[k] for k in range(len(tr))]))
    assert [kn for n, kn in ks if n == "istft_batch"] == [_bus_kernel(F, O)] * 3, ks
    ref = _singles(eng, tr, O, GS)
    for k in range(len(tr)):
        assert got[k].shape[0] == N_OUT and torch.equal(got[k], ref[k]), k
    same = eng.separate_batch(tr, overlap=O, mix=GS[2])
    ref = _singles(eng, tr, O, [GS[2]] * len(tr))
    for k in range(len(tr)):
        assert torch.equal(same[k], ref[k]), k
    nan = [torch.full_like(o, float("nan")) for o in got]
    with pytest.raises(srt.EngineError, match="Wiener"):
        eng.separate_batch(tr, nan, wiener=1, mix=GS)
    with pytest.raises(srt.EngineError, match="mix"):
        eng.separate_batch(tr, nan, overlap=O, mix=[GS[0], GS[1][:1], GS[2], GS[3], GS[4]])      # two n_out in one list
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in nan)
    plain = eng.separate_batch(tr, overlap=O, mix=None)
    want = eng.separate_batch(tr, overlap=O)
    for k in range(len(tr)):
        assert plain[k].shape[0] == S3 and torch.equal(plain[k], want[k]), k
    eng.close()
