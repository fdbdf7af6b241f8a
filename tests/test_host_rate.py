"""Host streams at the caller's sample rate (srtSeparateHostStreamRate).

CPU: srtHostRateLength / srtHostRatePieces against stream.host_rate_pieces and against the four properties of the plan checked from the converter's geometry
formulas (ten input rates x six output rates x four tile configurations x six lengths = 1 440 plans); both rates 44100 = srtHostOverlapPieces; the refusals that
need no device.  GPU (T = 64, F = 512, three stems, batch_invariant, about 6.4 s of audio): np.array_equal with the composition resample_host -> separate_host_stream_io
/ separate_host_overlap -> resample_host per pair, for five rate cases, max_tiles 1 (every seam through the carry) and 3, overlaps 0 and 16; ratio_mask, the average
extension, a one-output mix, 16-bit in, 16-bit out with clipping; both rates 44100 = separate_host_overlap's bits and launches; the timer names; one piece; a control
whose carry is lost; the refusals that need a device."""
import ctypes as C

import numpy as np
import pytest

from test_overlap import N_RAGGED, _engine
from test_pcm16 import rule

T_S = 64
SEED = 41
IN_RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 384000)
OUT_RATES = (8000, 22050, 44100, 48000, 96000, 384000)
TILINGS = ((64, 0, 1), (64, 16, 3), (64, 32, 1), (256, 64, 2))          # T, O, max_tiles


def _lib():
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def _geometry(fs_in, fs_out):
    """srt_rs_geometry's formulas for the built-in filter (22 438 points, 491 per input sample), written out here"""
    from math import gcd
    g = gcd(fs_in, fs_out)
    fi = 491 * min(fs_out / fs_in, 1.0)
    inc = int(np.rint(fi * 4096.0))
    half = ((22438 - 2) << 12) // inc
    return fs_in // g, fs_out // g, half, (2 * half + 2 + 3) // 4 * 4


def _sample(lo, hi, rng):
    """both ends of [lo, hi) and up to 500 frames between them"""
    if hi <= lo:
        return np.zeros(0, np.int64)
    return np.unique(np.concatenate([[lo, hi - 1], rng.integers(lo, hi, size=min(500, hi - lo))])).astype(np.int64)


def test_plan_against_the_mirror_and_the_four_properties():
    from spleeterrt_amd import capi, stream
    rng = np.random.default_rng(5)
    cases = 0
    for fi in IN_RATES:
        for fo in OUT_RATES:
            for T, O, P in TILINGS:
                n44s = [4096, P * T * 1024 + 3072, P * (T - O) * 1024 * 2 + 1] + [int(v) for v in rng.integers(4096, 4 * P * T * 1024, size=3)]
                for n44 in n44s:
                    n = max(-(-n44 * fi // 44100), 1)
                    while stream.resample_length(n, fi, 44100) < 4096 and fi != 44100:
                        n += 1
                    cases += 1
                    got = capi.host_rate_pieces(n, fi, fo, T, O, P)
                    assert got == stream.host_rate_pieces(n, fi, fo, T, O, P), (n, fi, fo, T, O, P)
                    len_out = capi.host_rate_length(n, fi, fo)
                    assert len_out == stream.host_rate_length(n, fi, fo)
                    n44r = n if fi == 44100 else stream.resample_length(n, fi, 44100)
                    rows = stream.stft_rows(n44r)
                    len44 = rows * 1024 + 3072
                    assert len_out == (len44 if fo == 44100 else stream.resample_length(len44, 44100, fo))
                    ov = stream.host_overlap_pieces(rows, T, O, P)
                    assert len(got) == len(ov)
                    # the 44.1 kHz side is the overlap plan's
                    for c, (p, q) in enumerate(zip(got, ov)):
                        last = c + 1 == len(got)
                        assert p["s0"] == q["row0"] * 1024 and p["s0"] + p["ns"] == min((q["row0"] + q["stft_rows"]) * 1024 + 3072, n44r)
                        assert p["fin0"] == p["s0"] and p["fin1"] == (len44 if last else p["s0"] + q["own_rows"] * 1024)
                    if fi == 44100:
                        assert all((p["src0"], p["src_len"]) == (p["s0"], p["ns"]) for p in got)
                    else:
                        Pi, Qi, LO, T4 = _geometry(fi, 44100)
                        for p in got:
                            # 1: every weighted tap (window taps 0 .. 2 LO + 1) of the piece's 44.1 kHz frames lies in the uploaded window or outside [0, n)
                            j = _sample(p["s0"], p["s0"] + p["ns"], rng)
                            first, lastt = j * Pi // Qi - LO, j * Pi // Qi + LO + 1
                            assert 0 <= p["src0"] and p["src0"] + p["src_len"] <= n
                            assert ((first >= p["src0"]) | (first < 0)).all() and ((lastt < p["src0"] + p["src_len"]) | (lastt >= n)).all(), (n, fi, fo, T, O, P, p)
                            assert ((np.maximum(first, 0) >= p["src0"]) & (np.minimum(lastt, n - 1) < p["src0"] + p["src_len"])).all()
                            # and the window is the issue's formula
                            assert p["src0"] == max(0, p["s0"] * Pi // Qi - LO) and p["src0"] + p["src_len"] == min(n, (p["s0"] + p["ns"] - 1) * Pi // Qi - LO + T4)
                    if fo == 44100:
                        assert all((p["out0"], p["out1"]) == (p["fin0"], p["fin1"]) for p in got)
                    else:
                        Po, Qo, LO, _ = _geometry(44100, fo)
                        # 2: the output ranges tile [0, len_out)
                        assert got[0]["out0"] == 0 and got[-1]["out1"] == len_out and all(a["out1"] == b["out0"] for a, b in zip(got, got[1:]))
                        for c, p in enumerate(got):
                            assert p["out0"] <= p["out1"]
                            j = _sample(p["out0"], p["out1"], rng)
                            i = j * Po // Qo
                            # 3: no frame needs history older than 2 LO + 1 samples before the piece's first finalised sample
                            assert (i - LO >= p["fin0"] - (2 * LO + 1)).all(), (n, fi, fo, T, O, P, p)
                            # 4: no frame of a piece that is not the last needs a sample at or after fin1
                            if c + 1 < len(got):
                                assert (i + LO + 1 < p["fin1"]).all(), (n, fi, fo, T, O, P, p)
                                assert p["fin1"] - p["fin0"] >= 2 * LO + 1            # the carry can be filled from one piece
                                # ... and the range is not cut short: the next frame does
                                assert p["out1"] == len_out or p["out1"] * Po // Qo + LO + 1 >= p["fin1"]
    assert cases == 1440


def test_both_rates_44100_is_the_overlap_plan():
    from spleeterrt_amd import capi, stream
    for T, O, P in TILINGS:
        for n in (4096, N_RAGGED, 3 * P * T * 1024 + 777):
            rows = stream.stft_rows(n)
            ov = capi.host_overlap_pieces(rows, T, O, P)
            got = capi.host_rate_pieces(n, 44100, 44100, T, O, P)
            want = [dict(src0=q["row0"] * 1024, src_len=min((q["row0"] + q["stft_rows"]) * 1024 + 3072, n) - q["row0"] * 1024,
                         s0=q["row0"] * 1024, ns=min((q["row0"] + q["stft_rows"]) * 1024 + 3072, n) - q["row0"] * 1024,
                         fin0=q["row0"] * 1024, fin1=(q["row0"] + q["own_rows"]) * 1024 + (3072 if c + 1 == len(ov) else 0),
                         out0=q["row0"] * 1024, out1=(q["row0"] + q["own_rows"]) * 1024 + (3072 if c + 1 == len(ov) else 0)) for c, q in enumerate(ov)]
            assert got == want, (T, O, P, n)
            assert capi.host_rate_length(n, 44100, 44100) == rows * 1024 + 3072


def test_refusals_without_a_device():
    from spleeterrt_amd import capi, stream
    L = _lib()
    cfg = capi._Config()
    cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles = 512, 64, 3, 2
    ok = (C.byref(cfg), 300000, 48000, 48000, 16)
    assert L.srtHostRatePieces(*ok, None, 0) == 3
    bad_cfg = capi._Config()
    bad_cfg.F, bad_cfg.T, bad_cfg.n_stems, bad_cfg.max_tiles = 512, 60, 3, 2
    for name, args in (("null config", (None,) + ok[1:]), ("bad config", (C.byref(bad_cfg),) + ok[1:]), ("input rate below", ok[:2] + (7999, 48000, 16)),
                       ("input rate above", ok[:2] + (384001, 48000, 16)), ("output rate below", ok[:2] + (48000, 7999, 16)),
                       ("output rate above", ok[:2] + (48000, 384001, 16)), ("short", (ok[0], 4457, 48000, 48000, 16)),
                       ("negative overlap", ok[:4] + (-1,)), ("overlap above T/2", ok[:4] + (33,))):
        assert L.srtHostRatePieces(*args, None, 0) == 0 and b"srtHostRatePieces" in L.srtLastError(), name
    assert L.srtHostRatePieces(ok[0], 4458, 48000, 48000, 16, None, 0) == 1             # ceil(4458 * 0.91875) = 4096
    for n, fi, fo in ((300000, 7999, 48000), (300000, 48000, 384001), (4457, 48000, 48000), (0, 44100, 44100)):
        assert L.srtHostRateLength(n, fi, fo) == 0 and b"srtHostRateLength" in L.srtLastError()
        with pytest.raises(capi.EngineError):
            capi.host_rate_length(n, fi, fo)
        with pytest.raises(ValueError):
            stream.host_rate_pieces(n, fi, fo, 64, 0, 1)
    # a table shorter than the plan is filled up to its length and the count is still the whole plan's
    buf = (capi._HostRatePiece * 2)()
    assert L.srtHostRatePieces(*ok, C.cast(buf, C.c_void_p), 2) == 3
    assert [(b.s0, b.fin0) for b in buf] == [(0, 0), (2 * 48 * 1024, 2 * 48 * 1024)]
    # the entry point itself: a null engine needs no device
    x = np.zeros(300000, np.float32)
    out = np.zeros(16, np.float32)
    assert L.srtSeparateHostStreamRate(None, C.c_void_p(x.ctypes.data), C.c_void_p(x.ctypes.data), 300000, 48000, 48000, 0, C.c_void_p(out.ctypes.data), 0, None) == -1
    assert b"srtSeparateHostStreamRate" in L.srtLastError()


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _n_at(rate):
    return N_RAGGED * rate // 44100


@pytest.fixture(scope="module")
def pcm(oracle):
    """the test signal at each input rate: the same generator, its own length (about 6.4 s); read-only"""
    cache = {}

    def get(rate):
        if rate not in cache:
            L, R = oracle.synth_audio(_n_at(rate), SEED, True)
            L.setflags(write=False)
            R.setflags(write=False)
            cache[rate] = (L, R)
        return cache[rate]
    return get


def _small(coeffs, max_tiles, **kw):
    return _engine(coeffs, S=3, F=512, max_tiles=max_tiles, batch_invariant=True, **kw)


def _composition(eng, LR, fs_in, fs_out, O, y44_out=None):
    """the definition, from the calls that exist without this feature: convert to 44.1 kHz, separate on the same engine, convert every pair"""
    import spleeterrt_amd as srt
    x44 = LR
    if fs_in != 44100:
        r = srt.Resampler(fs_in, 44100)
        x44 = r.resample_host(*LR)
        r.close()
    y44 = (eng.separate_host_overlap(x44, O) if O else eng.separate_host_stream_io(x44))[0]
    if y44_out is not None:
        y44_out.append(y44)
    if fs_out == 44100:
        return y44
    r = srt.Resampler(44100, fs_out)
    out = np.stack([np.stack(r.resample_host(y44[p, 0], y44[p, 1])) for p in range(y44.shape[0])])
    r.close()
    return out


def _nan_out(eng, n, fs_in, fs_out):
    return np.full((eng.outputs, 2, eng.host_rate_length(n, fs_in, fs_out)), np.nan, np.float32)


def _same(got, ref, tag):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert not np.isnan(got).any(), "%s: %d samples not written" % (tag, int(np.isnan(got).sum()))
    bad = np.argwhere(got != ref)
    assert bad.size == 0, "%s: %d samples differ, first at %s (max-abs %.3g)" % (tag, len(bad), bad[0], float(np.abs(got - ref).max()))


CASES = [(fi, fo, mt) for fi, fo in ((48000, 48000), (48000, 44100), (44100, 48000), (32000, 32000)) for mt in (1, 3)] + [(96000, 44100, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("O", [0, 16])
@pytest.mark.parametrize("fs_in,fs_out,max_tiles", CASES)
def test_equals_the_composition(coeffs, pcm, fs_in, fs_out, max_tiles, O):
    """max_tiles = 1: five pieces (six at O = 16), every seam through the rate carry; 3: two pieces"""
    from spleeterrt_amd import capi
    LR = pcm(fs_in)
    eng = _small(coeffs, max_tiles)
    ref = _composition(eng, LR, fs_in, fs_out, O)
    eng.set_timing(True)
    out, clipped = eng.separate_host_rate(LR, fs_in, fs_out, overlap=O, out=_nan_out(eng, LR[0].size, fs_in, fs_out))
    kn = eng.get_timing_kernels()
    eng.set_timing(False)
    eng.close()
    npieces = len(capi.host_rate_pieces(LR[0].size, fs_in, fs_out, T_S, O, max_tiles))
    assert npieces == {(1, 0): 5, (1, 16): 6, (3, 0): 2, (3, 16): 2}[(max_tiles, O)]
    for name, on in (("rate_in", fs_in != 44100), ("rate_out", fs_out != 44100)):
        ks = [k for nm, k in kn if nm == name]
        assert len(ks) == (npieces if on else 0) and all(k.startswith("srt_resample_spans_kernel<false, %d>" % (1 if name == "rate_in" else 3)) for k in ks), (name, ks)
    assert clipped.tolist() == [0, 0, 0]
    _same(out, ref, "%d -> %d max_tiles=%d O=%d" % (fs_in, fs_out, max_tiles, O))


MIX1 = [[0.5, -1.0, 0.25, 0.125]]          # one output over three stems and the input


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["ratio", "average", "mix"])
def test_options_come_from_the_engine(coeffs, pcm, option):
    LR = pcm(48000)
    eng = _small(coeffs, 1, ratio_mask=option == "ratio")
    if option == "average":
        eng.set_mask_extension("average")
    if option == "mix":
        eng.set_mix(MIX1)
    ref = _composition(eng, LR, 48000, 48000, 16)
    out, _ = eng.separate_host_rate(LR, 48000, overlap=16, out=_nan_out(eng, LR[0].size, 48000, 48000))
    eng.close()
    assert out.shape[0] == (1 if option == "mix" else 3)
    _same(out, ref, option)


@pytest.mark.gpu
def test_pcm16_in_and_out(coeffs, pcm):
    LR = pcm(48000)
    n = LR[0].size
    eng = _small(coeffs, 3)
    x = np.stack(LR, 1)
    unpack = lambda q: (np.ascontiguousarray(q[:, 0].astype(np.float32) / np.float32(32768)), np.ascontiguousarray(q[:, 1].astype(np.float32) / np.float32(32768)))
    first = _composition(eng, unpack(rule(x)[0]), 48000, 48000, 16)
    g = np.float32(1.0 / np.sort(np.abs(first).reshape(-1))[-3000])        # about three thousand samples of the float output pass full scale
    q = rule(x * g)[0]
    ref = _composition(eng, unpack(q), 48000, 48000, 16)
    # 16-bit in, floats out
    out, c0 = eng.separate_host_rate(q, 48000, overlap=16, out=_nan_out(eng, n, 48000, 48000))
    assert c0.tolist() == [0, 0, 0]
    _same(out, ref, "16-bit in")
    # 16-bit in and out: the rule on the composition, and its clipped counts
    rq, rc = rule(ref)
    want, wclip = np.ascontiguousarray(rq.transpose(0, 2, 1)), [int(rc[s].sum()) for s in range(3)]
    buf = np.full(want.shape, 0x5A5A, np.int16)
    out16, clipped = eng.separate_host_rate(q, 48000, overlap=16, out_pcm16=True, out=buf)
    # floats in, 16-bit out
    out16f, clippedf = eng.separate_host_rate(unpack(q), 48000, overlap=16, out_pcm16=True)
    eng.close()
    print("clipped per stem:", clipped.tolist(), "expected", wclip)
    bad = np.argwhere(out16 != want)
    assert bad.size == 0, "first mismatch (stem, sample, channel) %s of %d" % (bad[0], len(bad))
    assert clipped.tolist() == wclip and sum(wclip) > 0
    assert np.array_equal(out16f, want) and clippedf.tolist() == wclip


@pytest.mark.gpu
@pytest.mark.parametrize("O", [0, 16])
def test_both_rates_44100_is_the_overlap_call(coeffs, pcm, O):
    LR = pcm(44100)
    eng = _small(coeffs, 3)
    eng.set_timing(True)
    ref, _ = eng.separate_host_overlap(LR, O)
    kref = eng.get_timing_kernels()
    eng.set_timing(False)
    eng.set_timing(True)
    out, _ = eng.separate_host_rate(LR, 44100, overlap=O, out=_nan_out(eng, LR[0].size, 44100, 44100))
    kout = eng.get_timing_kernels()
    eng.set_timing(False)
    eng.close()
    assert len(kref) > 20 and kout == kref
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


@pytest.mark.gpu
def test_one_piece(coeffs, pcm):
    from spleeterrt_amd import capi
    LR = pcm(48000)
    eng = _small(coeffs, 12)
    assert len(capi.host_rate_pieces(LR[0].size, 48000, 32000, T_S, 16, 12)) == 1
    ref = _composition(eng, LR, 48000, 32000, 16)
    out, _ = eng.separate_host_rate(LR, 48000, 32000, overlap=16, out=_nan_out(eng, LR[0].size, 48000, 32000))
    eng.close()
    _same(out, ref, "one piece")


@pytest.mark.gpu
def test_the_comparison_can_fail(coeffs, pcm):
    """What a lost carry gives: every piece converts its own finalised samples with nothing before them (the 2 LO + 1 carried samples read as zeros).  That differs
    from the composition at every seam, and only in frames whose window reaches a carried sample: within 2 LO + 2 samples of a seam."""
    import torch
    import spleeterrt_amd as srt
    from spleeterrt_amd import capi, stream
    LR = pcm(44100)
    eng = _small(coeffs, 1)
    keep = []
    ref = _composition(eng, LR, 44100, 48000, 0, y44_out=keep)
    eng.close()
    y44 = keep[0]
    plan = capi.host_rate_pieces(LR[0].size, 44100, 48000, T_S, 0, 1)
    g = stream.rs_geometry(44100, 48000)
    K = 2 * g["LO"] + 1
    r = srt.Resampler(44100, 48000)
    lost = np.empty_like(ref[0])
    for p in plan:
        y = torch.from_numpy(y44[0].copy()).cuda()
        y[:, max(p["fin0"] - K, 0):p["fin0"]] = 0
        a, b = r.resample(y[0], y[1], out0=p["out0"], n_out=p["out1"] - p["out0"])
        lost[0, p["out0"]:p["out1"]], lost[1, p["out0"]:p["out1"]] = a.cpu().numpy(), b.cpu().numpy()
    r.close()
    differs = np.nonzero((lost != ref[0]).any(axis=0))[0]
    pos = differs * g["P"] // g["Q"]                           # the 44.1 kHz sample each differing frame sits on
    seams = np.array([p["fin0"] for p in plan[1:]])
    assert len(seams) == 4
    dist = np.abs(pos[:, None] - seams[None, :])
    assert (dist.min(axis=1) <= K + 1).all(), int((dist.min(axis=1) > K + 1).sum())
    assert sorted(set(dist.argmin(axis=1).tolist())) == [0, 1, 2, 3]           # every seam shows
    print("lost carry: %d frames differ around %d seams" % (len(differs), len(seams)))


@pytest.mark.gpu
def test_refusals(coeffs, pcm):
    import spleeterrt_amd as srt
    Lh, Rh = pcm(48000)
    n = Lh.size
    eng = _small(coeffs, 3)
    out = _nan_out(eng, n, 48000, 48000)
    q = np.zeros((n, 2), np.int16)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda h, a, b, n_, fi, fo, ov, o, fl: eng.L.srtSeparateHostStreamRate(h, a, b, n_, fi, fo, ov, o, fl, None)
    cases = [("null input", (eng.h, None, vp(Rh), n, 48000, 48000, 16, vp(out), 0), ""),
             ("null second channel", (eng.h, vp(Lh), None, n, 48000, 48000, 16, vp(out), 0), ""),
             ("null output", (eng.h, vp(Lh), vp(Rh), n, 48000, 48000, 16, None, 0), ""),
             ("unknown flag bits", (eng.h, vp(Lh), vp(Rh), n, 48000, 48000, 16, vp(out), 8), "flag"),
             ("16-bit input with a second buffer", (eng.h, vp(q), vp(Rh), n, 48000, 48000, 16, vp(out), srt.HOST_IN_PCM16), "h_in2"),
             ("input rate", (eng.h, vp(Lh), vp(Rh), n, 7999, 48000, 16, vp(out), 0), "8000..384000"),
             ("output rate", (eng.h, vp(Lh), vp(Rh), n, 48000, 384001, 16, vp(out), 0), "8000..384000"),
             ("short", (eng.h, vp(Lh), vp(Rh), 4457, 48000, 48000, 16, vp(out), 0), "4096"),
             ("negative overlap", (eng.h, vp(Lh), vp(Rh), n, 48000, 48000, -1, vp(out), 0), "overlap_rows"),
             ("overlap above T/2", (eng.h, vp(Lh), vp(Rh), n, 48000, 48000, T_S // 2 + 1, vp(out), 0), "overlap_rows")]
    for name, args, word in cases:
        assert call(*args) == -1, name
        text = eng.L.srtLastError().decode()
        assert "srtSeparateHostStreamRate" in text and word in text, (name, text)
    eng.set_wiener(1)
    assert call(eng.h, vp(Lh), vp(Rh), n, 48000, 48000, 16, vp(out), 0) == -1
    text = eng.L.srtLastError().decode()
    assert "srtSeparateHostStreamRate" in text and "Wiener" in text, text
    eng.set_wiener(0)
    bare = srt.Engine(F=512, T=T_S, stem_modes=(1, 0, 1), variant=srt.VARIANT_VST, max_tiles=3, batch_invariant=True)
    assert bare.L.srtSeparateHostStreamRate(bare.h, vp(Lh), vp(Rh), n, 48000, 48000, 16, vp(out), 0, None) == -5
    assert "srtSeparateHostStreamRate" in bare.L.srtLastError().decode()
    bare.close()
    assert np.isnan(out).all()                                  # nothing was written by any of them
    for bad in (-1, T_S // 2 + 1, 1.5, "x", None):
        with pytest.raises(srt.EngineError, match="separate_host_rate"):
            eng.separate_host_rate((Lh, Rh), 48000, overlap=bad)
    # a rate pair whose window does not fit the LDS: with the built-in filter no pair of 8000..384000 Hz reaches the limit, for one pair per workgroup
    # (the form the launch falls back to) - the refusal guards a longer table; the arithmetic that shows it
    from spleeterrt_amd import stream
    for fi, fo in ((384000, 44100), (44100, 8000), (8000, 44100), (44100, 384000)):
        g = stream.rs_geometry(fi, fo)
        assert (63 * g["P"] // g["Q"] + 1 + g["T4"]) * 8 <= 64 << 10
    # the engine's own overlap is neither read nor changed; the call works, and again after the staging (the carries with it) has been released
    eng.set_overlap(8)
    a, _ = eng.separate_host_rate((Lh, Rh), 48000, overlap=16, out=out)
    eng.set_overlap(0)
    assert not np.isnan(a).any()
    eng.release_staging()
    b, _ = eng.separate_host_rate((Lh, Rh), 48000, overlap=16, out=_nan_out(eng, n, 48000, 48000))
    eng.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
