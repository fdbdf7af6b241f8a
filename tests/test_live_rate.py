"""The converter as a stream (srtResamplerStream*, spleeterrt_amd.ResamplerStream) and the live mode at the host's sample rate
(srtLiveCreateRate, Spleeter4StemsInitRate, spleeterrt_amd.Live(sample_rate=...)).

Yardsticks: the offline converter (Resampler.resample, itself pinned to libsamplerate in test_resample.py) for the stream's bits; the composition
offline converter -> 44.1 kHz live stream -> offline converter for the rate instance's bits; the float64 restatements of test_resample.py and
test_live.py for its accuracy; an integer model of "what has arrived when" for its latency."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import test_live as TL
import test_resample as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
HOP = 1024
TABLE_LEN, INDEX_INC = 22438, 491                     # the built-in filter's layout (the reference table's)
RATES = (44100, 48000, 96000, 88200, 32000, 22050)


@pytest.fixture(scope="module")
def lib():
    from spleeterrt_amd import build as b
    b.build(verbose=False)
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


# ---------------------------------------------------------------- restatements
def horizon(fs_in, fs_out):
    """H: the last right-half tap that can carry weight, LO + 1 with LO = ((table_len - 2) << 12) // increment (srt_resample.hip's geometry)"""
    inc = int(np.rint(INDEX_INC * min(fs_out / float(fs_in), 1.0) * 4096))
    return (((TABLE_LEN - 2) << 12) // inc) + 1


def computable(fs_in, fs_out, H, n_in):
    """number of j >= 0 with floor(j * fs_in / fs_out) + H <= n_in - 1, counted one by one"""
    j = 0
    while (j * fs_in) // fs_out + H <= n_in - 1:
        j += 1
    return j


def model_latency(fs, K, Lk):
    """The least A of the issue's model, by bisection over a literal evaluation of the model (the condition is monotone in A): after N host samples
    c44(N) 44.1 kHz frames exist and hops(N) = c44(N) // 1024 hops are complete; output sample m, produced by the call that delivers input sample m, may
    read the 44.1 kHz stem stream up to floor((m - A) * 44100 / fs) + Dl + H2 and needs that to be at most 1024 * hops(m + 1) - 1."""
    D = Lk + 2 * K
    Dl = (D + 1) * HOP
    g = math.gcd(fs, 44100)
    P1, Q1 = fs // g, 44100 // g
    H1, H2 = (0, 0) if fs == 44100 else (horizon(fs, 44100), horizon(44100, fs))
    hops = D + 3 + max(40, Q1)                        # past the start-up and over a whole period of the hop / sample phase
    nmax = (hops * HOP * P1) // Q1 + H1 + 2
    N = np.arange(nmax + 1, dtype=np.int64)
    c44 = np.where(N > H1, -((-(N - H1) * Q1) // P1), 0)          # = computable(fs, 44100, H1, N), checked in test_emitted_counts
    rhs = HOP * (c44[1:] // HOP) - 1                               # index m: 1024 * hops(m + 1) - 1
    m = np.arange(nmax, dtype=np.int64)

    def causal(A):
        return bool(np.all(((m - A) * Q1) // P1 + Dl + H2 <= rhs))   # a negative left side never binds: the right side is >= -1
    lo, hi = -1, nmax
    assert causal(hi) and not causal(0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if causal(mid) else (mid, hi)
    assert causal(hi) and not causal(hi - 1)
    return hi


def builtin_table():
    """srt_resample.hip's built-in half filter: Kaiser-windowed sinc, beta 12, cutoff 0.918, 22 438 points at 491 per sample"""
    k = np.arange(TABLE_LEN, dtype=np.float64)
    t = k / INDEX_INC
    q = t / ((TABLE_LEN - 1) / float(INDEX_INC))
    c = 0.918 * np.sinc(0.918 * t) * np.i0(12.0 * np.sqrt(np.clip(1.0 - q * q, 0.0, None))) / np.i0(12.0)
    return c.astype(np.float32)


# ---------------------------------------------------------------- CPU
def test_create_calls_check_arguments_before_any_hip_call(lib):
    import torch
    from spleeterrt_amd import capi
    h = C.c_void_p()
    tab = np.ones(100, np.float32)
    for args, msg in (((4000, 44100, 2, 1024, None, 0, 0), b"8000..384000"), ((44100, 400000, 2, 1024, None, 0, 0), b"8000..384000"),
                      ((48000, 44100, 0, 1024, None, 0, 0), b"channels"), ((48000, 44100, 17, 1024, None, 0, 0), b"channels"),
                      ((48000, 44100, 2, 0, None, 0, 0), b"max_block"), ((48000, 44100, 2, -5, None, 0, 0), b"max_block"),
                      ((48000, 44100, 2, 1024, tab.ctypes.data, 1, 491), b"table_len"), ((48000, 44100, 2, 1024, tab.ctypes.data, 100, 0), b"index_inc")):
        assert lib.srtResamplerStreamCreate(*args, None, C.byref(h)) == -1, args
        assert msg in lib.srtLastError() and b"srtResamplerStreamCreate" in lib.srtLastError(), (args, lib.srtLastError())
    assert lib.srtResamplerStreamCreate(48000, 44100, 2, 1024, None, 0, 0, None, None) == -1 and b"null" in lib.srtLastError()
    assert lib.srtResamplerStreamProcess(None, None, 0, 1, None, 0) == -1 and b"null" in lib.srtLastError()
    assert lib.srtResamplerStreamFlush(None, None, 0) == -1 and lib.srtResamplerStreamReset(None) == -1 and lib.srtResamplerStreamHorizon(None) == -1
    assert lib.srtResamplerStreamDestroy(None) == 0
    assert lib.srtResampleHorizon(4000, 44100, 0, 0) == -1 and lib.srtResampleHorizon(48000, 44100, 1, 491) == -1

    blob = np.zeros(capi.COEFF_FLOATS, np.float32)

    def create(F=512, T=64, S=2, K=4, Lk=0, fs=48000, max_block=1024, max_tiles=1, blobs=None):
        cfg = capi._Config()
        cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles, cfg.variant = F, T, S, max_tiles, capi.VARIANT_VST
        for i in range(S if 0 < S <= capi.MAX_STEMS else 0):
            cfg.stem_mode[i], cfg.oob_weight[i] = 1, 0.25
        blobs = [blob.ctypes.data] * max(S, 1) if blobs is None else blobs
        hh = C.c_void_p()
        rc = lib.srtLiveCreateRate(C.byref(cfg), K, Lk, fs, max_block, (C.c_void_p * len(blobs))(*blobs), C.byref(hh))
        return rc, lib.srtLastError().decode(), hh
    for kw, text in (({"fs": 7999}, "8000..384000"), ({"fs": 384001}, "8000..384000"), ({"fs": 0}, "8000..384000"), ({"max_block": 0}, "max_block"),
                     ({"max_block": -1}, "max_block"), ({"K": 0}, "hops_per_run"), ({"K": 65}, "hops_per_run"), ({"K": 4, "Lk": 61}, "lookahead"),
                     ({"K": 4, "Lk": -1}, "lookahead"), ({"max_tiles": 2}, "max_tiles"), ({"blobs": [blob.ctypes.data, None]}, "null coefficient"),
                     ({"F": 500}, "multiples of 64"), ({"S": 0}, "n_stems"), ({"S": 9}, "n_stems")):
        rc, msg, hh = create(**kw)
        assert rc == -1 and text in msg and "srtLiveCreateRate" in msg and not hh.value, (kw, rc, msg)
    assert lib.srtLiveCreateRate(None, 4, 0, 48000, 1024, None, None) == -1 and "null argument" in lib.srtLastError().decode()
    assert lib.srtLiveRateLatency(4000, 1, 0) == -1 and lib.srtLiveRateLatency(48000, 0, 0) == -1 and lib.srtLiveRateLatency(48000, 1, -1) == -1
    if not torch.cuda.is_available():                                         # valid arguments get as far as the device check
        assert lib.srtResamplerStreamCreate(48000, 44100, 2, 1024, None, 0, 0, None, C.byref(h)) == -3 and b"no HIP device" in lib.srtLastError()
        rc, msg, hh = create()
        assert rc == -3 and "no HIP device" in msg


def test_latency_is_the_least_causal_delay(lib):
    """srtLiveRateLatency against the brute-force minimum of the model, and the figures the issue records for the built-in table's layout"""
    from spleeterrt_amd import capi
    assert horizon(48000, 44100) == 50 and horizon(44100, 48000) == 46
    assert lib.srtResampleHorizon(48000, 44100, 0, 0) == 50 and lib.srtResampleHorizon(44100, 48000, TABLE_LEN, INDEX_INC) == 46
    recorded = {48000: (4557, 20161, 23504), 96000: (9114, 40322, 47009), 88200: (8374, 37046, 43190), 32000: (3063, 13465, 15694),
                22050: (2139, 9307, 10843)}
    for fs in RATES:
        for i, (K, Lk) in enumerate(((1, 0), (4, 8), (7, 5))):
            A = model_latency(fs, K, Lk)
            assert lib.srtLiveRateLatency(fs, K, Lk) == capi.live_rate_latency(fs, K, Lk) == A, (fs, K, Lk, A)
            D = Lk + 2 * K
            if fs == 44100:
                assert A == (D + 2) * HOP - 1 == TL.live_schedule(K, Lk)[1] + HOP - 1
            else:
                assert A == recorded[fs][i]
                assert abs(A - (horizon(fs, 44100) + ((D + 2) * HOP + horizon(44100, fs)) * fs / 44100.0)) <= 3
    for K, Lk in ((1, 0), (4, 8)):                                            # 44100 / gcd = 4, even: the general form of the closed expression
        assert model_latency(33075, K, Lk) == lib.srtLiveRateLatency(33075, K, Lk)


def test_emitted_counts_sum_to_the_offline_length(lib):
    """what a call emits is host arithmetic: srtResampleComputable equals the one-by-one count of the frames whose last tap has arrived, at fixed n
    and at every cut of random partitions; what the flush adds to reach srtResampleLength is between 0 and the frames H input frames span"""
    rng = np.random.default_rng(3)
    for fs_in, fs_out in ((48000, 44100), (44100, 48000), (96000, 44100), (44100, 96000), (32000, 44100), (22050, 44100), (44056, 44100), (8000, 384000)):
        H = lib.srtResampleHorizon(fs_in, fs_out, 0, 0)
        assert H == horizon(fs_in, fs_out)
        for n in (0, 1, H - 1, H, H + 1, H + 2, 777, 4096):
            assert lib.srtResampleComputable(fs_in, fs_out, H, n) == computable(fs_in, fs_out, H, n), (fs_in, fs_out, n)
        for _ in range(20):
            total = int(rng.integers(1, 20000))
            have = j = 0                                                      # j: the one-by-one count, carried along (it only grows with the input)
            while have < total:
                n = min(int(rng.choice((1, 17, 300, 724, 1024, 4096))), total - have)
                have += n
                before = j
                while (j * fs_in) // fs_out + H <= have - 1:
                    j += 1
                assert lib.srtResampleComputable(fs_in, fs_out, H, have) == j, (fs_in, fs_out, have)
                assert j - before <= n * fs_out // fs_in + 1                  # what one call emits (the bound a caller may size its output with)
            length = lib.srtResampleLength(total, fs_in, fs_out)
            assert length == int(math.ceil(total * (fs_out / float(fs_in))))
            assert 0 <= length - j <= -((-min(H, total) * fs_out) // fs_in) + 1, (fs_in, fs_out, total, length, j)     # the flush


# ---------------------------------------------------------------- GPU: the converter
@pytest.mark.gpu
@pytest.mark.parametrize("fs_in,fs_out", [(48000, 44100), (96000, 44100), (44100, 48000), (44100, 96000), (32000, 44100), (22050, 44100), (44056, 44100),
                                          (44101, 44100)])
def test_stream_converter_is_the_offline_converter_bit_for_bit(fs_in, fs_out):
    """any partition of the input into blocks, 2 planar and 8 interleaved channels: concatenated output == Resampler.resample of the whole clip.
    Both forms of the kernel run for every pair: the one the filter selects (the weight bank; at 44101 -> 44100 the bank would take 16 MB, so that
    pair takes the on-the-fly form by itself, while 44056 -> 44100 still fits the bank) and the on-the-fly form forced with SPLEETERRT_RESAMPLE_ONFLY=1
    around the constructor, as test_resample.py does for the offline converter."""
    import torch
    import spleeterrt_amd as srt
    rng = np.random.default_rng(fs_in + 7 * fs_out)
    off = srt.Resampler(fs_in, fs_out)
    bank_bytes = (fs_out // math.gcd(fs_in, fs_out)) * ((2 * horizon(fs_in, fs_out) + 3) // 4 * 4) * 4      # Q phases x T4 taps (taps = 2 LO + 2 = 2 H)
    assert (bank_bytes > (8 << 20)) == (fs_in == 44101), bank_bytes
    for chunks, n in (((1024,), 9001), ((1,), 500), ((17, 300, 724, 1024, 4096), 15000)):
        x = torch.from_numpy((0.5 * rng.standard_normal((8, n))).astype(np.float32)).cuda()
        ref = torch.stack([t for p in range(4) for t in off.resample(x[2 * p].contiguous(), x[2 * p + 1].contiguous())])
        assert ref.shape[1] == off.length(n) and float(ref.abs().max()) > 0
        for channels, interleaved, onfly in ((2, False, False), (8, True, False), (2, False, True), (8, True, True)):
            if onfly:
                os.environ["SPLEETERRT_RESAMPLE_ONFLY"] = "1"
            try:
                rs = srt.ResamplerStream(fs_in, fs_out, channels=channels, max_block=4096)
            finally:
                os.environ.pop("SPLEETERRT_RESAMPLE_ONFLY", None)
            assert rs.horizon == horizon(fs_in, fs_out)
            pieces, pos, i = [], 0, 0
            while pos < n:
                c = min(chunks[i % len(chunks)], n - pos)
                i += 1
                blk = x[:channels, pos:pos + c]
                pieces.append(rs.process(blk.t().contiguous() if interleaved else blk.contiguous(), interleaved))
                pos += c
            assert sum(p.shape[1] for p in pieces) == rs.computable(n)
            pieces.append(rs.flush())
            got = torch.cat(pieces, 1)
            assert got.shape == (channels, off.length(n))
            assert torch.equal(got, ref[:channels]), (fs_in, fs_out, chunks, channels, onfly)
            if chunks == (1024,):                                             # a reset starts the same stream again
                rs.reset()
                again = torch.cat([rs.process(x[:channels, :777].t().contiguous() if interleaved else x[:channels, :777].contiguous(), interleaved), rs.flush()], 1)
                a, b = off.resample(x[0, :777].contiguous(), x[1, :777].contiguous())
                assert torch.equal(again[0], a) and torch.equal(again[1], b)
            rs.close()
    off.close()


# ---------------------------------------------------------------- GPU: the live mode at a rate
VST, F32 = 1, 0


def _live(F, T, modes, oob, variant, precision, K, Lk, cs, **kw):
    import spleeterrt_amd
    return spleeterrt_amd.Live(F, T, modes, oob, variant, precision, K, Lk, cs, **kw)


def _composition(oracle, cs, fs, T, F, K, Lk, modes=(1, 1, 1, 1), oob=TL.PLUGIN_OOB, variant=VST, precision=F32, ratio=False, seed=11, extra_hops=12,
                 chunks=(1024,)):
    """(got, expected, A, lo, hi): the rate instance's timeline and offline converter -> 44.1 kHz live stream (1024-sample calls) -> offline converter
    placed at A, comparable bit for bit on [lo, hi); before A - ceil((1024 + H2 + 1) fs / 44100) both are zero"""
    import spleeterrt_amd as srt
    D = Lk + 2 * K
    Dl = (D + 1) * HOP
    n = int((D + 2 + extra_hops) * HOP * fs / 44100.0)
    L, R = oracle.synth_audio(n, seed, True)
    down, up = srt.Resampler(fs, 44100), srt.Resampler(44100, fs)
    x44 = down.resample_host(L, R)
    live = _live(F, T, modes, oob, variant, precision, K, Lk, cs, ratio_mask=ratio)
    _, y44 = live.process(x44[0], x44[1])
    live.close()
    rate = _live(F, T, modes, oob, variant, precision, K, Lk, cs, ratio_mask=ratio, sample_rate=fs)
    A = rate.latency
    written, got = rate.process(L, R, chunks)
    rate.close()
    assert written.shape == got.shape == (2 * len(modes), n)                  # n out for n in, every call
    expected = np.zeros_like(got)
    for s in range(len(modes)):
        e = up.resample_host(np.ascontiguousarray(y44[2 * s, Dl:]), np.ascontiguousarray(y44[2 * s + 1, Dl:]))
        for c in range(2):
            k = min(n - A, e[c].size)
            expected[2 * s + c, A:A + k] = e[c][:k]
    down.close()
    up.close()
    H2 = horizon(44100, fs)
    w = int(math.ceil((H2 + 1) * fs / 44100.0))
    margin = int(math.ceil(HOP * fs / 44100.0)) + w
    return got, expected, A, A + w, n - margin


@pytest.fixture(scope="module")
def cs4(coeffs):
    return [np.ascontiguousarray(coeffs(k)) for k in range(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(1024,), (17, 300, 724, 1024), (480,), (1,)])
def test_rate_44100_is_the_live_stream_one_hop_later(oracle, cs4, chunks):
    """no converter runs at 44.1 kHz: the timeline is the 44.1 kHz instance's 1024-call timeline shifted by 1023 samples, for every chunking"""
    T, F, K, Lk = 64, 512, 4, 4
    n = (Lk + 2 * K + 14) * HOP
    L, R = oracle.synth_audio(n, 4410, True)
    plain = _live(F, T, (1, 1, 1, 1), TL.PLUGIN_OOB, VST, F32, K, Lk, cs4)
    _, ref = plain.process(L, R)
    lat = plain.latency
    plain.close()
    rate = _live(F, T, (1, 1, 1, 1), TL.PLUGIN_OOB, VST, F32, K, Lk, cs4, sample_rate=44100, max_block=1000)
    assert rate.latency == lat + HOP - 1 == (Lk + 2 * K + 2) * HOP - 1
    w, tl = rate.process(L, R, chunks)
    rate.close()
    assert w.shape == tl.shape == ref.shape and np.abs(ref).max() > 1e-3
    assert np.all(tl[:, :HOP - 1] == 0) and np.array_equal(tl[:, HOP - 1:], ref[:, :n - (HOP - 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("fs,T,F,K,Lk", [(48000, 64, 512, 1, 0), (48000, 64, 512, 4, 8), (96000, 64, 512, 1, 0), (96000, 64, 512, 4, 8),
                                         (32000, 64, 512, 1, 0), (32000, 64, 512, 4, 8), (48000, 256, 1536, 4, 8),
                                         (44101, 64, 512, 1, 0)])               # 44101 Hz: both converters of the instance take the on-the-fly form
def test_rate_instance_is_the_composition_bit_for_bit(oracle, cs4, fs, T, F, K, Lk):
    got, exp, A, lo, hi = _composition(oracle, cs4, fs, T, F, K, Lk)
    assert hi - lo > 4 * HOP and np.abs(exp[:, lo:hi]).max() > 1e-3
    assert np.array_equal(got[:, lo:hi], exp[:, lo:hi]), (fs, K, Lk, float(np.abs(got[:, lo:hi] - exp[:, lo:hi]).max()))
    zero_to = A - int(math.ceil((HOP + horizon(44100, fs) + 1) * fs / 44100.0))
    assert zero_to > 0 and np.all(got[:, :zero_to] == 0)


@pytest.mark.gpu
def test_rate_instance_against_the_float64_restatement(oracle, cs4):
    """restate (float64 converter) -> restate_segments (float64 live hop, masks from a separate engine) -> restate, at 48 kHz, K = 4, L = 4:
    test_live.py's bound for the live stream, 1e-4 rel-RMS and max-abs over peak.  Measured on MI355X: see DESIGN.md §12."""
    import spleeterrt_amd
    fs, T, F, K, Lk = 48000, 64, 512, 4, 4
    D = Lk + 2 * K
    Dl = (D + 1) * HOP
    hops = D + 14
    n = int(hops * HOP * fs / 44100.0)
    L, R = oracle.synth_audio(n, 2024, True)
    rate = _live(F, T, (1, 1, 1, 1), TL.PLUGIN_OOB, VST, F32, K, Lk, cs4, sample_rate=fs)
    A = rate.latency
    _, got = rate.process(L, R, (512,))
    rate.close()
    table = builtin_table()
    x44 = TR.restate(np.stack([L, R], 1).astype(np.float32), fs, 44100, table)
    n44 = (x44.shape[0] // HOP) * HOP
    masks = TL._Masks(F, T, (1, 1, 1, 1), TL.PLUGIN_OOB, VST, F32, cs4)
    segs, _ = TL.restate_segments(x44[:, 0].astype(np.float64), x44[:, 1].astype(np.float64), n44 // HOP, F, T, K, Lk, TL.PLUGIN_OOB, masks)
    y44 = segs.transpose(1, 0, 2).reshape(8, -1)                              # hop h's segment at [1024 h, 1024 h + 1024)
    H2 = horizon(44100, fs)
    w = int(math.ceil((H2 + 1) * fs / 44100.0))
    lo, hi = A + w, n - int(math.ceil(HOP * fs / 44100.0)) - w                # as the composition test: past the offline converter's zero fill, short of the last hop
    worst_rms = worst_peak = 0.0
    for s in range(4):
        e = TR.restate(np.ascontiguousarray(y44[2 * s:2 * s + 2, Dl:].T).astype(np.float32), 44100, fs, table).astype(np.float64)
        assert e.shape[0] >= hi - A
        for c in range(2):
            ref, g = e[lo - A:hi - A, c], got[2 * s + c, lo:hi].astype(np.float64)
            worst_rms = max(worst_rms, TL.rel_rms(g, ref))
            worst_peak = max(worst_peak, float(np.abs(g - ref).max() / np.abs(ref).max()))
    print("48 kHz rate instance vs float64 restatement: rel-RMS %.3g max-abs/peak %.3g over [%d, %d)" % (worst_rms, worst_peak, lo, hi))
    assert hi - lo > 8 * HOP
    assert worst_rms <= 1e-4 and worst_peak <= 1e-4, (worst_rms, worst_peak)


@pytest.mark.gpu
def test_rate_chunking_independence(oracle, cs4):
    """n out for n in and one constant delay: the whole timeline, from sample 0, is the same bits for every call size (slices above max_block too)"""
    T, F, K, Lk, fs = 64, 512, 4, 4, 48000
    n = int((Lk + 2 * K + 12) * HOP * fs / 44100.0)
    L, R = oracle.synth_audio(n, 1234, True)
    outs = []
    for chunks, mb in (((1024,), 4096), ((512,), 4096), ((480,), 4096), ((17, 300, 724, 1024), 4096), ((4096,), 4096), ((1,), 4096), ((4096,), 1000), ((n,), 480)):
        rate = _live(F, T, (1, 1, 1, 1), TL.PLUGIN_OOB, VST, F32, K, Lk, cs4, sample_rate=fs, max_block=mb)
        w, tl = rate.process(L, R, chunks)
        rate.close()
        assert w.shape == tl.shape == (8, n), (chunks, w.shape)
        outs.append(tl)
    assert np.abs(outs[0]).max() > 1e-3
    for tl in outs[1:]:
        assert np.array_equal(tl, outs[0])


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [48000, 96000, 88200, 32000])
def test_rate_latency_measured(fs):
    """all-zero weights (VST masks exactly 0.5) and oob 0.5, input band-limited below 0.8 of the lower Nyquist frequency: the lag of the
    cross-correlation peak is `latency` exactly; at 48 kHz 2 x output equals the delayed input to the converter pair's round-trip figure, 1e-4"""
    from spleeterrt_amd import capi
    T, F, K, Lk = 64, 512, 1, 0
    zero = np.zeros(capi.COEFF_FLOATS, np.float32)
    rate = _live(F, T, (1, 0), (0.5, 0.5), VST, F32, K, Lk, [zero, zero], sample_rate=fs)
    A = rate.latency
    assert A == capi.live_rate_latency(fs, K, Lk)
    n = A + int(16 * HOP * fs / 44100.0)
    rng = np.random.default_rng(fs)
    t = np.arange(n) / float(fs)
    top = 0.8 * min(fs, 44100) / 2.0
    x = np.zeros((2, n))
    for f, p0, p1 in zip(rng.uniform(40.0, top, 48), rng.uniform(0, 6.28, 48), rng.uniform(0, 6.28, 48)):
        x[0] += 0.015 * np.sin(2 * np.pi * f * t + p0)
        x[1] += 0.015 * np.sin(2 * np.pi * f * t + p1)
    x = x.astype(np.float32)
    _, got = rate.process(x[0], x[1], (512,))
    rate.close()
    nf = 1 << int(math.ceil(math.log2(2 * n)))
    for j in range(4):
        src = x[j % 2].astype(np.float64)
        corr = np.fft.irfft(np.fft.rfft(got[j].astype(np.float64), nf) * np.conj(np.fft.rfft(src, nf)), nf)[:n]
        assert int(np.argmax(corr)) == A, (fs, j, int(np.argmax(corr)), A)
        err = TL.rel_rms(2.0 * got[j, A + 600:n - 600].astype(np.float64), src[600:n - A - 600])
        print("fs %d plane %d: lag %d = latency, 2 x out vs delayed input rel-RMS %.3g" % (fs, j, A, err))
        if fs == 48000:
            assert err <= 1e-4, (j, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name,modes,oob,variant,precision,ratio", [
    ("2stem", (0, 1), (0.1, 0.3), 1, 0, False),
    ("5stem", (1, 0, 1, 0, 1), (0.0, 0.1, 0.2, 0.3, 0.4), 1, 0, False),
    ("exe", (1, 1, 1, 1), TL.PLUGIN_OOB, 0, 0, False),
    ("ratio", (1, 0, 1, 1), TL.PLUGIN_OOB, 1, 0, True),
    ("f16", (1, 1, 1, 1), TL.PLUGIN_OOB, 1, 1, False)])
def test_rate_other_configs(oracle, coeffs, name, modes, oob, variant, precision, ratio):
    """the composition of test_rate_instance_is_the_composition_bit_for_bit in the other configurations; fp16: test_live_other_configs' bounds, for
    the reason given there (the fp16 networks' bits vary between engine instances of one process)"""
    import spleeterrt_amd
    cs = [np.ascontiguousarray(coeffs(k)) for k in range(len(modes))]
    got, exp, A, lo, hi = _composition(oracle, cs, 48000, 64, 512, 4, 4, modes, oob, variant, precision, ratio, seed=7, chunks=(512,))
    assert got.shape[0] == 2 * len(modes) and np.abs(exp[:, lo:hi]).max() > 1e-3
    g, e = got[:, lo:hi], exp[:, lo:hi]
    if precision == spleeterrt_amd.PREC_F16:
        errs = [TL.rel_rms(g[j], e[j]) for j in range(g.shape[0])]
        peak = float(np.abs(g - e).max() / np.abs(e).max())
        print("%s rel-rms %.3g max/peak %.3g" % (name, max(errs), peak))
        assert max(errs) <= 5e-2 and peak <= 5e-1, (errs, peak)
    else:
        assert np.array_equal(g, e), (name, float(np.abs(g - e).max()))


@pytest.mark.gpu
def test_plugin_surface_at_a_rate(oracle, cs4):
    """Spleeter4StemsInitRate: inSampleCount samples per plane and call, Spleeter4StemsLatency = A, the bits of srtLiveCreateRate in the plugin's config"""
    import spleeterrt_amd
    lib = spleeterrt_amd.load_library()
    T, F, K, Lk, fs = 64, 512, 4, 4, 48000
    n = int((Lk + 2 * K + 8) * HOP * fs / 44100.0)
    L, R = oracle.synth_audio(n, 99, True)
    rate = _live(F, T, (1, 1, 1, 1), TL.PLUGIN_OOB, VST, F32, K, Lk, cs4, sample_rate=fs, max_block=512)
    _, ref = rate.process(L, R, (512,))
    A = rate.latency
    rate.close()
    msr = C.create_string_buffer(4096)
    prov = (C.c_void_p * 4)(*[c.ctypes.data for c in cs4])
    lib.Spleeter4StemsInitRate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.Spleeter4StemsProcessSamples.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.Spleeter4StemsLatency.argtypes = [C.c_void_p]
    lib.Spleeter4StemsFree.argtypes = [C.c_void_p]
    lib.Spleeter4StemsInitRate(msr, F, T, prov, K, Lk, fs, 512)
    assert lib.Spleeter4StemsLatency(msr) == A
    out = np.full((8, n), np.nan, np.float32)
    pos = 0
    while pos < n:
        c = min(441, n - pos)
        lib.Spleeter4StemsProcessSamples(msr, L.ctypes.data + 4 * pos, R.ctypes.data + 4 * pos, c, (C.c_void_p * 8)(*[out[j].ctypes.data + 4 * pos for j in range(8)]))
        pos += c
    lib.Spleeter4StemsFree(msr)
    assert np.array_equal(out, ref)


@pytest.mark.gpu
def test_rate_call_latency(tmp_path, coeffs):
    """host/live_latency at 48 kHz, T = 256, F = 1536, 512-sample calls paced at the block period (10.7 ms): test_live_call_latency's bounds for paced
    runs (p99 < 2 ms, worst call < one hop period; eight instances: worst < 5 ms) and, in addition, worst call < the block period itself"""
    subprocess.check_call(["make", "-s", "-C", HOST, "live_latency"])
    F, T, fs, call = 1536, 256, 48000, 512
    hop_us, block_us = HOP / 44100 * 1e6, call / float(fs) * 1e6
    w = tmp_path / "w4.f32"
    with open(w, "wb") as f:
        for k in range(4):
            np.ascontiguousarray(coeffs(k), np.float32).tofile(f)
    record = {}
    for tag, K, Lk, ni in (("k1_paced", 1, 0, 2), ("k4_paced", 4, 8, 2), ("k4_eight_paced", 4, 8, 8)):
        from spleeterrt_amd import capi
        A = capi.live_rate_latency(fs, K, Lk)
        calls = (A + int(48 * HOP * fs / 44100.0)) // call
        out = tmp_path / (tag + ".json")
        subprocess.check_call([os.path.join(HOST, "live_latency"), str(F), str(T), str(K), str(Lk), str(calls), str(w), str(int(round(block_us))), str(out),
                               str(ni), str(fs), str(call)], timeout=300)
        r = json.load(open(out))
        record[tag] = r
        assert r["sample_rate"] == fs and r["call_size"] == call
        for i, inst in enumerate(r["instances"]):
            assert inst["init_error"] == "", "%s instance %d came up muted: %s" % (tag, i, inst["init_error"])
            c = inst["calls"]
            assert c["n"] == calls and c["p50_us"] > 20.0
            assert inst["latency_samples"] == A
            assert inst["output_peak"] > 1e-4
            if ni == 2:
                assert c["p99_us"] < 2000.0 and c["max_us"] < hop_us and c["max_us"] < block_us, "%s instance %d: %r" % (tag, i, c)
            else:
                assert c["max_us"] < 5000.0 and c["p99_us"] < 2000.0 and c["max_us"] < block_us, "%s instance %d: %r" % (tag, i, c)
    print("rate live latency:", json.dumps(record))
