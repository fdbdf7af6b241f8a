"""Live separation with a sliding network window (srtLive*, Spleeter4StemsInitLive, spleeterrt_amd.Live).

The yardstick is a float64 numpy restatement of the live hop: the reference's asymmetric analysis / synthesis windows
(Spleeter4Stems.c:383-416), the analysis FFT with the conjugate convention and magnitude x4096, mask and out-of-band weight,
the inverse with the reference's bin packing, the 50 % overlap-add, the (K, L, D) schedule and the reference's sample accounting.
Masks come from a function the caller passes in.  At K = T, L = 0 it is pinned against the real reference streaming engine
(oracle/_ref/libspleeter_ref_stream.so); the GPU tests hold srtLive to it for sliding windows."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
FFT, HOP = 4096, 1024
PLUGIN_OOB = (0.25, 0.0, 0.25, 0.25)                  # Spleeter4Stems.c:444-447


# ---------------------------------------------------------------- float64 restatement
def asymmetric_window():
    """srt_stream.hip asymmetric_window (Spleeter4Stems.c:383-416, k = 4096, m = 1024) in float64: (analysis incl. its 0.5/4096, pre-shifted synthesis)"""
    k, m = FFT, HOP
    an, sy = np.zeros(k), np.zeros(k)
    n = ((k - m) << 1) + 2
    i = np.arange(k - m)
    an[:k - m] = 0.5 * (1.0 - np.cos(2.0 * np.pi * (i + 1.0) / n))
    n = (m << 1) + 2
    i = np.arange(k - m, k)
    an[k - m:] = np.sqrt(0.5 * (1.0 - np.cos(2.0 * np.pi * ((m + i - (k - m)) + 1.0) / n)))
    n = m << 1
    i = np.arange(k - 2 * m, k)
    sy[k - 2 * m:] = 0.5 * (1.0 - np.cos(2.0 * np.pi * (i - (k - 2 * m)) / n)) / an[k - 2 * m:]
    sy[:k - 2048] = sy[2048:].copy()                  # pre-shift by SAMPLESHIFT
    return an * (1.0 / FFT) * 0.5, sy


def live_schedule(K, L):
    """D (hops between a frame's analysis and its synthesis) and the latency in samples for 1024-sample calls"""
    D = L + 2 * K
    return D, D * HOP + HOP


def mask_run(g, K, L):
    """the run (its last hop h_r = K-1 mod K) whose window holds frame g at a row in [T-L-K, T-L-1]: h_r - g in [L, L+K-1]"""
    lo = g + L
    return lo + (K - 1 - lo) % K


def restate_segments(L_in, R_in, hops, F, T, K, Lk, oob, masks_fn):
    """per-hop output segments [hops][2S][1024] of the live stream.  masks_fn(h_r, window [2][T][F] float32) -> masks [S][2][T][F]"""
    an, sy = asymmetric_window()
    S = len(oob)
    D, _ = live_schedule(K, Lk)
    x = np.zeros((2, hops * HOP + FFT))
    nin = min(L_in.size, hops * HOP)
    x[0, FFT - HOP:FFT - HOP + nin] = L_in[:nin]
    x[1, FFT - HOP:FFT - HOP + nin] = R_in[:nin]
    spec = np.empty((hops, 2, 2049), complex)
    for g in range(hops):                             # frame g = the 4096 samples ending with hop g's block
        fr = x[:, g * HOP:g * HOP + FFT] * an
        spec[g] = 2.0 * np.conj(np.fft.fft(fr, axis=1)[:, :2049])
    mag = (np.abs(spec[:, :, :F]) * 4096.0).astype(np.float32)
    runs = {}

    def masks_of(hr):
        if hr not in runs:
            win = np.zeros((2, T, F), np.float32)
            for i in range(T):
                gg = hr - T + 1 + i
                if gg >= 0:
                    win[:, i] = mag[gg]
            runs[hr] = np.asarray(masks_fn(hr, win), np.float64)
        return runs[hr]
    segs = np.zeros((hops, 2 * S, HOP))
    ov = np.zeros((S, 2, HOP))
    for h in range(D, hops):
        g = h - D
        hr = mask_run(g, K, Lk)
        p = T - 1 - (hr - g)
        m = masks_of(hr)[:, :, p]                     # [S][2][F]
        for s in range(S):
            gain = np.full((2, 2049), float(oob[s]))
            gain[:, :F] = m[s]
            A = spec[g] * gain                        # [2 ch][2049]
            AL, AR = A[0], A[1]
            z = np.zeros(FFT, complex)
            z[0] = AR[0].real + 1j * AL[0].real
            z[2048] = (AR[2048].real - AR[2048].imag) + 1j * (AL[2048].real - AL[2048].imag)
            k = np.arange(1, 2048)
            z[k] = AR[k] + 1j * AL[k]
            z[FFT - k] = np.conj(AR[k]) + 1j * np.conj(AL[k])
            y = np.fft.fft(z)
            yL, yR = y.imag, y.real
            segs[h, 2 * s] = ov[s, 0] + yL[2048:3072] * sy[:1024]
            segs[h, 2 * s + 1] = ov[s, 1] + yR[2048:3072] * sy[:1024]
            ov[s, 0] = yL[3072:] * sy[1024:2048]
            ov[s, 1] = yR[3072:] * sy[1024:2048]
    return segs, runs


def account(segs, n, chunks):
    """The reference's sample accounting (Spleeter4Stems.c:512-582): (written [2S][m], timeline [2S][n], position of the first written sample)"""
    nc = segs.shape[1]
    timeline = np.zeros((nc, n))
    q, off, needed, hop, pos, i = [], 0, HOP, 0, 0, 0
    pieces, first = [], None
    while pos < n:
        c = min(chunks[i % len(chunks)], n - pos)
        i += 1
        rem = c
        while rem > 0:
            t = min(needed, rem)
            rem -= t
            needed -= t
            if needed == 0:
                if len(q) >= 2:                       # the queue overrun case: drop the oldest segment
                    q.pop(0)
                    off = 0
                q.append(hop)
                hop += 1
                needed = HOP
        w = 0
        while q and w < c:
            take = min(HOP - off, c - w)
            timeline[:, pos + w:pos + w + take] = segs[q[0]][:, off:off + take]
            w += take
            off += take
            if off == HOP:
                q.pop(0)
                off = 0
        if w:
            first = pos if first is None else first
            pieces.append((pos, w))
        pos += c
    written = np.concatenate([timeline[:, p:p + w] for p, w in pieces], axis=1) if pieces else np.zeros((nc, 0))
    return written, timeline, first


def rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


def _run_plugin(lib, struct_bytes, coeffs, F, T, L, R, chunks, live=None):
    """tests/test_stream.py's _run (timeline form); live=(K, L) drives Spleeter4StemsInitLive instead of Spleeter4StemsInit"""
    msr = C.create_string_buffer(struct_bytes)
    prov = (C.c_void_p * 4)(*[c.ctypes.data for c in coeffs])
    lib.Spleeter4StemsProcessSamples.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.Spleeter4StemsFree.argtypes = [C.c_void_p]
    if live is None:
        lib.Spleeter4StemsInit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        lib.Spleeter4StemsInit(msr, F, T, prov)
    else:
        lib.Spleeter4StemsInitLive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        lib.Spleeter4StemsInitLive(msr, F, T, prov, live[0], live[1])
    lat = None
    if live is not None:
        lib.Spleeter4StemsLatency.argtypes = [C.c_void_p]
        lat = lib.Spleeter4StemsLatency(msr)
    n = L.size
    out = np.zeros((8, n), np.float32)
    pos = i = 0
    while pos < n:
        c = min(chunks[i % len(chunks)], n - pos)
        i += 1
        ptrs = (C.c_void_p * 8)(*[out[j].ctypes.data + 4 * pos for j in range(8)])
        lib.Spleeter4StemsProcessSamples(msr, L.ctypes.data + 4 * pos, R.ctypes.data + 4 * pos, c, ptrs)
        pos += c
    lib.Spleeter4StemsFree(msr)
    return out if live is None else (out, lat)


# ---------------------------------------------------------------- CPU: the restatement itself
def test_restatement_matches_reference_stream(oracle, coeffs):
    """K = T, L = 0 with the oracle's VST network on each window is the reference plugin engine, at test_stream.py's bound"""
    if oracle.ref_path("stream") is None:
        pytest.skip("oracle/_ref/libspleeter_ref_stream.so not built")
    T, F = 64, 512
    hops = 3 * T + 9
    n = hops * HOP
    L, R = oracle.synth_audio(n, 4711, True)
    cs = [np.ascontiguousarray(coeffs(k)) for k in range(4)]
    ref = _run_plugin(C.CDLL(oracle.ref_path("stream")), 1 << 20, cs, F, T, L, R, (1024,))

    def masks(hr, win):
        return np.stack([oracle.forward(cs[s], win, 1, oracle.VARIANT_VST) for s in range(4)])
    segs, _ = restate_segments(L, R, hops, F, T, T, 0, PLUGIN_OOB, masks)
    _, got, first = account(segs, n, (1024,))
    assert first == 0
    D, _ = live_schedule(T, 0)
    assert np.all(got[:, :D * HOP] == 0) and np.all(ref[:, :D * HOP] == 0)
    tr, tg = ref[:, D * HOP:], got[:, D * HOP:]
    assert np.abs(tr).max() > 1e-3
    for j in range(8):
        assert rel_rms(tg[j], tr[j]) <= 1e-4, "component %d rel rms %g" % (j, rel_rms(tg[j], tr[j]))
    assert np.abs(tg - tr).max() <= 1e-4 * np.abs(tr).max()


@pytest.mark.parametrize("K,Lk", [(1, 0), (4, 8), (7, 5), (64, 0)])
def test_restatement_latency_constant_masks(K, Lk):
    """masks of exactly 0.5 and out-of-band weight 0.5: every stem is 0.5 x the input delayed by (L + 2K) * 1024 + 1024 samples"""
    T, F = 64, 512
    D, lat = live_schedule(K, Lk)
    hops = D + 12
    n = hops * HOP
    rng = np.random.default_rng(5)
    L, R = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    segs, _ = restate_segments(L, R, hops, F, T, K, Lk, (0.5, 0.5), lambda hr, w: np.full((2, 2, T, F), 0.5))
    _, tl, _ = account(segs, n, (1024,))
    for s in range(2):
        for c, x in enumerate((L, R)):
            d = np.abs(tl[2 * s + c, lat:] - 0.5 * x[:n - lat]).max()
            assert d <= 1e-9, (K, Lk, s, c, d)
    assert np.all(tl[:, :D * HOP] == 0)


def test_accounting_start_rule():
    """the queue starts emitting at the beginning of the call that completes the first hop, and emits no more than a call received"""
    segs = np.arange(6 * 2 * HOP, dtype=float).reshape(6, 2, HOP) + 1.0
    n = 5 * HOP
    for chunks, start in (((1024,), 0), ((17, 300, 724, 1024), 317), ((1,), 1023), ((700,), 700)):
        w, tl, first = account(segs, n, chunks)
        assert first == start, (chunks, first)
        assert n - start - HOP < w.shape[1] <= n - start                     # a call can emit less than it was given when the queue runs low
        assert np.array_equal(w, segs.transpose(1, 0, 2).reshape(2, -1)[:, :w.shape[1]])


def test_live_argument_checks():
    """every refused case: -1 with a message, before any device call (also on a machine without a GPU)"""
    import spleeterrt_amd
    from spleeterrt_amd import capi
    lib = spleeterrt_amd.load_library()
    blob = np.zeros(capi.COEFF_FLOATS, np.float32)

    def create(F=512, T=64, S=2, K=4, Lk=0, max_tiles=1, blobs=None):
        cfg = capi._Config()
        cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles, cfg.variant = F, T, S, max_tiles, capi.VARIANT_VST
        for i in range(S if 0 < S <= capi.MAX_STEMS else 0):
            cfg.stem_mode[i], cfg.oob_weight[i] = 1, 0.25
        blobs = [blob.ctypes.data] * max(S, 1) if blobs is None else blobs
        h = C.c_void_p()
        rc = lib.srtLiveCreate(C.byref(cfg), K, Lk, (C.c_void_p * len(blobs))(*blobs), C.byref(h))
        return rc, lib.srtLastError().decode(), h
    for kw, text in (({"K": 0}, "hops_per_run"), ({"K": 65}, "hops_per_run"), ({"K": 4, "Lk": 61}, "lookahead"), ({"K": 4, "Lk": -1}, "lookahead"),
                     ({"max_tiles": 2}, "max_tiles"), ({"blobs": [blob.ctypes.data, None]}, "null coefficient"),
                     ({"F": 500}, "multiples of 64"), ({"T": 100}, "multiples of 64"), ({"S": 0}, "n_stems"), ({"S": 9}, "n_stems")):
        rc, msg, h = create(**kw)
        assert rc == -1 and text in msg and "srtLiveCreate" in msg and not h.value, (kw, rc, msg)
    rc = lib.srtLiveCreate(None, 4, 0, None, None)
    assert rc == -1 and "null argument" in lib.srtLastError().decode()
    assert lib.srtLiveLatency(None) == -1
    assert lib.srtLiveProcess(None, None, None, 16, None) == -1
    lib.srtLiveDestroy(None)
    for K, Lk in ((1, 0), (4, 8), (7, 5), (64, 0), (256, 0)):
        assert capi.live_latency(K, Lk) == live_schedule(K, Lk)[1] == (Lk + 2 * K) * 1024 + 1024


# ---------------------------------------------------------------- GPU
def _gpu():
    import torch
    return torch.cuda.is_available()


class _Masks:
    """masks for the restatement from a separate Engine(max_tiles=1) of the same config: the same kernels as the live engine"""

    def __init__(self, F, T, modes, oob, variant, precision, coeffs, ratio=False):
        import spleeterrt_amd
        self.eng = spleeterrt_amd.Engine(F=F, T=T, stem_modes=modes, oob_weights=oob, variant=variant, max_tiles=1, precision=precision)
        for s, c in enumerate(coeffs):
            self.eng.set_coeff(s, c)
        self.ratio = ratio

    def __call__(self, hr, win):
        import torch
        m = self.eng.forward(torch.from_numpy(np.ascontiguousarray(win[None])).cuda())
        if self.ratio:
            self.eng.ratio_mask(m)
        return m[:, 0].cpu().numpy()


def _check(got, ref, D, bound=1e-4, peak_bound=1e-4):
    assert np.all(got[:, :D * HOP] == 0), "the first D hops must be silence"
    assert np.abs(got[:, D * HOP:(D + 1) * HOP]).max() > 1e-4, "hop D must carry signal"
    tg, tr = got[:, D * HOP:], ref[:, D * HOP:]
    errs = [rel_rms(tg[j], tr[j]) for j in range(got.shape[0])]
    peak = float(np.abs(tg - tr).max() / np.abs(tr).max())
    assert max(errs) <= bound and peak <= peak_bound, (errs, peak)
    return max(errs), peak


@pytest.mark.gpu
@pytest.mark.parametrize("T,F,chunks", [(64, 512, (1024,)), (64, 512, (300, 724, 1024, 512, 17)), (256, 1536, (480, 1024, 544))])
def test_live_special_case_is_the_plugin(oracle, coeffs, T, F, chunks):
    """srtLive at K = T, L = 0 in the plugin's config equals Spleeter4Stems bit for bit (test_stream.py's geometries and chunkings)"""
    import spleeterrt_amd
    hops = 3 * T + 9
    n = hops * HOP
    L, R = oracle.synth_audio(n, 4711, True)
    cs = [np.ascontiguousarray(coeffs(k)) for k in range(4)]
    plug = _run_plugin(spleeterrt_amd.load_library(), 4096, cs, F, T, L, R, chunks)
    live = spleeterrt_amd.Live(F, T, (1, 1, 1, 1), PLUGIN_OOB, spleeterrt_amd.VARIANT_VST, spleeterrt_amd.PREC_F32, T, 0, cs)
    assert live.latency == 2 * T * HOP + HOP
    _, tl = live.process(L, R, chunks)
    live.close()
    assert np.abs(plug).max() > 1e-3
    assert np.array_equal(tl, plug)
    plug2, lat = _run_plugin(spleeterrt_amd.load_library(), 4096, cs, F, T, L, R, chunks, live=(T, 0))
    assert lat == 2 * T * HOP + HOP and np.array_equal(plug2, plug)


@pytest.fixture(scope="module")
def small4(coeffs):
    """one mask engine of the 64 x 512 VST 4-stem config, shared by the sliding-window cases"""
    cs = [np.ascontiguousarray(coeffs(k)) for k in range(4)]
    import spleeterrt_amd
    return cs, _Masks(512, 64, (1, 1, 1, 1), PLUGIN_OOB, spleeterrt_amd.VARIANT_VST, spleeterrt_amd.PREC_F32, cs)


@pytest.mark.gpu
@pytest.mark.parametrize("K,Lk", [(1, 0), (1, 8), (4, 4), (7, 5), (16, 16), (32, 0)])
def test_live_sliding_windows(oracle, small4, K, Lk):
    import spleeterrt_amd
    cs, masks = small4
    T, F = 64, 512
    D, lat = live_schedule(K, Lk)
    hops = D + max(3 * K, 24)
    n = hops * HOP
    L, R = oracle.synth_audio(n, 99 + K, True)
    live = spleeterrt_amd.Live(F, T, (1, 1, 1, 1), PLUGIN_OOB, spleeterrt_amd.VARIANT_VST, spleeterrt_amd.PREC_F32, K, Lk, cs)
    assert live.latency == lat
    _, got = live.process(L, R)
    live.close()
    segs, _ = restate_segments(L, R, hops, F, T, K, Lk, PLUGIN_OOB, masks)
    _, ref, _ = account(segs, n, (1024,))
    print("K=%d L=%d rel-rms %.3g max/peak %.3g" % ((K, Lk) + _check(got, ref, D)))


@pytest.mark.gpu
def test_live_shipped_geometry(oracle, coeffs):
    """T = 256, F = 1536 (PluginProcessor.cpp:124), K = 4, L = 8: a few runs past D"""
    import spleeterrt_amd
    T, F, K, Lk = 256, 1536, 4, 8
    D, lat = live_schedule(K, Lk)
    hops = D + 3 * K
    n = hops * HOP
    L, R = oracle.synth_audio(n, 31, True)
    cs = [np.ascontiguousarray(coeffs(k)) for k in range(4)]
    live = spleeterrt_amd.Live(F, T, (1, 1, 1, 1), PLUGIN_OOB, spleeterrt_amd.VARIANT_VST, spleeterrt_amd.PREC_F32, K, Lk, cs)
    _, got = live.process(L, R)
    live.close()
    masks = _Masks(F, T, (1, 1, 1, 1), PLUGIN_OOB, spleeterrt_amd.VARIANT_VST, spleeterrt_amd.PREC_F32, cs)
    segs, _ = restate_segments(L, R, hops, F, T, K, Lk, PLUGIN_OOB, masks)
    _, ref, _ = account(segs, n, (1024,))
    print("shipped geometry rel-rms %.3g max/peak %.3g" % _check(got, ref, D))


@pytest.mark.gpu
@pytest.mark.parametrize("name,modes,oob,variant,precision,ratio", [
    ("2stem", (0, 1), (0.1, 0.3), 1, 0, False),
    ("5stem", (1, 0, 1, 0, 1), (0.0, 0.1, 0.2, 0.3, 0.4), 1, 0, False),
    ("exe", (1, 1, 1, 1), PLUGIN_OOB, 0, 0, False),
    ("ratio", (1, 0, 1, 1), PLUGIN_OOB, 1, 0, True),
    ("f16", (1, 1, 1, 1), PLUGIN_OOB, 1, 1, False)])
def test_live_other_configs(oracle, coeffs, name, modes, oob, variant, precision, ratio):
    import spleeterrt_amd
    T, F, K, Lk = 64, 512, 4, 4
    D, _ = live_schedule(K, Lk)
    hops = D + 16
    n = hops * HOP
    L, R = oracle.synth_audio(n, 7, True)
    cs = [np.ascontiguousarray(coeffs(k)) for k in range(len(modes))]
    live = spleeterrt_amd.Live(F, T, modes, oob, variant, precision, K, Lk, cs, ratio_mask=ratio)
    written, got = live.process(L, R)
    live.close()
    assert got.shape[0] == 2 * len(modes) and written.shape == got.shape     # 1024-sample calls: every call writes its whole block
    masks = _Masks(F, T, modes, oob, variant, precision, cs, ratio)
    segs, _ = restate_segments(L, R, hops, F, T, K, Lk, oob, masks)
    _, ref, _ = account(segs, n, (1024,))
    # fp16: both sides run the same fp16 networks, but the restatement's float64 magnitudes can round to other halves than the stream's float32 ones
    # fp16: measured over nine runs rel-RMS 4.4e-4 .. 1.8e-2 and max-abs 3.1e-4 .. 1.8e-1 of the peak.  The fp16 networks' bits vary between engine
    # instances of one process (an eager engine alone is reproducible), so this case checks the stream's schedule, not fp16 accuracy
    bound, peak_bound = (5e-2, 5e-1) if precision == spleeterrt_amd.PREC_F16 else (1e-4, 1e-4)
    print("%s rel-rms %.3g max/peak %.3g" % ((name,) + _check(got, ref, D, bound, peak_bound)))


@pytest.mark.gpu
@pytest.mark.parametrize("K,Lk", [(1, 0), (4, 8), (7, 5), (64, 0)])
def test_live_latency_measured(K, Lk):
    """all-zero weights (VST: masks exactly sigmoid(0) = 0.5) and oob 0.5: every stem is 0.5 x input, delayed by srtLiveLatency() samples"""
    import spleeterrt_amd
    from spleeterrt_amd import capi
    T, F = 64, 512
    zero = np.zeros(capi.COEFF_FLOATS, np.float32)
    live = spleeterrt_amd.Live(F, T, (1, 0), (0.5, 0.5), spleeterrt_amd.VARIANT_VST, spleeterrt_amd.PREC_F32, K, Lk, [zero, zero])
    lat = live.latency
    D, _ = live_schedule(K, Lk)
    n = (D + 12) * HOP
    rng = np.random.default_rng(K * 100 + Lk)
    L = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    R = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    _, got = live.process(L, R)
    live.close()
    peak = max(np.abs(L).max(), np.abs(R).max()) * 0.5
    for j in range(4):
        x = (L, R)[j % 2]
        d = float(np.abs(got[j, lat:] - 0.5 * x[:n - lat]).max())
        assert d <= 1e-5 * peak, (K, Lk, j, d)
    assert np.all(got[:, :lat - HOP] == 0)
    assert lat == (Lk + 2 * K) * HOP + HOP


@pytest.mark.gpu
def test_live_chunking_independence(oracle, small4):
    import spleeterrt_amd
    cs, _ = small4
    T, F, K, Lk = 64, 512, 4, 4
    D, _ = live_schedule(K, Lk)
    n = (D + 20) * HOP
    L, R = oracle.synth_audio(n, 1234, True)
    outs = {}
    for chunks, start in (((1024,), 0), ((17, 300, 724, 1024), 317), ((1,), 1023)):
        live = spleeterrt_amd.Live(F, T, (1, 1, 1, 1), PLUGIN_OOB, spleeterrt_amd.VARIANT_VST, spleeterrt_amd.PREC_F32, K, Lk, cs)
        w, tl = live.process(L, R, chunks)
        live.close()
        wr, _, first = account(np.ones((n // HOP + 1, 8, HOP)), n, chunks)    # the reference rule: where the stream starts, how much the calls write
        assert first == start and w.shape[1] == wr.shape[1], (chunks, w.shape, wr.shape)
        assert np.all(tl[:, :start] == 0)
        outs[chunks] = w
    ws = list(outs.values())
    assert np.abs(ws[0]).max() > 1e-3
    for w in ws[1:]:
        m = min(w.shape[1], ws[0].shape[1])
        assert np.array_equal(w[:, :m], ws[0][:, :m])


@pytest.mark.gpu
def test_live_call_latency(tmp_path, coeffs):
    """host/live_latency.c: the real-time contract of test_latency.py in the live mode at the shipped geometry.  Two instances on two threads, K = 1 and 4,
    back to back and paced: p99 per call < 2 ms, worst call < the 23.2 ms hop period.  Eight instances paced at K = 4: worst call < 5 ms."""
    subprocess.check_call(["make", "-s", "-C", HOST, "live_latency"])
    F, T = 1536, 256
    hop_us = 1024 / 44100 * 1e6
    w = tmp_path / "w4.f32"
    with open(w, "wb") as f:
        for k in range(4):
            np.ascontiguousarray(coeffs(k), np.float32).tofile(f)
    record = {}
    for tag, K, Lk, pace, ni in (("k1_back_to_back", 1, 0, 0, 2), ("k1_paced", 1, 0, 23220, 2), ("k4_back_to_back", 4, 8, 0, 2),
                                 ("k4_paced", 4, 8, 23220, 2), ("k4_eight_paced", 4, 8, 23220, 8)):
        D, _ = live_schedule(K, Lk)
        hops = D + 48
        out = tmp_path / (tag + ".json")
        subprocess.check_call([os.path.join(HOST, "live_latency"), str(F), str(T), str(K), str(Lk), str(hops), str(w), str(pace), str(out), str(ni)], timeout=300)
        r = json.load(open(out))
        record[tag] = r
        for i, inst in enumerate(r["instances"]):
            assert inst["init_error"] == "", "%s instance %d came up muted: %s" % (tag, i, inst["init_error"])
            c = inst["calls"]
            assert c["n"] == hops and c["p50_us"] > 20.0
            assert inst["latency_samples"] == live_schedule(K, Lk)[1]
            assert inst["output_peak"] > 1e-4
            if ni == 2 and pace:
                assert c["p99_us"] < 2000.0 and c["max_us"] < hop_us, "%s instance %d: %r" % (tag, i, c)
            elif ni == 2:                                      # back to back: at K = 1 every call is a join hop, test_latency.py's join bound (measured 1.9 and 4.3 ms p99)
                assert c["p99_us"] < 5000.0 and c["max_us"] < hop_us, "%s instance %d: %r" % (tag, i, c)
            else:
                assert c["max_us"] < 5000.0 and c["p99_us"] < 2000.0, "%s instance %d: %r" % (tag, i, c)
    print("live latency:", json.dumps(record))
