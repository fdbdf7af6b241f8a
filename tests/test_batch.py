"""srtSeparateBatch: many independent tracks in one packed batch (one batched STFT, one srtForward over the packed tiles, one batched
inverse transform).

CPU: srtBatchPlan against stream.pack_tracks.  GPU: every track's stems equal srtSeparate on that track alone (bit for bit under
batch_invariant, at F = 512 and F = 1536 - both inverse-kernel families - with and without ratio_mask; within the split-K association in the
default mode), the CPU oracle end to end, the fp16 mode at the bench shape, one launch per transform, full coverage of every output,
refusals, and the Python grouping over several calls."""
import ctypes as C

import numpy as np
import pytest

T_S, F_S = 64, 512
# one exact tile multiple (64 rows), the 4096-sample minimum, ragged tails; 1 + 1 + 2 + 1 + 3 = 8 tiles at T = 64
TRACKS = (64 * 1024, 4096, 4096 * 24 + 8192 + 333, 50000, 140077)


def _lib():
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


def _plan(L, ns, T):
    k = len(ns)
    t0 = (C.c_size_t * max(k, 1))()
    tot = C.c_size_t(0)
    rc = L.srtBatchPlan((C.c_size_t * max(k, 1))(*ns), k, T, t0, C.byref(tot))
    return rc, list(t0[:k]), tot.value


def test_batch_plan_matches_pack_tracks():
    from spleeterrt_amd import stream
    L = _lib()
    rng = np.random.default_rng(7)
    for T in (64, 128, 256):
        for trial in range(20):
            k = int(rng.integers(1, 12))
            ns = [int(x) for x in rng.integers(4096, 40 * T * 1024, size=k)]
            ns[0] = 4096                                            # the minimum
            if k > 1:
                ns[1] = int(rng.integers(1, 4)) * T * 1024          # an exact tile multiple: rows = whole tiles, no tail
            if k > 2:
                ns[2] = int(rng.integers(1, 4)) * T * 1024 + 1      # one sample into the next row
            rc, t0, tot = _plan(L, ns, T)
            assert rc == 0, L.srtLastError()
            g = stream.pack_tracks(ns, T, 1 << 30)
            assert len(g) == 1 and g[0].tracks == list(range(k))
            assert g[0].tile0 == t0 and g[0].ntiles == tot
            want = [(stream.stft_rows(n) + T - 1) // T for n in ns]
            assert tot == sum(want) and t0 == [sum(want[:i]) for i in range(k)]
            assert want[0] == 1 and (k < 2 or want[1] * T == stream.stft_rows(ns[1]))
    # tile0 may be NULL
    tot = C.c_size_t(0)
    assert L.srtBatchPlan((C.c_size_t * 2)(4096, 70000), 2, 64, None, C.byref(tot)) == 0 and tot.value == 3
    # refusals: ntracks < 1, T < 1, a track below 4096 samples, missing arrays
    assert _plan(L, [], 64)[0] == -1
    assert _plan(L, [5000], 0)[0] == -1
    assert _plan(L, [5000, 4095], 64)[0] == -1 and b"4096" in L.srtLastError()
    assert L.srtBatchPlan(None, 1, 64, None, C.byref(tot)) == -1
    assert L.srtBatchPlan((C.c_size_t * 1)(5000), 1, 64, None, None) == -1


def test_pack_tracks_groups_in_order():
    from spleeterrt_amd import stream
    T = 64
    ns = [n for n in TRACKS] * 3                                    # 3 x 8 tiles
    g = stream.pack_tracks(ns, T, 8)
    assert [x.tracks for x in g] == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11, 12, 13, 14]]
    assert all(x.tile0 == [0, 1, 2, 4, 5] and x.ntiles == 8 for x in g)
    g = stream.pack_tracks(ns, T, 3)                                # greedy: a track that does not fit starts the next call
    assert [x.tracks for x in g][:4] == [[0, 1], [2, 3], [4], [5, 6]]
    for x in g:
        assert x.ntiles <= 3
    assert sorted(sum((x.tracks for x in g), [])) == list(range(len(ns)))
    with pytest.raises(ValueError, match="max_tiles"):
        stream.pack_tracks([4096, 140077], T, 2)
    with pytest.raises(ValueError, match="4096"):
        stream.pack_tracks([4095], T, 2)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _engine(coeffs, S=2, **kw):
    import spleeterrt_amd as srt
    modes = (1, 0, 1, 0, 1, 0, 1, 0)[:S]
    kw.setdefault("variant", srt.VARIANT_VST)
    eng = srt.Engine(stem_modes=modes, **kw)
    for s in range(S):
        eng.set_coeff(s, coeffs(s))
    return eng


def _tracks(oracle, ns, seed=100):
    import torch
    out = []
    for k, n in enumerate(ns):
        L, R = oracle.synth_audio(n, seed + k, True)
        out.append((torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()))
    return out


def _rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
@pytest.mark.parametrize("ratio", [False, True])
def test_batch_bit_identical_to_single_tracks(oracle, coeffs, F, ratio):
    """batch_invariant, fp32: every track's stems from ONE srtSeparateBatch call are bit for bit srtSeparate of that track alone."""
    import torch
    eng = _engine(coeffs, F=F, T=T_S, max_tiles=8, batch_invariant=True, ratio_mask=ratio)
    tr = _tracks(oracle, TRACKS)
    eng.set_timing(True)
    got = eng.separate_batch(tr)
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    istft = [k for n, k in ks if n == "istft_batch"]
    assert len(istft) == 1 and istft[0].startswith("srt_istft_batch_kernel<%s, %s, false>" % ("true" if F <= 1024 else "false", "true" if ratio else "false")), istft
    for k, (L, R) in enumerate(tr):
        ref = eng.separate(L, R)
        assert got[k].shape == ref.shape
        assert torch.equal(got[k], ref), (k, float((got[k] - ref).abs().max()))
    eng.close()


@pytest.fixture(scope="module")
def default_batch(oracle, coeffs):
    """the default mode (split-K association free to differ with the batch), 2 stems at T = 64, F = 512: the batch and each track alone"""
    eng = _engine(coeffs, F=F_S, T=T_S, max_tiles=8)
    tr = _tracks(oracle, TRACKS, seed=300)
    got = [o.cpu().numpy() for o in eng.separate_batch(tr)]
    single = [eng.separate(L, R).cpu().numpy() for L, R in tr]
    host = [(L.cpu().numpy(), R.cpu().numpy()) for L, R in tr]
    eng.close()
    return host, got, single


@pytest.mark.gpu
def test_batch_default_mode_matches_single_tracks(default_batch):
    _, got, single = default_batch
    for k in range(len(TRACKS)):
        assert got[k].shape == single[k].shape
        peak = float(np.abs(single[k]).max())
        assert float(np.abs(got[k] - single[k]).max()) <= 1e-5 * peak, k


@pytest.mark.gpu
def test_batch_against_oracle(oracle, coeffs, default_batch):
    """three tracks of a batch against the oracle's stft -> processMT -> istft of each track (main.c:776-785)"""
    host, got, _ = default_batch
    modes = (1, 0)
    for k in (1, 2, 4):                                            # the 4096-sample track and two ragged ones
        L, R = host[k]
        re, im = oracle.stft(L, R)
        for s in range(2):
            r, i = re.copy(), im.copy()
            oracle.process_spectrogram(coeffs(s), r, i, F_S, T_S, modes[s], oracle.VARIANT_VST, 0.1)
            ref = oracle.istft(r, i)
            assert got[k][s].shape == ref.shape
            peak = float(np.abs(ref).max())
            assert _rel_rms(got[k][s], ref) <= 1e-4, (k, s, _rel_rms(got[k][s], ref))
            assert float(np.abs(got[k][s] - ref).max()) <= 1e-4 * peak, (k, s)


@pytest.mark.gpu
def test_batch_fp16_bench_shape(oracle, coeffs):
    """the fp16 mode at the bench shape (T = 256, F = 1024, 4 stems) with tracks totalling 64 tiles: the half-mask inverse form runs, and two sampled
    tracks are within the fp16 tolerance class (stems rel-RMS <= 1e-2) of the fp32 oracle"""
    import spleeterrt_amd as srt
    T, F, S = 256, 1024, 4
    tiles = [1, 1, 3, 5, 2, 8, 4, 6, 7, 3, 2, 9, 5, 8]            # 64
    assert sum(tiles) == 64
    ns = [((t - 1) * T + 1 + (37 * k) % (T - 1)) * 1024 - 300 for k, t in enumerate(tiles)]
    ns[0] = 4096
    eng = _engine(coeffs, S=S, F=F, T=T, max_tiles=64, precision=srt.PREC_F16)
    tr = _tracks(oracle, ns, seed=500)
    eng.set_timing(True)
    got = eng.separate_batch(tr)
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    istft = [k for n, k in ks if n == "istft_batch"]
    assert istft == ["srt_istft_batch_kernel<true, false, true>"], istft
    modes = (1, 0, 1, 0)
    for k, stems in ((0, (0, 3)), (1, (1, 2))):                     # every stem once, on two one-tile tracks
        L, R = tr[k][0].cpu().numpy(), tr[k][1].cpu().numpy()
        re, im = oracle.stft(L, R)
        out = got[k].cpu().numpy()
        assert np.isfinite(out).all()
        for s in stems:
            r, i = re.copy(), im.copy()
            oracle.process_spectrogram(coeffs(s), r, i, F, T, modes[s], oracle.VARIANT_VST, 0.1)
            ref = oracle.istft(r, i)
            assert _rel_rms(out[s], ref) <= 1e-2, (k, s, _rel_rms(out[s], ref))
    eng.close()


@pytest.mark.gpu
def test_batch_one_launch_per_transform(oracle, coeffs):
    """K = 16 tracks: exactly one stft_batch and one istft_batch launch; the network launches are the list srtForward issues for the packed tile count"""
    import torch
    from spleeterrt_amd import stream
    ns = [4096 + 9000 * k for k in range(16)]
    eng = _engine(coeffs, F=F_S, T=T_S, max_tiles=32)
    g = stream.pack_tracks(ns, T_S, 32)
    assert len(g) == 1
    tr = _tracks(oracle, ns, seed=700)
    eng.separate_batch(tr)                                           # (first call allocates the table; not part of the count)
    eng.set_timing(True)
    eng.separate_batch(tr)
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    names = [n for n, _ in ks]
    assert names.count("stft_batch") == 1 and names.count("istft_batch") == 1, names
    assert names[0] == "stft_batch" and names[-1] == "istft_batch"
    assert ks[0][1] == "srt_stft_batch_kernel"
    net = ks[1:-1]
    mag = torch.zeros((g[0].ntiles, 2, T_S, F_S), device="cuda")
    eng.forward(mag)
    eng.set_timing(True)
    eng.forward(mag)
    ref = eng.get_timing_kernels()
    eng.set_timing(False)
    assert net == ref
    eng.close()


@pytest.mark.gpu
def test_batch_writes_every_sample_and_nothing_past(oracle, coeffs):
    """outputs pre-filled with NaN hold none afterwards; oversized buffers keep everything past S x 2 x len_k"""
    import torch
    eng = _engine(coeffs, F=F_S, T=T_S, max_tiles=8)
    tr = _tracks(oracle, TRACKS, seed=900)
    L = eng.L
    need = [2 * 2 * L.srtIstftLength(L.srtStftRows(n)) for n in TRACKS]
    outs = [torch.full((m + 5000,), float("nan"), device="cuda") for m in need]
    for o, m in zip(outs, need):
        o[m:] = 12345.0
    eng.separate_batch(tr, outs)
    for k, (o, m) in enumerate(zip(outs, need)):
        h = o.cpu().numpy()
        assert np.isfinite(h[:m]).all(), (k, int(np.isnan(h[:m]).sum()))
        assert (h[m:] == 12345.0).all(), k
    eng.close()


@pytest.mark.gpu
def test_batch_refusals(oracle, coeffs):
    """too many tiles, the Wiener filter, null entries and short tracks: -1 with srtLastError text, nothing written; a valid call afterwards succeeds"""
    import torch
    eng = _engine(coeffs, F=F_S, T=T_S, max_tiles=4)
    L = eng.L
    tr = _tracks(oracle, TRACKS[:3], seed=1100)                    # 1 + 1 + 2 = 4 tiles
    ns = [int(a.numel()) for a, _ in tr]
    outs = [torch.full((2, 2, L.srtIstftLength(L.srtStftRows(n))), float("nan"), device="cuda") for n in ns]
    P = C.c_void_p * 3

    def call(ns_, Lp=None, Rp=None, Op=None, k=3):
        Lp = Lp or [a.data_ptr() for a, _ in tr]
        Rp = Rp or [b.data_ptr() for _, b in tr]
        Op = Op or [o.data_ptr() for o in outs]
        return L.srtSeparateBatch(eng.h, k, P(*Lp), P(*Rp), (C.c_size_t * 3)(*ns_), P(*Op))
    # too many tiles: a 3-tile third track (real buffers of its length, so even a launch would stay inside them)
    (Ll, Rl), = _tracks(oracle, [140077], seed=1200)
    ol = torch.full((2, 2, L.srtIstftLength(L.srtStftRows(140077))), float("nan"), device="cuda")
    assert call([ns[0], ns[1], 140077], Lp=[tr[0][0].data_ptr(), tr[1][0].data_ptr(), Ll.data_ptr()], Rp=[tr[0][1].data_ptr(), tr[1][1].data_ptr(), Rl.data_ptr()],
                Op=[outs[0].data_ptr(), outs[1].data_ptr(), ol.data_ptr()]) == -1 and b"max_tiles" in L.srtLastError()
    assert call(ns, Lp=[tr[0][0].data_ptr(), None, tr[2][0].data_ptr()]) == -1 and b"null" in L.srtLastError()
    assert call(ns, Op=[outs[0].data_ptr(), outs[1].data_ptr(), None]) == -1 and b"null" in L.srtLastError()
    assert call([ns[0], 4095, ns[2]]) == -1 and b"4096" in L.srtLastError()
    assert call(ns, k=0) == -1 and L.srtLastError()
    eng.set_wiener(1)
    assert call(ns) == -1 and b"Wiener" in L.srtLastError()
    eng.set_wiener(0)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs + [ol])
    assert call(ns) == 0, L.srtLastError()
    for o in outs:
        assert torch.isfinite(o).all()
    eng.close()


@pytest.mark.gpu
def test_separate_batch_splits_into_calls(oracle, coeffs):
    """more tracks than fit max_tiles: several srtSeparateBatch calls, each track equal to separate() on it (batch_invariant: bit for bit)"""
    import torch
    from spleeterrt_amd import stream
    ns = list(TRACKS) + [4096 * 9 + 11, 64 * 1024 * 2]               # 8 + 1 + 2 = 11 tiles
    eng = _engine(coeffs, F=F_S, T=T_S, max_tiles=4, batch_invariant=True)
    groups = stream.pack_tracks(ns, T_S, 4)
    assert len(groups) >= 3
    tr = _tracks(oracle, ns, seed=1300)
    eng.set_timing(True)
    got = eng.separate_batch(tr)
    names = [n for n, _ in eng.get_timing()]
    eng.set_timing(False)
    assert names.count("stft_batch") == len(groups) and names.count("istft_batch") == len(groups)
    for k, (L, R) in enumerate(tr):
        assert torch.equal(got[k], eng.separate(L, R)), k
    eng.close()
