"""srtSeparateBatchWiener: the multichannel Wiener filter per track of a packed batch (one batched STFT, one srtForward over the packed tiles with fp32
masks, `iterations` x (statistics + finalize) and one filter pass over the packed rows, one batched inverse of the per-stem filtered spectra).

The contract: track k's stems are what srtSeparate gives for track k alone with srtSetWiener(e, iterations) - its statistics window, its a and its row
chunks are the track's own.  Shapes as tests/test_batch.py (T = 64, five tracks over 8 tiles: an exact tile, the one-row minimum, ragged tails, three tiles);
the tracks are scaled to different levels so that an a or a covariance shared across the batch could not pass.  The float64 restatement of the filter and
its bounds are those of tests/test_wiener.py (wiener_np; rel-RMS 1e-4, max 1e-3 of the peak)."""
import ctypes as C

import numpy as np
import pytest

import test_wiener as TW

T_S, F_S = 64, 512
TRACKS = (64 * 1024, 4096, 4096 * 24 + 8192 + 333, 50000, 140077)      # 1 + 1 + 2 + 1 + 3 = 8 tiles at T = 64
LEVELS = (1.0, 0.01, 0.3, 2.0, 0.05)
NEW_KERNELS = ("srt_wiener_stats_batch_kernel", "srt_wiener_finalize_batch_kernel", "srt_wiener_filter_batch_kernel", "srt_istft_batch_spec_kernel")
OLD_KERNELS = ("srt_wiener_stats_kernel", "srt_wiener_finalize_kernel", "srt_wiener_filter_kernel")


def test_null_engine_is_refused():
    import spleeterrt_amd
    L = spleeterrt_amd.load_library()
    assert L.srtSeparateBatchWiener(None, 1, None, None, None, None, 1) == -1
    assert b"srtSeparateBatchWiener" in L.srtLastError()


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _engine(coeffs, S=4, **kw):
    import spleeterrt_amd as srt
    kw.setdefault("variant", srt.VARIANT_VST)
    kw.setdefault("F", F_S)
    kw.setdefault("T", T_S)
    kw.setdefault("max_tiles", 8)
    eng = srt.Engine(stem_modes=(1, 0, 1, 0, 1, 0, 1, 0)[:S], **kw)
    for s in range(S):
        eng.set_coeff(s, coeffs(s))
    return eng


def _tracks(oracle, ns, seed=100, levels=LEVELS):
    import torch
    out = []
    for k, n in enumerate(ns):
        L, R = oracle.synth_audio(n, seed + k, True)
        g = np.float32(levels[k % len(levels)])
        out.append((torch.from_numpy(L * g).cuda(), torch.from_numpy(R * g).cuda()))
    return out


def _covs(eng, S, iters, track=0):
    return [[eng.wiener_cov(j, i, track=track) for i in range(1, iters + 1)] for j in range(S)]


def _same_covs(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] for ra, rb in zip(a, b) for x, y in zip(ra, rb))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
@pytest.mark.parametrize("iters", [1, 2])
def test_bit_identical_to_single_tracks(oracle, coeffs, F, iters):
    """batch_invariant, fp32, 4 stems, both inverse families: every track of ONE call equals srtSeparate of it alone with srtSetWiener(iters), bit for bit,
    and so do its R tables, weight sums and a; the launches are the four batch kernels and none of the single-signal Wiener kernels."""
    import torch
    S = 4
    eng = _engine(coeffs, S, F=F, batch_invariant=True)
    tr = _tracks(oracle, TRACKS)
    eng.set_timing(True)
    got = eng.separate_batch(tr, wiener=iters)                      # (the engine's own setting is off)
    ks = [k for _, k in eng.get_timing_kernels()]
    eng.set_timing(False)
    for kn in NEW_KERNELS:
        assert any(k.startswith(kn) for k in ks), (kn, ks)
    assert not any(k.startswith(OLD_KERNELS) for k in ks), ks
    assert [k for k in ks if k.startswith("srt_istft")] == ["srt_istft_batch_spec_kernel<%s>" % ("true" if F <= 1024 else "false")], ks
    covs = [_covs(eng, S, iters, track=k) for k in range(len(tr))]
    with pytest.raises(Exception, match="wiener_cov"):
        eng.wiener_cov(0, iters + 1, track=0)
    with pytest.raises(Exception, match="wiener_cov"):
        eng.wiener_cov(0, 1, track=len(tr))
    eng.set_wiener(iters)
    for k, (L, R) in enumerate(tr):
        ref = eng.separate(L, R)
        assert got[k].shape == ref.shape
        assert torch.equal(got[k], ref), (k, float((got[k] - ref).abs().max()))
        assert _same_covs(covs[k], _covs(eng, S, iters)), k
    with pytest.raises(Exception, match="wiener_cov"):               # after a single-signal call there is no track 1
        eng.wiener_cov(0, 1, track=1)
    a = [covs[k][0][0][2] for k in range(len(tr))]
    assert len(set(a)) > 1 and min(a) == 1.0 and max(a) > 1.0, a     # the levels do exercise a per track (the quiet tracks sit at the floor of 1)
    eng.close()


@pytest.mark.gpu
def test_position_independent(oracle, coeffs):
    """the same tracks in reversed order in one call: the same bits per track, stems and tables"""
    import torch
    S, iters = 4, 2
    eng = _engine(coeffs, S, batch_invariant=True)
    tr = _tracks(oracle, TRACKS, seed=200)
    K = len(tr)
    fwd = [o.clone() for o in eng.separate_batch(tr, wiener=iters)]
    cf = [_covs(eng, S, iters, track=k) for k in range(K)]
    rev = eng.separate_batch(tr[::-1], wiener=iters)
    cr = [_covs(eng, S, iters, track=k) for k in range(K)]
    for k in range(K):
        assert torch.equal(fwd[k], rev[K - 1 - k]), k
        assert _same_covs(cf[k], cr[K - 1 - k]), k
    eng.close()


def _restated(oracle, spec, masks, T, F, S):
    out, _ = TW.wiener_np(TW._to_complex(spec), masks, T, F, 1, [0.1] * S)
    return TW._istft_of(oracle, out)


@pytest.mark.gpu
def test_against_the_float64_restatement(oracle, coeffs):
    """default mode, 4 stems, one iteration: each track against the engine's own stft + forward of that track alone through wiener_np and oracle.istft, at the
    bounds tests/test_wiener.py holds the single-signal path to"""
    S = 4
    eng = _engine(coeffs, S)
    tr = _tracks(oracle, TRACKS, seed=300)
    got = [o.cpu().numpy() for o in eng.separate_batch(tr, wiener=1)]
    for k, (L, R) in enumerate(tr):
        spec, mag = eng.stft(L, R)
        masks = eng.forward(mag).cpu().numpy()
        ref = _restated(oracle, spec, masks, T_S, F_S, S)
        assert got[k].shape == ref.shape
        TW._compare(got[k], ref, "batch wiener track %d" % k)
    eng.close()


@pytest.mark.gpu
def test_fp16_mode_keeps_float_masks(oracle, coeffs):
    """SRT_PREC_F16, 5 stems: no launch of the call is a half-mask form, and every track is within the same bounds of the restatement fed with the engine's own
    masks of that track - taken from one srtForward over the packed magnitudes (the per-track srtStft outputs back to back), so that the network runs the kernels
    it runs inside the batch call (a track alone is a smaller launch and takes other fp16 kernels, whose masks differ at the fp16 level)."""
    import torch
    import spleeterrt_amd as srt
    S = 5
    eng = _engine(coeffs, S, precision=srt.PREC_F16)
    tr = _tracks(oracle, TRACKS, seed=400)
    eng.set_timing(True)
    got = [o.cpu().numpy() for o in eng.separate_batch(tr, wiener=1)]
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    for name, k in ks:
        assert not k.startswith("srt_istft_batch_kernel") and not k.startswith("srt_istft_ola"), ks      # the only inverse is the per-stem-spectrum form (no M16 form exists)
        if k.startswith("srt_head_rows_kernel"):
            assert not k.rstrip("> ").endswith(", 4, true"), k                                             # the head's half-mask form
    assert [k for _, k in ks if k.startswith("srt_istft")] == ["srt_istft_batch_spec_kernel<true>"], ks
    st = [eng.stft(L, R) for L, R in tr]
    masks = eng.forward(torch.cat([m for _, m in st])).cpu().numpy()
    t0 = 0
    for k, (spec, mag) in enumerate(st):
        nt = mag.shape[0]
        ref = _restated(oracle, spec, masks[:, t0:t0 + nt], T_S, F_S, S)
        t0 += nt
        assert got[k].shape == ref.shape
        TW._compare(got[k], ref, "batch wiener fp16 track %d" % k)
    assert t0 == 8
    eng.close()


@pytest.mark.gpu
def test_one_launch_per_stage(oracle, coeffs):
    """5 tracks, 2 iterations: 1 stft_batch, 2 wiener_stats_batch, 2 wiener_cov_batch, 1 wiener_filter_batch, 1 istft_batch; the network launches are srtForward's over 8 tiles"""
    import torch
    eng = _engine(coeffs, 2)
    tr = _tracks(oracle, TRACKS, seed=500)
    eng.separate_batch(tr, wiener=2)                                  # (first call allocates; not part of the count)
    eng.set_timing(True)
    eng.separate_batch(tr, wiener=2)
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    names = [n for n, _ in ks]
    tail = ["wiener_stats_batch", "wiener_cov_batch", "wiener_stats_batch", "wiener_cov_batch", "wiener_filter_batch", "istft_batch"]
    assert names[0] == "stft_batch" and names[-6:] == tail, names
    for n in set(tail) | {"stft_batch"}:
        assert names.count(n) == ([names[0]] + tail).count(n), (n, names)
    assert not any(n in ("wiener_stats", "wiener_cov", "wiener_filter", "istft", "stft") for n in names), names
    mag = torch.zeros((8, 2, T_S, F_S), device="cuda")
    eng.forward(mag)
    eng.set_timing(True)
    eng.forward(mag)
    ref = eng.get_timing_kernels()
    eng.set_timing(False)
    assert ks[1:-6] == ref
    eng.close()


@pytest.mark.gpu
def test_writes_every_sample_nothing_past_and_repeats(oracle, coeffs):
    """NaN-filled outputs come back finite, guard elements after each d_out[k] stay, and two identical calls give the same bits"""
    import torch
    S = 2
    eng = _engine(coeffs, S)
    tr = _tracks(oracle, TRACKS, seed=600)
    L = eng.L
    need = [S * 2 * L.srtIstftLength(L.srtStftRows(n)) for n in TRACKS]
    runs = []
    for _ in range(2):
        outs = [torch.full((m + 5000,), float("nan"), device="cuda") for m in need]
        for o, m in zip(outs, need):
            o[m:] = 12345.0
        eng.separate_batch(tr, outs, wiener=2)
        runs.append(outs)
    for k, m in enumerate(need):
        h = runs[0][k].cpu().numpy()
        assert np.isfinite(h[:m]).all(), (k, int(np.isnan(h[:m]).sum()))
        assert (h[m:] == 12345.0).all(), k
        assert torch.equal(runs[0][k], runs[1][k]), k
    eng.close()


@pytest.mark.gpu
def test_refusals(oracle, coeffs):
    """everything srtSeparateBatch refuses, iterations outside 1..3, ratio_mask, overlap, the average mask extension, a stream capture: -1 with text and nothing
    written; missing weights: -5; a valid call afterwards succeeds; srtSeparateBatch itself still refuses while srtSetWiener is on"""
    import torch
    import spleeterrt_amd as srt
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                   # (a non-default stream, so that the capture case below can capture it)
        eng = _engine(coeffs, 2, max_tiles=4)
    L = eng.L
    tr = _tracks(oracle, TRACKS[:3], seed=700)                     # 1 + 1 + 2 = 4 tiles
    ns = [int(a.numel()) for a, _ in tr]
    outs = [torch.full((2, 2, L.srtIstftLength(L.srtStftRows(n))), float("nan"), device="cuda") for n in ns]
    torch.cuda.synchronize()
    P = C.c_void_p * 3

    def call(ns_, Lp=None, Rp=None, Op=None, k=3, it=1, e=None, arrays=True):
        Lp = Lp or [a.data_ptr() for a, _ in tr]
        Rp = Rp or [b.data_ptr() for _, b in tr]
        Op = Op or [o.data_ptr() for o in outs]
        return L.srtSeparateBatchWiener((e or eng).h, k, P(*Lp) if arrays else None, P(*Rp), (C.c_size_t * 3)(*ns_), P(*Op), it)
    (Ll, Rl), = _tracks(oracle, [140077], seed=800)
    ol = torch.full((2, 2, L.srtIstftLength(L.srtStftRows(140077))), float("nan"), device="cuda")
    assert call([ns[0], ns[1], 140077], Lp=[tr[0][0].data_ptr(), tr[1][0].data_ptr(), Ll.data_ptr()], Rp=[tr[0][1].data_ptr(), tr[1][1].data_ptr(), Rl.data_ptr()],
                Op=[outs[0].data_ptr(), outs[1].data_ptr(), ol.data_ptr()]) == -1 and b"max_tiles" in L.srtLastError()
    assert call(ns, Lp=[tr[0][0].data_ptr(), None, tr[2][0].data_ptr()]) == -1 and b"null" in L.srtLastError()
    assert call(ns, Op=[outs[0].data_ptr(), outs[1].data_ptr(), None]) == -1 and b"null" in L.srtLastError()
    assert call(ns, arrays=False) == -1 and b"arrays" in L.srtLastError()
    assert call([ns[0], 4095, ns[2]]) == -1 and b"4096" in L.srtLastError()
    assert call(ns, k=0) == -1 and L.srtLastError()
    for it in (0, 4, -1):
        assert call(ns, it=it) == -1 and b"iterations" in L.srtLastError()
    eng.set_overlap(8)
    assert call(ns) == -1 and b"overlap" in L.srtLastError()
    eng.set_overlap(0)
    eng.set_mask_extension("average")
    assert call(ns) == -1 and b"mask extension" in L.srtLastError()
    eng.set_mask_extension("constant")
    er = _engine(coeffs, 2, max_tiles=4, ratio_mask=True)
    assert call(ns, e=er) == -1 and b"ratio_mask" in L.srtLastError()
    er.close()
    bare = srt.Engine(F=F_S, T=T_S, stem_modes=(1, 0), variant=srt.VARIANT_VST, max_tiles=4)
    assert call(ns, e=bare) == -5 and b"weights" in L.srtLastError()
    bare.close()
    torch.cuda.synchronize()
    dummy = torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                      # the engine's stream is capturing: refused before anything is enqueued
        dummy += 1.0                                                # (so that the captured graph is not empty)
        rc = call(ns)
        msg = L.srtLastError()
    assert rc == -1 and b"capture" in msg, (rc, msg)
    del graph
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs + [ol])
    with torch.cuda.stream(side):
        assert call(ns) == 0, L.srtLastError()
        side.synchronize()
    for o in outs:
        assert torch.isfinite(o).all()
    eng.set_wiener(1)
    assert L.srtSeparateBatch(eng.h, 3, P(*[a.data_ptr() for a, _ in tr]), P(*[b.data_ptr() for _, b in tr]), (C.c_size_t * 3)(*ns),
                              P(*[o.data_ptr() for o in outs])) == -1 and b"Wiener" in L.srtLastError()
    eng.close()


@pytest.mark.gpu
def test_python_splits_into_calls(oracle, coeffs):
    """Engine(wiener=1).separate_batch over 11 tiles at max_tiles = 4: several srtSeparateBatchWiener calls, each track bit-equal to separate() on it;
    wiener=0 on that engine equals a plain engine's separate_batch and leaves the engine's setting as it was"""
    import torch
    from spleeterrt_amd import stream
    ns = list(TRACKS) + [4096 * 9 + 11, 64 * 1024 * 2]               # 8 + 1 + 2 = 11 tiles
    eng = _engine(coeffs, 2, max_tiles=4, batch_invariant=True, wiener=1)
    groups = stream.pack_tracks(ns, T_S, 4)
    assert len(groups) >= 3
    tr = _tracks(oracle, ns, seed=900)
    eng.set_timing(True)
    got = eng.separate_batch(tr)
    names = [n for n, _ in eng.get_timing()]
    eng.set_timing(False)
    assert names.count("stft_batch") == len(groups) and names.count("wiener_filter_batch") == len(groups) and names.count("istft_batch") == len(groups)
    for k, (L, R) in enumerate(tr):
        assert torch.equal(got[k], eng.separate(L, R)), k
    off = eng.separate_batch(tr, wiener=0)
    assert eng.wiener == 1
    plain = _engine(coeffs, 2, max_tiles=4, batch_invariant=True)
    want = plain.separate_batch(tr)
    for k in range(len(tr)):
        assert torch.equal(off[k], want[k]), k
        assert not torch.equal(off[k], got[k]), k                    # (the filter does change the stems)
    plain.close()
    eng.close()
