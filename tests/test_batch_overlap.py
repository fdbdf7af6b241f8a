"""srtSeparateBatchOverlap: overlapped network tiles with cross-faded masks inside every track of a packed batch (§10.2).

CPU: srtBatchPlanOverlap against stream.pack_tracks(.., overlap) and a per-track srtOverlapTiles prefix sum, O = 0 against srtBatchPlan, every refusal of the
plan with its text, the null-engine call.  GPU: every track of one call equals srtSeparate on it alone with srtSetOverlap(O) (bit for bit under
batch_invariant, both inverse-kernel families, with and without ratio_mask, O = 1 / 16 / 32), O = 0 is srtSeparateBatch, the average mask extension (stems and
each track's gain table), the default mode, the CPU oracle end to end, the fp16 mode at the bench shape, coverage of every output, capacity in overlapped
tiles, every refusal, and the Python grouping over several calls."""
import ctypes as C

import numpy as np
import pytest

T_S, F_S = 64, 512
MODES = (1, 0, 1, 0, 1, 0, 1, 0)
# rows 160 (an exact fit at O = 16 and 32: no pad row), 4 (the minimum length), 65 (one new row in a second tile that is nearly all pad), 64 (rows = T, one
# tile), 137 (ragged tail).  A one-tile track follows a multi-tile track, and a multi-tile track follows a one-tile track.
TRACKS_OV = (160 * 1024, 4096, 65 * 1024 - 300, 64 * 1024, 140077)
ROWS_OV = (160, 4, 65, 64, 137)
TILES_OV = {16: (3, 1, 2, 1, 3), 32: (4, 1, 2, 1, 4), 1: (3, 1, 2, 1, 3), 0: (3, 1, 2, 1, 3)}      # 10 / 12 / 10 packed tiles: max_tiles = 12 holds them all
MAX_TILES = 12


def _lib():
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


def _plan_ov(L, ns, T, O):
    k = len(ns)
    t0 = (C.c_size_t * max(k, 1))()
    tot = C.c_size_t(0)
    rc = L.srtBatchPlanOverlap((C.c_size_t * max(k, 1))(*ns), k, T, O, t0, C.byref(tot))
    return rc, list(t0[:k]), tot.value


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_track_list_geometry():
    """the table of the track list: rows and overlapped tiles per track as the tests below assume them"""
    from spleeterrt_amd import stream
    assert tuple(stream.stft_rows(n) for n in TRACKS_OV) == ROWS_OV
    for O, want in TILES_OV.items():
        assert tuple(stream.overlap_tiles(r, T_S, O) for r in ROWS_OV) == want, O
        assert sum(want) <= MAX_TILES
    assert sum(TILES_OV[32]) == MAX_TILES
    assert 2 * (T_S - 16) + T_S == 160 and 3 * (T_S - 32) + T_S == 160      # the exact fits: the last tile has no pad row


def test_plan_matches_pack_tracks_and_overlap_tiles():
    from spleeterrt_amd import stream
    L = _lib()
    rng = np.random.default_rng(11)
    T = T_S
    lists = [list(TRACKS_OV)]
    for trial in range(20):
        k = int(rng.integers(1, 12))
        ns = [int(x) for x in rng.integers(4096, 12 * T * 1024, size=k)]
        ns[0] = 4096
        if k > 1:
            ns[1] = int(rng.integers(1, 4)) * T * 1024
        if k > 2:
            ns[2] = int(rng.integers(1, 4)) * T * 1024 + 1
        lists.append(ns)
    for ns in lists:
        for O in (0, 1, 16, 32):
            rc, t0, tot = _plan_ov(L, ns, T, O)
            assert rc == 0, L.srtLastError()
            want = [int(L.srtOverlapTiles(stream.stft_rows(n), T, O)) for n in ns]
            assert want == [stream.overlap_tiles(stream.stft_rows(n), T, O) for n in ns]
            assert tot == sum(want) and t0 == [sum(want[:i]) for i in range(len(ns))], (ns, O)
            g = stream.pack_tracks(ns, T, 1 << 30, overlap=O)
            assert len(g) == 1 and g[0].tracks == list(range(len(ns))) and g[0].tile0 == t0 and g[0].ntiles == tot
            if O == 0:                                                  # ... is srtBatchPlan, and pack_tracks as it always was
                t0b = (C.c_size_t * len(ns))()
                totb = C.c_size_t(0)
                assert L.srtBatchPlan((C.c_size_t * len(ns))(*ns), len(ns), T, t0b, C.byref(totb)) == 0
                assert list(t0b) == t0 and totb.value == tot
                assert stream.pack_tracks(ns, T, 1 << 30) == g
    for O in (1, 16, 32):
        rc, t0, tot = _plan_ov(L, list(TRACKS_OV), T, O)
        assert tot == sum(TILES_OV[O]) and t0 == [sum(TILES_OV[O][:i]) for i in range(5)]
    # greedy cut by OVERLAPPED tiles
    g = stream.pack_tracks(list(TRACKS_OV), T, 4, overlap=16)
    assert [x.tracks for x in g] == [[0, 1], [2, 3], [4]] and [x.ntiles for x in g] == [4, 3, 3] and g[1].tile0 == [0, 2]
    with pytest.raises(ValueError, match="max_tiles"):
        stream.pack_tracks(list(TRACKS_OV), T, 3, overlap=32)          # track 0 alone takes four overlapped tiles
    with pytest.raises(ValueError):
        stream.pack_tracks(list(TRACKS_OV), T, 12, overlap=33)


def test_layout_rule_writes_every_slot_once():
    """the device rule restated (srt_ov_row per track + the pad rule of srt_stft_batch_ov_kernel): over a packed batch every magnitude slot (tile, t) of every
    track's tiles is written exactly once - by row jS + t as its primary or its second copy, or by the pad loop, which touches the track's LAST tile only - and
    nothing outside the track's tiles is"""
    from spleeterrt_amd import stream
    rng = np.random.default_rng(5)
    T = T_S
    for O in (1, 16, 32):
        S = T - O
        rows_list = list(ROWS_OV) + [1, O, S, S + 1, T + 1, S + T, S + T + 1] + [int(x) for x in rng.integers(1, 6 * T, size=30)]
        tiles = [stream.overlap_tiles(r, T, O) for r in rows_list]
        total = sum(tiles)
        hits = np.zeros((total, T), np.int32)
        tile0 = 0
        for rows, nt in zip(rows_list, tiles):
            own = hits[tile0:tile0 + nt]                                # (a view: an index outside the track's tiles raises)
            for f in range(rows):
                j1 = min(f // S, nt - 1)
                k = f - j1 * S
                own[j1, k] += 1
                if j1 > 0 and k < O:
                    own[j1 - 1, k + S] += 1
            J = nt - 1
            t0 = rows - J * S
            assert 1 <= t0 <= T, (rows, O)
            own[J, t0:] += 1
            assert rows <= nt * T                                       # the spectrum rows fit the track's packed rows
            tile0 += nt
        assert (hits == 1).all(), (O, np.argwhere(hits != 1)[:5])


def test_plan_refusals():
    L = _lib()
    tot = C.c_size_t(0)
    # tile0 may be NULL
    assert L.srtBatchPlanOverlap((C.c_size_t * 2)(4096, 160 * 1024), 2, 64, 32, None, C.byref(tot)) == 0 and tot.value == 5
    # everything srtBatchPlan refuses
    assert _plan_ov(L, [], 64, 16)[0] == -1 and b"srtBatchPlanOverlap" in L.srtLastError()
    assert _plan_ov(L, [5000], 0, 0)[0] == -1 and b"srtBatchPlanOverlap" in L.srtLastError()
    assert _plan_ov(L, [5000, 4095], 64, 16)[0] == -1 and b"4096" in L.srtLastError() and b"srtBatchPlanOverlap" in L.srtLastError()
    assert L.srtBatchPlanOverlap(None, 1, 64, 16, None, C.byref(tot)) == -1 and b"srtBatchPlanOverlap" in L.srtLastError()
    assert L.srtBatchPlanOverlap((C.c_size_t * 1)(5000), 1, 64, 16, None, None) == -1 and b"srtBatchPlanOverlap" in L.srtLastError()
    # the overlap outside 0..T/2
    for T, O in ((64, -1), (64, 33), (256, 129)):
        assert _plan_ov(L, [5000], T, O)[0] == -1 and b"overlap" in L.srtLastError() and b"srtBatchPlanOverlap" in L.srtLastError(), (T, O)
    assert _plan_ov(L, [5000], 64, 32)[0] == 0 and _plan_ov(L, [5000], 256, 128)[0] == 0


def test_null_engine():
    L = _lib()
    P1 = C.c_void_p * 1
    assert L.srtSeparateBatchOverlap(None, 1, P1(None), P1(None), (C.c_size_t * 1)(4096), P1(None), 16) == -1
    assert b"srtSeparateBatchOverlap" in L.srtLastError()


def test_new_kernels_keep_their_single_signal_resources():
    """srt_dsp.hip compiled with the resource remarks: every batch overlap kernel has no scratch, and the transforms at least the occupancy of the single-signal
    overlap kernel whose body they run (DESIGN.md §10.2's table); the gain-table kernel uses no LDS"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the resource check needs the compiler the library is built with")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + root + "/include", "-I" + root + "/spleeterrt_amd/csrc", "-Wno-pass-failed",
           "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(root, "spleeterrt_amd", "csrc", "srt_dsp.hip"), "-o", os.devnull]
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
    tf = {"true": True, "false": False}
    pairs = {"srt_stft_batch_ov_kernel": "srt_stft_ov_kernel"}
    for k in res:
        m = re.match(r"srt_istft_batch_ov_kernel<(\w+), (\w+), (\w+), (\w+)>$", k)
        if m:
            ola3, ratio, m16, ext = (tf[x] for x in m.groups())
            e = "_ext" if ext else ""
            pairs[k] = ("srt_istft_ola3_ov%s_kernel<4, %s, %s>" % (e, m.group(2), m.group(3))) if ola3 else "srt_istft_ola_ov%s_kernel<%s>" % (e, m.group(2))
        m = re.match(r"srt_mask_ext_batch_kernel<(\w+), (\w+)>$", k)
        if m:
            pairs[k] = "srt_mask_ext_kernel<%s, %s, true>" % m.groups()
    assert len(pairs) == 1 + 10 + 3, sorted(pairs)
    for k, sib in sorted(pairs.items()):
        assert k in res and sib in res, (k, sib)
        a, b = res[k], res[sib]
        print("%-58s vgpr %s sgpr %s scratch %s occ %s | %s vgpr %s occ %s" % (k, a["VGPRs"], a["TotalSGPRs"], a["ScratchSize [bytes/lane]"],
              a["Occupancy [waves/SIMD]"], sib, b["VGPRs"], b["Occupancy [waves/SIMD]"]))
        assert int(a["ScratchSize [bytes/lane]"]) == 0 and int(a["VGPRs Spill"]) == 0, (k, a)
        if k.startswith("srt_mask_ext"):
            # the gain-table kernel streams the masks once and keeps no data on chip: no LDS; the track look-up costs it registers (84 / 115 / 130 VGPRs
            # against 62 / 88 / 130), so it is held to the family's floor - 3 waves per SIMD, what the half-mask single-signal form runs at - not to its sibling
            assert int(a["LDS Size [bytes/block]"]) == 0 and int(a["Occupancy [waves/SIMD]"]) >= 3, (k, a)
        else:
            assert int(a["Occupancy [waves/SIMD]"]) >= int(b["Occupancy [waves/SIMD]"]), (k, a, b)
    # three workgroups per CU for the non-ratio three-per-CU forms, two for the rest (the launch bounds; workgroups of four waves, one per SIMD)
    for k in pairs:
        if k.startswith("srt_istft_batch_ov_kernel<true, false"):
            assert int(res[k]["Occupancy [waves/SIMD]"]) >= 3, (k, res[k])
        elif k.startswith("srt_istft_batch_ov_kernel"):
            assert int(res[k]["Occupancy [waves/SIMD]"]) >= 2, (k, res[k])
    assert int(res["srt_stft_batch_ov_kernel"]["Occupancy [waves/SIMD]"]) >= 3


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _engine(coeffs, S=2, **kw):
    import spleeterrt_amd as srt
    kw.setdefault("variant", srt.VARIANT_VST)
    kw.setdefault("F", F_S)
    kw.setdefault("T", T_S)
    kw.setdefault("max_tiles", MAX_TILES)
    eng = srt.Engine(stem_modes=MODES[:S], **kw)
    for s in range(S):
        eng.set_coeff(s, coeffs(s))
    return eng


def _tracks(oracle, ns, seed):
    import torch
    out = []
    for k, n in enumerate(ns):
        L, R = oracle.synth_audio(n, seed + k, True)
        out.append((torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()))
    return out


def _rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


def _timed(eng, fn):
    eng.set_timing(True)
    out = fn()
    ks = eng.get_timing_kernels()
    eng.set_timing(False)
    return out, ks


def _raw_call(eng, fn, tr, outs, *extra):
    k = len(tr)
    P = C.c_void_p * k
    return fn(eng.h, k, P(*[a.data_ptr() for a, _ in tr]), P(*[b.data_ptr() for _, b in tr]), (C.c_size_t * k)(*[int(a.numel()) for a, _ in tr]),
              P(*[o.data_ptr() for o in outs]), *extra)


def _nan_outs(eng, tr, S=2):
    import torch
    L = eng.L
    return [torch.full((S, 2, L.srtIstftLength(L.srtStftRows(int(a.numel())))), float("nan"), device="cuda") for a, _ in tr]


def _singles(eng, tr, O):
    """separate() per track with set_overlap(O); the engine's setting is put back"""
    own = eng.overlap
    eng.set_overlap(O)
    out = [eng.separate(L, R).clone() for L, R in tr]
    eng.set_overlap(own)
    return out


def _form(F, ratio, m16=False, ext=False):
    """srt_istft_batch_ov_kernel<OLA3, RATIO, M16, EXT>"""
    return "<%s>" % ", ".join("true" if x else "false" for x in (F <= 1024, ratio, m16, ext))


@pytest.mark.gpu
@pytest.mark.parametrize("O", [1, 16, 32])
@pytest.mark.parametrize("ratio", [False, True])
@pytest.mark.parametrize("F", [512, 1536])
def test_bit_identical_to_single_tracks(oracle, coeffs, F, ratio, O):
    """batch_invariant, fp32: every track's stems from ONE srtSeparateBatchOverlap call are bit for bit srtSeparate of that track alone after srtSetOverlap(O);
    one stft_batch and one istft_batch launch, the overlap forms for this F and ratio"""
    import torch
    eng = _engine(coeffs, F=F, batch_invariant=True, ratio_mask=ratio)
    tr = _tracks(oracle, TRACKS_OV, seed=2100)
    got, ks = _timed(eng, lambda: eng.separate_batch(tr, overlap=O))
    assert eng.overlap == 0
    names = [n for n, _ in ks]
    assert names.count("stft_batch") == 1 and names.count("istft_batch") == 1, names
    assert ks[0] == ("stft_batch", "srt_stft_batch_ov_kernel"), ks[0]
    assert ks[-1] == ("istft_batch", "srt_istft_batch_ov_kernel" + _form(F, ratio)), ks[-1]
    ref = _singles(eng, tr, O)
    for k in range(len(tr)):
        assert got[k].shape == ref[k].shape
        assert torch.equal(got[k], ref[k]), (k, float((got[k] - ref[k]).abs().max()))
    assert not torch.equal(got[0], eng.separate(*tr[0]))                # (the overlap does change the stems of a multi-tile track)
    eng.close()


@pytest.mark.gpu
def test_overlap_zero_is_separate_batch(oracle, coeffs):
    """overlap_rows = 0: the stems and the launch list of srtSeparateBatch"""
    import torch
    eng = _engine(coeffs, batch_invariant=True)
    tr = _tracks(oracle, TRACKS_OV, seed=2200)
    eng.separate_batch(tr, overlap=0)                                    # (first call allocates the table)
    want, ks0 = _timed(eng, lambda: [o.clone() for o in eng.separate_batch(tr, overlap=0)])
    outs = _nan_outs(eng, tr)
    rc, ks1 = _timed(eng, lambda: _raw_call(eng, eng.L.srtSeparateBatchOverlap, tr, outs, 0))
    assert rc == 0, eng.L.srtLastError()
    assert ks0 == ks1
    assert ks1[0] == ("stft_batch", "srt_stft_batch_kernel") and ks1[-1] == ("istft_batch", "srt_istft_batch_kernel<true, false, false>")
    for k in range(len(tr)):
        assert torch.equal(outs[k], want[k]), k
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [False, True])
@pytest.mark.parametrize("F", [512, 1536])
def test_mask_extension_average(oracle, coeffs, F, ratio):
    """SRT_MASK_EXT_AVERAGE at O = 16: the stems are bit-equal to the single calls, and each track's gain table - read at the packed rows tile0 * T .. - is
    bit-equal to the table the single call leaves"""
    import torch
    O = 16
    eng = _engine(coeffs, F=F, batch_invariant=True, ratio_mask=ratio, mask_extension="average")
    tr = _tracks(oracle, TRACKS_OV, seed=2300)
    got, ks = _timed(eng, lambda: eng.separate_batch(tr, overlap=O))
    assert ks[-2:] == [("mask_ext", "srt_mask_ext_batch_kernel<false, %s>" % ("true" if ratio else "false")),
                       ("istft_batch", "srt_istft_batch_ov_kernel" + _form(F, ratio, ext=True))], ks[-2:]
    total = sum(TILES_OV[O])
    packed = np.stack([eng.mask_ext(s, total * T_S) for s in range(2)])      # [S][total * T][2]
    eng.set_overlap(O)
    tile0 = 0
    for k, (L, R) in enumerate(tr):
        ref = eng.separate(L, R)
        assert torch.equal(got[k], ref), (k, float((got[k] - ref).abs().max()))
        rows = ROWS_OV[k]
        single = np.stack([eng.mask_ext(s, rows) for s in range(2)])
        mine = packed[:, tile0 * T_S:tile0 * T_S + rows]
        assert np.isfinite(single).all() and np.array_equal(mine, single), (k, float(np.abs(mine - single).max()))
        tile0 += TILES_OV[O][k]
    eng.close()


@pytest.mark.gpu
def test_default_mode_matches_single_tracks(oracle, coeffs):
    """not batch_invariant (the network's split-K association is free to differ with the batch): max-abs <= 1e-5 of the peak against the single calls, the bound
    of tests/test_batch.py::test_batch_default_mode_matches_single_tracks"""
    eng = _engine(coeffs)
    tr = _tracks(oracle, TRACKS_OV, seed=2400)
    got = [o.cpu().numpy() for o in eng.separate_batch(tr, overlap=16)]
    ref = [o.cpu().numpy() for o in _singles(eng, tr, 16)]
    eng.close()
    for k in range(len(tr)):
        assert got[k].shape == ref[k].shape
        peak = float(np.abs(ref[k]).max())
        err = float(np.abs(got[k] - ref[k]).max())
        print("default mode track %d: max-abs / peak = %.3g" % (k, err / peak))
        assert err <= 1e-5 * peak, (k, err / peak)


def _blend_rows(masks, rows, T, O):
    """the rule of DESIGN.md §13 on the host, fp32 step by step: masks [S][tiles][2][T][F] in the overlapped layout -> per-row masks [S][2][rows][F]"""
    from spleeterrt_amd import stream
    S_, nt = masks.shape[0], masks.shape[1]
    assert nt == stream.overlap_tiles(rows, T, O)
    st = T - O
    out = np.empty((S_, 2, rows, masks.shape[-1]), np.float32)
    for r in range(rows):
        j1 = min(r // st, nt - 1)
        k = r - j1 * st
        b = masks[:, j1, :, k]
        if j1 > 0 and k < O:
            a = masks[:, j1 - 1, :, k + st]
            w = np.float32(k + 0.5) / np.float32(O)
            out[:, :, r] = a + w * (b - a)
        else:
            out[:, :, r] = b
    return out


def _oracle_masks(oracle, coeffs, re, im, T, F, O, S):
    """the network of every (stem, overlapped tile) of one track on the CPU oracle: masks [S][tiles][2][T][F]"""
    from spleeterrt_amd import stream
    rows = re.shape[1]
    nt, st = stream.overlap_tiles(rows, T, O), T - O
    masks = np.empty((S, nt, 2, T, F), np.float32)
    for j in range(nt):
        mag = oracle.magnitude_tile(re, im, j * st, T, F)
        for s in range(S):
            masks[s, j] = oracle.forward(coeffs(s), mag, MODES[s], oracle.VARIANT_VST)
    return masks


def _oracle_overlap(oracle, coeffs, L, R, T, F, O, S, ratio, oob=0.1, masks=None):
    """tests/test_overlap.py::_oracle_overlap: the feature restated over the oracle's stages - stft; magnitudes of rows [jS, jS + T) per tile; the network per
    (stem, tile); blend; ratio; mask; istft.  (masks: the network's output of an earlier call on the same track - it does not depend on `ratio`.)"""
    re, im = oracle.stft(L, R)
    rows = re.shape[1]
    if masks is None:
        masks = _oracle_masks(oracle, coeffs, re, im, T, F, O, S)
    m = _blend_rows(masks, rows, T, O)
    if ratio:
        m = oracle.ratio_mask(m)
    out = []
    for s in range(S):
        r, i = re.copy(), im.copy()
        r[:, :, :F] *= m[s]
        i[:, :, :F] *= m[s]
        r[:, :, F:2049] *= np.float32(oob)
        i[:, :, F:2049] *= np.float32(oob)
        out.append(oracle.istft(r, i))
    return np.stack(out), masks


_ORACLE_MASKS = {}      # track index -> the oracle network's masks at O = 16, 4 stems (shared by the two ratio cases; never modified)


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [False, True])
def test_end_to_end_against_the_oracle(oracle, coeffs, ratio):
    """4 stems fp32, O = 16: the 4096-sample track, the 65-row track and the ragged 137-row track of one batch call against the oracle restatement of each
    track alone: stems rel-RMS <= 1e-4 and max-abs <= 1e-4 of the peak (the project's fp32 bounds)"""
    S, O = 4, 16
    eng = _engine(coeffs, S=S, ratio_mask=ratio)
    tr = _tracks(oracle, TRACKS_OV, seed=2500)
    got = [o.cpu().numpy() for o in eng.separate_batch(tr, overlap=O)]
    eng.close()
    for k in (1, 2, 4):
        L, R = tr[k][0].cpu().numpy(), tr[k][1].cpu().numpy()
        ref, _ORACLE_MASKS[k] = _oracle_overlap(oracle, coeffs, L, R, T_S, F_S, O, S, ratio, masks=_ORACLE_MASKS.get(k))
        assert got[k].shape == ref.shape and np.isfinite(got[k]).all()
        for s in range(S):
            peak = float(np.abs(ref[s]).max())
            rr, ma = _rel_rms(got[k][s], ref[s]), float(np.abs(got[k][s] - ref[s]).max()) / peak
            print("oracle ratio=%d track %d stem %d: rel-RMS %.3g, max-abs / peak %.3g" % (ratio, k, s, rr, ma))
            assert rr <= 1e-4, (ratio, k, s, rr)
            assert ma <= 1e-4, (ratio, k, s, ma)


@pytest.mark.gpu
def test_fp16_mode_at_the_bench_shape(oracle, coeffs):
    """the fp16 mode at F = 1024, T = 256, O = 64, max_tiles = 5: a 300-row track (2 overlapped tiles) and a 500-row track (3) in one call.  Four stems: the half
    masks need stems x tiles >= 16 head instances (srt_head_out16_ok), which the five packed tiles reach and a single track does not - so the single calls
    read float masks and the comparison is the fp16 class, rel-RMS <= 1e-2, not bits."""
    import spleeterrt_amd as srt
    from spleeterrt_amd import stream
    T, F, O, S = 256, 1024, 64, 4
    ns = (300 * 1024 - 77, 500 * 1024 - 500)
    assert [stream.overlap_tiles(stream.stft_rows(n), T, O) for n in ns] == [2, 3]
    eng = _engine(coeffs, S=S, F=F, T=T, max_tiles=5, precision=srt.PREC_F16)
    tr = _tracks(oracle, ns, seed=2600)
    eng.separate_batch(tr, overlap=O)
    got, ks = _timed(eng, lambda: [o.cpu().numpy() for o in eng.separate_batch(tr, overlap=O)])
    assert ks[0] == ("stft_batch", "srt_stft_batch_ov_kernel") and ks[-1] == ("istft_batch", "srt_istft_batch_ov_kernel<true, false, true, false>"), (ks[0], ks[-1])
    ref = [o.cpu().numpy() for o in _singles(eng, tr, O)]
    eng.close()
    for k in range(2):
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all()
        for s in range(S):
            rr = _rel_rms(got[k][s], ref[k][s])
            print("fp16 bench shape track %d stem %d: rel-RMS %.3g" % (k, s, rr))
            assert rr <= 1e-2, (k, s, rr)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [512, 1536])
def test_writes_every_sample_and_nothing_past(oracle, coeffs, F):
    """outputs pre-filled with NaN hold none afterwards; the guard zone behind each keeps its pattern"""
    import torch
    eng = _engine(coeffs, F=F)
    tr = _tracks(oracle, TRACKS_OV, seed=2700)
    L = eng.L
    need = [2 * 2 * L.srtIstftLength(L.srtStftRows(n)) for n in TRACKS_OV]
    for O in (16, 32):
        outs = [torch.full((m + 5000,), float("nan"), device="cuda") for m in need]
        for o, m in zip(outs, need):
            o[m:] = 12345.0
        eng.separate_batch(tr, outs, overlap=O)
        for k, (o, m) in enumerate(zip(outs, need)):
            h = o.cpu().numpy()
            assert np.isfinite(h[:m]).all(), (O, k, int(np.isnan(h[:m]).sum()))
            assert (h[m:] == 12345.0).all(), (O, k)
    eng.close()


@pytest.mark.gpu
def test_capacity_counts_overlapped_tiles(oracle, coeffs):
    """a list whose ceil(rows / T) sum fits max_tiles but whose overlapped sum does not is refused, with max_tiles in the text and nothing written; the
    largest list that fits is accepted"""
    import torch
    from spleeterrt_amd import stream
    O, mt = 32, 4
    eng = _engine(coeffs, max_tiles=mt)
    big = (128 * 1024, 64 * 1024, 64 * 1024)                           # 2 + 1 + 1 back-to-back tiles, 3 + 1 + 1 overlapped
    fit = (96 * 1024, 64 * 1024, 64 * 1024)                            # 96 rows: the most that two overlapped tiles hold
    assert sum((stream.stft_rows(n) + T_S - 1) // T_S for n in big) == mt
    assert sum(stream.overlap_tiles(stream.stft_rows(n), T_S, O) for n in big) == mt + 1
    assert sum(stream.overlap_tiles(stream.stft_rows(n), T_S, O) for n in fit) == mt and stream.overlap_tiles(97, T_S, O) == 3
    tr = _tracks(oracle, big, seed=2800)
    outs = _nan_outs(eng, tr)
    assert _raw_call(eng, eng.L.srtSeparateBatchOverlap, tr, outs, O) == -1
    msg = eng.L.srtLastError()
    assert b"max_tiles" in msg and b"srtBatchPlanOverlap" in msg, msg
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)
    assert _raw_call(eng, eng.L.srtSeparateBatch, tr, outs) == 0, eng.L.srtLastError()      # ... and it does fit the back-to-back cut
    trf = [(tr[0][0][:fit[0]].contiguous(), tr[0][1][:fit[0]].contiguous())] + tr[1:]
    outf = _nan_outs(eng, trf)
    assert _raw_call(eng, eng.L.srtSeparateBatchOverlap, trf, outf, O) == 0, eng.L.srtLastError()
    for o in outf:
        assert torch.isfinite(o).all()
    eng.close()


@pytest.mark.gpu
def test_refusals(oracle, coeffs):
    """the mix, the Wiener filter, an overlap outside 0..T/2, a stream capture, everything srtSeparateBatch refuses: -1 with text and nothing written; missing
    weights: -5.  With srtSetOverlap(16) on the engine srtSeparateBatch still refuses, and srtSeparateBatchOverlap(.., 32) runs at ITS overlap: bit for bit the
    single calls at O = 32, which is what test_bit_identical_to_single_tracks holds the call to"""
    import torch
    import spleeterrt_amd as srt
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                   # (a non-default stream, so that the capture case below can capture it)
        eng = _engine(coeffs, batch_invariant=True)
    L = eng.L
    tr = _tracks(oracle, TRACKS_OV, seed=2900)
    outs = _nan_outs(eng, tr)
    torch.cuda.synchronize()
    fn = L.srtSeparateBatchOverlap
    k = len(tr)
    P = C.c_void_p * k
    Lp, Rp, Op = [a.data_ptr() for a, _ in tr], [b.data_ptr() for _, b in tr], [o.data_ptr() for o in outs]
    ns = (C.c_size_t * k)(*TRACKS_OV)
    for bad in (-1, T_S // 2 + 1, T_S):
        assert _raw_call(eng, fn, tr, outs, bad) == -1 and b"overlap" in L.srtLastError() and b"srtSeparateBatchOverlap" in L.srtLastError(), bad
    eng.set_mix(np.array([[1.0, 0.0, 0.0]], np.float32))
    assert _raw_call(eng, fn, tr, outs, 16) == -1 and b"mix" in L.srtLastError() and b"srtSeparateBatchOverlap" in L.srtLastError()
    eng.set_mix(None)
    eng.set_wiener(1)
    assert _raw_call(eng, fn, tr, outs, 16) == -1 and b"Wiener" in L.srtLastError() and b"srtSeparateBatchOverlap" in L.srtLastError()
    assert _raw_call(eng, fn, tr, outs, 0) == -1 and b"Wiener" in L.srtLastError()
    eng.set_wiener(0)
    # what srtSeparateBatch refuses
    assert fn(eng.h, k, P(*([Lp[0], None] + Lp[2:])), P(*Rp), ns, P(*Op), 16) == -1 and b"null" in L.srtLastError()
    assert fn(eng.h, k, P(*Lp), P(*Rp), ns, P(*(Op[:4] + [None])), 16) == -1 and b"null" in L.srtLastError()
    assert fn(eng.h, k, None, P(*Rp), ns, P(*Op), 16) == -1 and b"arrays" in L.srtLastError()
    assert fn(eng.h, k, P(*Lp), P(*Rp), (C.c_size_t * k)(TRACKS_OV[0], 4095, *TRACKS_OV[2:]), P(*Op), 16) == -1 and b"4096" in L.srtLastError()
    assert fn(eng.h, 0, P(*Lp), P(*Rp), ns, P(*Op), 16) == -1 and L.srtLastError()
    bare = srt.Engine(F=F_S, T=T_S, stem_modes=(1, 0), variant=srt.VARIANT_VST, max_tiles=MAX_TILES)
    assert _raw_call(bare, fn, tr, outs, 16) == -5 and b"weights" in L.srtLastError()
    bare.close()
    torch.cuda.synchronize()
    dummy = torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                      # the engine's stream is capturing: refused before anything is enqueued
        dummy += 1.0                                                # (so that the captured graph is not empty)
        rc = _raw_call(eng, fn, tr, outs, 16)
        msg = L.srtLastError()
    assert rc == -1 and b"capture" in msg, (rc, msg)
    del graph
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)
    # the engine's own setting is neither read nor changed
    with torch.cuda.stream(side):
        eng.set_overlap(16)
        assert _raw_call(eng, L.srtSeparateBatch, tr, outs) == -1 and b"overlap" in L.srtLastError()
        side.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs)
        assert _raw_call(eng, fn, tr, outs, 32) == 0, L.srtLastError()
        side.synchronize()
        assert eng.overlap == 16 and eng.tiles(160) == 3
        ref = _singles(eng, tr, 32)
        side.synchronize()
        for i in range(k):
            assert torch.equal(outs[i], ref[i]), i
        at16 = eng.separate(*tr[0])                                  # (the engine's setting is still 16, and 16 is not 32)
        side.synchronize()
        assert not torch.equal(at16, ref[0])
    eng.close()


@pytest.mark.gpu
def test_python_splits_into_calls(oracle, coeffs):
    """Engine(overlap=16).separate_batch at max_tiles = 4: the list is cut by overlapped tiles into three srtSeparateBatchOverlap calls, each track bit-equal to
    separate() on that engine; overlap=0 on that engine is a plain engine's separate_batch and leaves the setting as it was; the filter with an overlap is refused"""
    import torch
    import spleeterrt_amd as srt
    from spleeterrt_amd import stream
    eng = _engine(coeffs, max_tiles=4, batch_invariant=True, overlap=16)
    groups = stream.pack_tracks(TRACKS_OV, T_S, 4, overlap=16)
    assert len(groups) == 3
    tr = _tracks(oracle, TRACKS_OV, seed=3000)
    got, ks = _timed(eng, lambda: eng.separate_batch(tr))
    names = [n for n, _ in ks]
    assert names.count("stft_batch") == 3 and names.count("istft_batch") == 3
    assert [kn for n, kn in ks if n == "stft_batch"] == ["srt_stft_batch_ov_kernel"] * 3
    for k, (L, R) in enumerate(tr):
        assert torch.equal(got[k], eng.separate(L, R)), k
    off = eng.separate_batch(tr, overlap=0)
    assert eng.overlap == 16
    plain = _engine(coeffs, max_tiles=4, batch_invariant=True)
    want = plain.separate_batch(tr)
    for k in range(len(tr)):
        assert torch.equal(off[k], want[k]), k
    plain.close()
    with pytest.raises(srt.EngineError, match="Wiener"):
        eng.separate_batch(tr, wiener=1)
    eng.close()
