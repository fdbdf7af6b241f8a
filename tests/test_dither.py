"""TPDF-dithered 16-bit output: srtPcm16PackDither, SRT_HOST_OUT_DITHER on every call that takes `flags`, srtSetDitherSeed, and
SPLEETERRT_DITHER of the CLI.

The dither is a pure function of (seed, plane, i) in 32-bit integer arithmetic, so the device's output is compared with a numpy restatement bit for bit; only
the checks of the restatement's own statistics are statistical, and their bounds are five sampling sigmas of 2^20 draws (sigma of the mean 4.0e-4, of the
variance 1.9e-4, of a correlation 9.8e-4).  The rule:
    mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16                       (uint32, wrap-around)
    k = mix32(lo32(seed) ^ mix32(hi32(seed) ^ mix32(plane + 0x9e3779b9)));  h = mix32(lo32(i) ^ mix32(hi32(i) ^ k))
    a = mix32(h ^ 0x68bc21eb) >> 8;  b = mix32(h ^ 0x02e5be93) >> 8;  d = float32(a - b) * 2^-24
    v = rint(float32(x) * 32768 + d) in float32;  q = clip(v, -32768, 32767), NaN -> 0;  clipped = NaN or v outside the range
with plane = 2 * pair + channel in output order and i the sample's index in its whole output plane.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_pcm24 as P24
from test_pcm16 import F, T, _engine
from test_pcm24 import PATHS, _cli_path, cli_runs, float_ref, pack_harness, run_path, signal24, strides_of

COUNTS = P24.COUNTS
U32 = np.uint32


def mix32(x):
    x = np.array(x, np.uint32, copy=True, ndmin=1)
    with np.errstate(over="ignore"):
        x ^= x >> U32(16)
        x *= U32(0x7feb352d)
        x ^= x >> U32(15)
        x *= U32(0x846ca68b)
        x ^= x >> U32(16)
    return x


def dither_ab(seed, plane, i):
    """the two 24-bit uniforms of (seed, plane) at the uint64 indices i"""
    i = np.asarray(i, np.uint64)
    k = mix32(U32(seed & 0xffffffff) ^ mix32(U32(seed >> 32) ^ mix32(U32((plane + 0x9e3779b9) & 0xffffffff))))
    h = mix32((i & np.uint64(0xffffffff)).astype(np.uint32) ^ mix32((i >> np.uint64(32)).astype(np.uint32) ^ k))
    return mix32(h ^ U32(0x68bc21eb)) >> U32(8), mix32(h ^ U32(0x02e5be93)) >> U32(8)


def dither(seed, plane, i):
    """d float32 in (-1, 1) LSB"""
    a, b = dither_ab(seed, plane, i)
    return (a.astype(np.int64) - b.astype(np.int64)).astype(np.float32) * np.float32(2.0 ** -24)


def dither_rule(x, seed=0, first_pair=0, first_index=0):
    """x float32 [pairs, 2, count] -> (int16 q [pairs, 2, count], bool clipped) with plane 2 * (first_pair + p) + c and index first_index + sample"""
    x = np.asarray(x, np.float32)
    i = np.uint64(first_index) + np.arange(x.shape[2], dtype=np.uint64)
    d = np.stack([np.stack([dither(seed, 2 * (first_pair + p) + c, i) for c in range(2)]) for p in range(x.shape[0])])
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint((x * np.float32(32768) + d).astype(np.float32))
        nan = np.isnan(v)
        clipped = nan | (v < -32768) | (v > 32767)
        q = np.clip(v, -32768, 32767)
        q[nan] = 0
        return q.astype(np.int16), clipped


def as_dithered(ref, seed=0):
    """float outputs [S, 2, len] -> (int16 [S, len, 2], clipped per output): the rule with whole-output indices"""
    q, c = dither_rule(ref, seed)
    return np.ascontiguousarray(q.transpose(0, 2, 1)), [int(c[s].sum()) for s in range(ref.shape[0])]


# ------------------------------------------------------------------------------------------------ CPU
# (seed, plane, i, a, b): computed once with the restatement above and written down, so that a change of either the restatement or the device shows
TABLE = (
    (0x0, 0, 0, 13726193, 3260007),
    (0x0, 0, 1, 11618964, 2246734),
    (0x0, 1, 0, 16643363, 1167525),
    (0x1, 0, 0, 6572160, 1153984),
    (0x0, 3, 12345, 3356030, 11724154),
    (0x0123456789abcdef, 2, 7, 567672, 8571311),
    (0x0, 0, 1 << 32, 6042267, 9577330),
    (0x5, 1, (1 << 32) + 1, 13080623, 9766128),
    (0x0123456789abcdef, 3, (1 << 40) + 99, 4225815, 9886119),
    (0x7, 0, (1 << 32) - 1, 4971072, 4024158),
)


def test_the_hash_is_pinned_by_a_table():
    for seed, plane, i, a, b in TABLE:
        ga, gb = dither_ab(seed, plane, [i])
        assert (int(ga[0]), int(gb[0])) == (a, b), (hex(seed), plane, i)
        assert dither(seed, plane, [i])[0] == np.float32((a - b) / 16777216.0)
    d = dither(3, 1, np.arange(1 << 16, dtype=np.uint64))
    assert d.dtype == np.float32 and np.abs(d).max() < 1.0


def _corr(a, b):
    return abs(float(np.corrcoef(a, b)[0, 1]))


def test_the_hash_is_tpdf_noise():
    """statistical: five sampling sigmas of 2^20 draws (the module docstring)"""
    i = np.arange(1 << 20, dtype=np.uint64)
    d = {(s, p): dither(s, p, i).astype(np.float64) for s in (0, 1) for p in (0, 1)}
    for key, x in d.items():
        print(key, "mean %.3e var %.5f lag-1 %.3e min %.6f max %.6f" % (x.mean(), x.var(), _corr(x[:-1], x[1:]), x.min(), x.max()))
        assert abs(x.mean()) <= 2e-3, key
        assert abs(x.var() - 1.0 / 6.0) <= 1e-3, key
        assert _corr(x[:-1], x[1:]) <= 5e-3, key
        assert -1.0 < x.min() and x.max() < 1.0
    for s in (0, 1):
        assert _corr(d[s, 0], d[s, 1]) <= 5e-3, ("cross-plane", s)
    for p in (0, 1):
        assert _corr(d[0, p], d[1, p]) <= 5e-3, ("cross-seed", p)
    assert _corr(d[0, 0], dither(0, 0, i + np.uint64(1 << 32)).astype(np.float64)) <= 5e-3      # the index's high word
    # what the dither is for: the quantisation error of a constant c has mean 0 and variance 1/4 whatever c is
    for key, x in d.items():
        for c in (0.0, 0.3, 0.5):
            q = np.rint((np.float32(c) + x.astype(np.float32)).astype(np.float32)).astype(np.float64)
            print(key, "c = %.1f: mean of rint(c + d) %.5f, error variance %.5f" % (c, q.mean(), (q - c).var()))
            assert abs(q.mean() - c) <= 2e-3, (key, c)
            assert abs((q - c).var() - 0.25) <= 2e-3, (key, c)


def test_the_pack_refuses_bad_arguments_before_any_device_work():
    L = P24._lib()
    p = C.c_void_p(4096)                                                      # never dereferenced: every case below is refused first
    bad = [
        L.srtPcm16PackDither(None, None, 8, 1, 8, p, 8, None, 0, 0, 0), L.srtPcm16PackDither(None, p, 8, 1, 8, None, 8, None, 0, 0, 0),
        L.srtPcm16PackDither(None, p, 8, 0, 8, p, 8, None, 0, 0, 0), L.srtPcm16PackDither(None, p, 8, 65536, 8, p, 8, None, 0, 0, 0),
        L.srtPcm16PackDither(None, p, 7, 1, 8, p, 8, None, 0, 0, 0), L.srtPcm16PackDither(None, p, 8, 1, 8, p, 7, None, 0, 0, 0),
        L.srtPcm16PackDither(None, p, 8, 1, 8, p, 8, None, 0, -1, 0),
    ]
    assert bad == [-1] * len(bad) and b"srtPcm16PackDither" in L.srtLastError()
    assert L.srtSetDitherSeed(None, 1) == -1 and b"srtSetDitherSeed" in L.srtLastError()


def test_cli_refuses_dither_without_16_bit_output(tmp_path):
    cli = _cli_path()
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPLEETERRT_")}
    for extra in ({}, {"SPLEETERRT_OUT_BITS": "32"}, {"SPLEETERRT_OUT_BITS": "24"}):
        r = subprocess.run([cli, "1", "64", "512", "2", "none.wav", "none.f16"], cwd=tmp_path, capture_output=True, env=dict(env, SPLEETERRT_DITHER="7", **extra))
        assert r.returncode != 0 and b"SPLEETERRT_DITHER" in r.stderr and b"16" in r.stderr and b"none.wav" not in r.stderr, (extra, r.stderr)
    assert not os.listdir(tmp_path)


# ------------------------------------------------------------------------------------------------ GPU: the kernel
def _pack_dither(x, plane_stride, out_stride, offs, start, seed, first_pair, first_index):
    L = P24._lib()
    pairs, _, count = x.shape

    def call(pp, po, pc):
        assert L.srtPcm16PackDither(None, pp, plane_stride, pairs, count, po, out_stride, pc, seed, first_pair, first_index) == 0, L.srtLastError()
    body, clip = pack_harness(call, x, plane_stride, out_stride, offs, start, 2)
    return np.ascontiguousarray(body).view(np.int16).reshape(pairs, count, 2), clip


def _check(x, stride, offs, seed, first_pair, first_index):
    pairs = x.shape[0]
    start = [3 + 5 * p for p in range(pairs)]
    got, clip = _pack_dither(x, stride, stride, offs, start, seed, first_pair, first_index)
    rq, rc = dither_rule(x, seed, first_pair, first_index)
    what = (x.shape, stride, offs, hex(seed), first_pair, first_index)
    assert np.array_equal(got, rq.transpose(0, 2, 1)), what
    assert clip.tolist() == [start[p] + int(rc[p].sum()) for p in range(pairs)], what      # the counts are those of the dithered v, added to what was there
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("pairs", [1, 3, 5])
def test_pack_equals_the_restatement_at_every_size_stride_alignment_and_index(pairs):
    rng = np.random.default_rng(1600 + pairs)
    for count in COUNTS:
        x = (0.5 * rng.standard_normal((pairs, 2, count))).astype(np.float32)      # |x| >= 1 about once in 22 samples
        x.reshape(-1)[:3] = (np.nan, 1.0, -1.0)[:min(3, x.size)]
        for stride in strides_of(count):
            for offs in ((0, 0), (1, 0), (0, 1), (1, 1)):
                for first_index in (0, 12345, (1 << 32) - 3):                      # the last one crosses 2^32 inside the launch
                    for first_pair in (0, 2):
                        _check(x, stride, offs, 0x0123456789abcdef, first_pair, first_index)


@pytest.mark.gpu
def test_seeds_and_the_table_on_the_device():
    """the device at the table's (seed, plane, i): a launch of nine frames of x = 1000 LSB that holds index i at frame `at`, in the vector group and in the tail"""
    for seed, plane, i, a, b in TABLE:
        x = np.full((1, 2, 9), np.float32(1000.0 / 32768.0), np.float32)
        d = np.float32((a - b) / 16777216.0)
        for at in (0, 2, 8):
            if i >= at:
                got = _check(x, 16, (0, 0), seed, plane // 2, i - at)
                assert got[0, at, plane & 1] == np.int16(np.rint(np.float32(1000.0) + d)), (hex(seed), plane, i, at)


@pytest.mark.gpu
def test_two_launches_split_at_an_odd_index_give_the_bytes_of_one():
    rng = np.random.default_rng(3)
    n, cut, first = 4099, 1235, (1 << 32) - 2000
    x = (0.5 * rng.standard_normal((3, 2, n))).astype(np.float32)
    whole = _check(x, n + 5, (0, 0), 9, 1, first)
    a = _check(np.ascontiguousarray(x[:, :, :cut]), cut + 1, (0, 0), 9, 1, first)
    b = _check(np.ascontiguousarray(x[:, :, cut:]), n - cut, (0, 0), 9, 1, first + cut)
    assert np.array_equal(np.concatenate([a, b], 1), whole)
    # ... and a pair packed alone under its first_pair is the pair of the joint launch
    one = _check(np.ascontiguousarray(x[2:3]), n + 5, (0, 0), 9, 3, first)
    assert np.array_equal(one[0], whole[2])


@pytest.mark.gpu
def test_clip_counts_are_those_of_the_dithered_value_and_the_grid_stride_trip():
    """samples within one LSB of full scale clip or not as d decides; 4 x 256 x 2048 frames and more take the second trip of the loop"""
    n = 4 * 256 * 2048 + 2853
    rng = np.random.default_rng(8)
    x = np.empty((1, 2, n), np.float32)
    x[0, 0] = np.float32(32767.0 / 32768.0)                                      # v = 32767 + rint-ed d: clips when d >= 0.5
    x[0, 1] = (0.5 * rng.standard_normal(n)).astype(np.float32)
    x[0, 0, ::3] = np.float32(-1.0)                                              # v = -32768 + d: clips when d < -0.5
    import torch
    import spleeterrt_amd as srt
    out, clip = srt.pcm16_pack_dither(torch.from_numpy(x).cuda(), seed=77, first_pair=0, first_index=5)
    rq, rc = dither_rule(x, 77, 0, 5)
    plain = int((np.rint(x * np.float32(32768)) > 32767).sum() + (np.rint(x * np.float32(32768)) < -32768).sum())
    assert np.array_equal(out.cpu().numpy(), rq.transpose(0, 2, 1))
    assert clip.cpu().tolist() == [int(rc.sum())] and int(rc[0, 0].sum()) > n // 10 and int(rc.sum()) != plain


# ------------------------------------------------------------------------------------------------ GPU: the pipelines
@pytest.fixture(scope="module")
def eng(coeffs):
    e = _engine(coeffs, 2)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True])
def test_stream_dithered_output_is_the_rule_with_whole_output_indices(eng, pinned):
    import torch
    _, L, R = signal24()
    ref = float_ref(eng, "stream")
    want, wclip = as_dithered(ref)
    if pinned:
        mk = lambda a: torch.from_numpy(a.copy()).pin_memory()
        src = (mk(L), mk(R))
        buf = torch.full(want.shape, 0x5A5A, dtype=torch.int16).pin_memory()
    else:
        src = (L, R)
        buf = np.full(want.shape, 0x5A5A, np.int16)                            # every element must be overwritten
    out, clipped = eng.separate_host_stream_io(src, out_bits=16, dither=True, out=buf, pinned=pinned)
    got = out.numpy() if pinned else out
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first mismatch (stem, sample, channel) %s of %d" % (bad[0], len(bad))      # a chunk that restarted i at 0 would differ from sample 131072 on
    assert clipped.tolist() == wclip
    plain, _ = eng.separate_host_stream_io(src, out_pcm16=True, pinned=pinned)
    diff = np.asarray(plain, np.int32) - got
    assert np.abs(diff).max() == 1 and 0.30 < (diff != 0).mean() < 0.37         # fraction + d is a sum of three uniforms: it leaves (-0.5, 0.5) one time in three


@pytest.mark.gpu
def test_stream_dithered_output_counts_the_clipped_samples_of_the_dithered_value(eng):
    _, L, R = signal24()
    mags = np.sort(np.abs(float_ref(eng, "stream")).reshape(-1))
    g = np.float32(1.0 / mags[-6000])
    Lg, Rg = L * g, R * g
    want, wclip = as_dithered(eng.separate_host_stream(Lg, Rg))
    out, clipped = eng.separate_host_stream_io((Lg, Rg), out_bits=16, dither=True)
    print("clipped per stem:", clipped.tolist(), "expected", wclip)
    assert np.array_equal(out, want) and clipped.tolist() == wclip and sum(wclip) > 0


@pytest.mark.gpu
def test_the_noise_does_not_depend_on_the_chunking(coeffs):
    """max_tiles = 2 against max_tiles = 3 under batch_invariant: the floats agree bit for bit except where the overlap-add of a chunk seam associates differently,
    and wherever they do the dithered samples are identical"""
    import spleeterrt_amd as srt
    _, L, R = signal24()
    outs = {}
    for mt in (2, 3):
        e = srt.Engine(F=F, T=T, stem_modes=(1, 0), variant=srt.VARIANT_EXE, max_tiles=mt, device="cuda:0", batch_invariant=True)
        try:
            for s in range(2):
                e.set_coeff(s, coeffs(s))
            outs[mt] = (e.separate_host_stream(L, R), e.separate_host_stream_io((L, R), out_bits=16, dither=True)[0])
        finally:
            e.close()
    same = outs[2][0].view(np.uint32) == outs[3][0].view(np.uint32)              # [S, 2, len]
    print("bit-equal float samples: %.4f %%" % (100.0 * same.mean()))
    assert same.mean() >= 0.99
    d2, d3 = outs[2][1].transpose(0, 2, 1), outs[3][1].transpose(0, 2, 1)
    assert np.array_equal(d2[same], d3[same])
    assert np.array_equal(outs[3][1], as_dithered(outs[3][0])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS[1:])
def test_every_other_path_dithers_its_own_float_output(eng, path):
    _, L, R = signal24()
    ref = float_ref(eng, path)
    want, wclip = as_dithered(ref)                                              # (the rate path: i runs over the converted output)
    out, clipped = run_path(eng, path, (L, R), out_bits=16, dither=True)
    assert out.dtype == np.int16 and out.shape == want.shape
    bad = np.argwhere(out != want)
    assert bad.size == 0, "%s: first mismatch (output, sample, channel) %s of %d" % (path, bad[0], len(bad))
    assert clipped.tolist() == wclip


@pytest.mark.gpu
def test_the_seed_changes_the_dithered_bits_and_nothing_else(eng):
    import test_pcm16 as P16
    q, L, R = signal24()
    ref = float_ref(eng, "stream")
    base = eng.separate_host_stream_io((L, R), out_bits=16, dither=True)[0]
    try:
        eng.set_dither_seed(5)
        five = eng.separate_host_stream_io((L, R), out_bits=16, dither=True)[0]
        assert np.array_equal(five, as_dithered(ref, 5)[0]) and (five != base).mean() > 0.2
        assert np.array_equal(eng.separate_host_stream_io((L, R))[0], ref)
        assert np.array_equal(eng.separate_host_stream_io((L, R), out_pcm16=True)[0], P16._as_pcm(ref)[0])
        assert np.array_equal(eng.separate_host_stream_io((L, R), out_bits=24)[0], P24.as_pcm24(ref)[0])
        eng.set_dither_seed(0x0123456789abcdef)
        wide = eng.separate_host_wiener((L, R), out_bits=16, dither=True)[0]
        assert np.array_equal(wide, as_dithered(float_ref(eng, "wiener"), 0x0123456789abcdef)[0])      # the Wiener paths read the same seed
    finally:
        eng.set_dither_seed(0)
    assert np.array_equal(eng.separate_host_stream_io((L, R), out_bits=16, dither=True)[0], base)
    assert np.array_equal(base, as_dithered(ref, 0)[0])


# ------------------------------------------------------------------------------------------------ GPU: the CLI program
@pytest.mark.gpu
def test_cli_program_dithers_with_its_seed(tmp_path, oracle):
    files, texts, n = cli_runs(tmp_path, oracle, {"f32": {}, "d7": {"SPLEETERRT_OUT_BITS": "16", "SPLEETERRT_DITHER": "7"}})
    for k, nm in enumerate(("Drum", "Vocal", "Accompaniment")):
        h, body = files["f32"][nm]
        h16, body16 = files["d7"][nm]
        assert (h16["format"], h16["bits"], h16["align"], h16["data_bytes"]) == (1, 16, 4, n * 4)
        x = np.frombuffer(body, "<f4").reshape(n, 2).T[None]                     # the file holds the output's frames [4096, 4096 + n)
        want, wc = dither_rule(x, 7, k, 4096)
        assert np.array_equal(np.frombuffer(body16, "<i2").reshape(n, 2), want[0].T), nm
        if wc.any():
            assert ("in.wav_%s.wav: " % nm) in texts["d7"] and "clipped sample" in texts["d7"]
