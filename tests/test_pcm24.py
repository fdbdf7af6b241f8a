"""Packed 24-bit PCM at the host-stream boundary: srtPcm24Unpack / srtPcm24Pack, the SRT_HOST_IN_PCM24 / SRT_HOST_OUT_PCM24 flags of every
call that takes `flags`, and SPLEETERRT_OUT_BITS=24 of the CLI.  (The dithered 16-bit output of the same section: tests/test_dither.py, which shares the
references computed here.)

Every comparison is an exact integer or bit equality: the unpack (q * 2^-23) and the pack's product (x * 2^23) are exact in fp32, the float path is unchanged,
and the rounding rule has one answer.  The rule in numpy (`rule24` below, self-checked on the CPU against hand-written values):
    v = rint(float32(x) * float32(2^23));  q = clip(v, -8388608, 8388607), NaN -> 0;  clipped = NaN or v outside [-8388608, 8388607];
    bytes: q's low three bytes, little-endian.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from test_pcm16 import N_PIPE, HOST, _engine, _wav_fields, _signal

IN16, OUT16, IN24, OUT24, DITHER = 2, 4, 16, 32, 64
MAX_WGS = 2048                                   # SRT_PCM_MAX_WGS
BIG24 = 8 * 256 * MAX_WGS + 2853                 # past the grid cap of the 24-bit kernels (2048 workgroups x 256 lanes x 8 frames): a second trip, ragged tail
COUNTS = (1, 7, 8, 9, 4099)
TWO23 = np.float32(8388608)


def rule24(x):
    """-> (int32 q, bool clipped) of float32 x"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(np.asarray(x, np.float32) * TWO23)
        nan = np.isnan(v)
        clipped = nan | (v < -8388608) | (v > 8388607)
        q = np.clip(v, -8388608, 8388607)
        q[nan] = 0
        return q.astype(np.int32), clipped


def to_bytes(q):
    """int32 [...] -> uint8 [..., 3]: the low three bytes, little-endian"""
    u = np.asarray(q, np.int32).astype(np.uint32)
    return np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255], -1).astype(np.uint8)


def from_bytes(b):
    """uint8 [..., 3] -> int32 [...], sign-extended"""
    b = np.asarray(b, np.uint8).astype(np.int32)
    return ((b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16) ^ 0x800000) - 0x800000


def as_pcm24(ref):
    """float stems [S, 2, len] -> (uint8 [S, len, 2, 3], clipped per stem) by the rule"""
    q, c = rule24(ref)
    return np.ascontiguousarray(to_bytes(q.transpose(0, 2, 1))), [int(c[s].sum()) for s in range(ref.shape[0])]


def edge_list24():
    """(x float32, expected q, expected clipped)"""
    f = np.float32
    lsb = f(2.0) ** -23
    rows = [
        (f(0.0), 0, 0), (f(-0.0), 0, 0),
        (f(0.5) * lsb, 0, 0), (-f(0.5) * lsb, 0, 0),                           # ties go to even
        (f(1.5) * lsb, 2, 0), (-f(1.5) * lsb, -2, 0),
        (f(2.5) * lsb, 2, 0), (-f(2.5) * lsb, -2, 0),
        (f(1.0), 8388607, 1), (f(-1.0), -8388608, 0),                           # +1 is 2^23: clips; -1 is -2^23: fits
        (f(8388607.5) * lsb, 8388607, 1),                                       # 8388607.5 rounds to 8388608 (even): clips
        (f(-8388607.5) * lsb, -8388608, 0),
        (f(8388607.0) * lsb, 8388607, 0), (f(-8388608.0) * lsb, -8388608, 0),
        (f(-8388609.0) * lsb, -8388608, 1),
        (f(np.inf), 8388607, 1), (f(-np.inf), -8388608, 1), (f(np.nan), 0, 1),
        (np.frombuffer(struct.pack("<I", 1), np.float32)[0], 0, 0),             # smallest denormal
        (np.frombuffer(struct.pack("<I", 0x007fffff), np.float32)[0], 0, 0),    # largest denormal
        (f(1e30), 8388607, 1), (f(-1e30), -8388608, 1),
    ]
    return (np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], bool))


# ------------------------------------------------------------------------------------------------ CPU
def _lib():
    import spleeterrt_amd as srt
    return srt.load_library()


def test_symbols_exist():
    L = _lib()
    for sym in ("srtPcm24Unpack", "srtPcm24Pack", "srtPcm16PackDither", "srtSetDitherSeed"):
        getattr(L, sym)
    import spleeterrt_amd as srt
    assert (srt.HOST_IN_PCM24, srt.HOST_OUT_PCM24, srt.HOST_OUT_DITHER) == (IN24, OUT24, DITHER)
    assert callable(srt.pcm24_pack) and callable(srt.pcm24_unpack) and callable(srt.pcm16_pack_dither)
    assert hasattr(srt.Engine, "set_dither_seed")


def test_conversion_calls_refuse_bad_arguments_before_any_device_work():
    """no device here: a refusal that came after a HIP call could not return -1 with its own text"""
    L = _lib()
    p = C.c_void_p(4096)                                                      # never dereferenced: every case below is refused first
    bad = [
        L.srtPcm24Unpack(None, None, 8, p, p), L.srtPcm24Unpack(None, p, 8, None, p), L.srtPcm24Unpack(None, p, 8, p, None),
        L.srtPcm24Pack(None, None, 8, 1, 8, p, 8, None), L.srtPcm24Pack(None, p, 8, 1, 8, None, 8, None),
        L.srtPcm24Pack(None, p, 8, 0, 8, p, 8, None), L.srtPcm24Pack(None, p, 8, -1, 8, p, 8, None), L.srtPcm24Pack(None, p, 8, 65536, 8, p, 8, None),
        L.srtPcm24Pack(None, p, 7, 1, 8, p, 8, None), L.srtPcm24Pack(None, p, 8, 1, 8, p, 7, None),
    ]
    assert bad == [-1] * len(bad)
    for call, word in ((lambda: L.srtPcm24Unpack(None, None, 8, p, p), b"null"), (lambda: L.srtPcm24Pack(None, p, 8, 0, 8, p, 8, None), b"pairs"),
                       (lambda: L.srtPcm24Pack(None, p, 8, 65536, 8, p, 8, None), b"65535"),
                       (lambda: L.srtPcm24Pack(None, p, 7, 1, 8, p, 8, None), b"stride"), (lambda: L.srtPcm24Pack(None, p, 8, 1, 8, p, 7, None), b"stride")):
        assert call() == -1 and word in L.srtLastError() and b"srtPcm24" in L.srtLastError()


def test_numpy_rule_on_the_tie_and_edge_list():
    x, q, c = edge_list24()
    gq, gc = rule24(x)
    assert np.array_equal(gq, q), (gq, q)
    assert np.array_equal(gc, c), (gc, c)
    some = np.concatenate([np.arange(-8388608, -8388608 + 70000), np.arange(-70000, 70000), np.arange(8388608 - 70000, 8388608)]).astype(np.int32)
    rq, rc = rule24(some.astype(np.float32) / TWO23)
    assert np.array_equal(rq, some) and not rc.any()
    assert np.array_equal(from_bytes(to_bytes(some)), some)
    assert to_bytes(np.int32(-2)).tolist() == [0xFE, 0xFF, 0xFF] and to_bytes(np.int32(0x123456)).tolist() == [0x56, 0x34, 0x12]


def test_python_out_bits_arguments():
    """_host_io's argument checks run before the engine is touched"""
    import spleeterrt_amd as srt
    z = np.zeros(8192, np.float32)
    for kw in ({"out_pcm16": True, "out_bits": 24}, {"out_pcm16": True, "out_bits": 32}, {"out_bits": 12}, {"out_bits": 24, "dither": True}, {"dither": True}):
        with pytest.raises(ValueError):
            srt.Engine._host_io(None, (z, z), kw.pop("out_pcm16", False), 2, None, None, False, **kw)


def _cli_path():
    subprocess.check_call(["make", "-s", "-C", HOST, "spleeterrt_cli"])
    return os.path.join(HOST, "spleeterrt_cli")


def test_cli_refuses_bad_out_bits(tmp_path):
    """both refusals come before the input file is opened: nothing here exists"""
    cli = _cli_path()
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPLEETERRT_")}
    r = subprocess.run([cli, "1", "64", "512", "2", "none.wav", "none.f16"], cwd=tmp_path, capture_output=True, env=dict(env, SPLEETERRT_OUT_BITS="12"))
    assert r.returncode != 0 and all(w in r.stderr for w in (b"16", b"24", b"32")) and b"none.wav" not in r.stderr
    assert not os.listdir(tmp_path)


# ------------------------------------------------------------------------------------------------ GPU: the two kernels
GUARD = 16
SENT = 0x5A


def _unpack24(b, offs):
    """b uint8 [n, 2, 3] -> (L, R) through srtPcm24Unpack, the packed pointer offs[0] bytes and the plane pointers offs[1], offs[2] floats past a 256-byte aligned base"""
    import torch
    L = _lib()
    n = b.shape[0]
    src = torch.zeros(6 * n + 32, dtype=torch.uint8, device="cuda")
    src[offs[0]:offs[0] + 6 * n] = torch.from_numpy(b.reshape(-1)).cuda()
    width = (n + 7) // 8 * 8 + 2 * GUARD + 16
    dst = torch.full((2, width), -7.0, dtype=torch.float32, device="cuda")
    oL, oR = GUARD + offs[1], GUARD + offs[2]
    assert L.srtPcm24Unpack(None, C.c_void_p(src.data_ptr() + offs[0]), n, C.c_void_p(dst[0].data_ptr() + 4 * oL), C.c_void_p(dst[1].data_ptr() + 4 * oR)) == 0, L.srtLastError()
    d = dst.cpu().numpy()
    assert (d[0, :oL] == -7.0).all() and (d[0, oL + n:] == -7.0).all() and (d[1, :oR] == -7.0).all() and (d[1, oR + n:] == -7.0).all(), "guard words overwritten"
    return d[0, oL:oL + n], d[1, oR:oR + n]


def pack_harness(call, x, plane_stride, out_stride, offs, start, elem):
    """x float32 [pairs, 2, count] through a pack `call(planes_ptr, out_ptr, clip_ptr)` whose output sample is `elem` bytes: the planes start offs[0] floats and the
    output offs[1] samples past an aligned base; the stride padding of the planes is NaN (reading it would show in the counts); whatever lies between and around
    the outputs must keep its sentinel.  -> (uint8 [pairs, count, 2 * elem], clipped [pairs])"""
    import torch
    pairs, _, count = x.shape
    planes = np.full((2 * pairs, plane_stride), np.nan, np.float32)
    planes[:, :count] = x.reshape(2 * pairs, count)
    src = torch.zeros(2 * pairs * plane_stride + 16, dtype=torch.float32, device="cuda")
    src[offs[0]:offs[0] + planes.size] = torch.from_numpy(planes.reshape(-1)).cuda()
    fb = 2 * elem                                                               # bytes of a stereo frame
    dst = torch.full((pairs * out_stride * fb + 2 * 64 + 64,), SENT, dtype=torch.uint8, device="cuda")
    o = 64 + offs[1] * elem
    clip = torch.tensor(start, dtype=torch.int64, device="cuda")
    call(C.c_void_p(src.data_ptr() + 4 * offs[0]), C.c_void_p(dst.data_ptr() + o), C.c_void_p(clip.data_ptr()))
    d = dst.cpu().numpy()
    body = d[o:o + pairs * out_stride * fb].reshape(pairs, out_stride, fb)
    assert (d[:o] == SENT).all() and (d[o + pairs * out_stride * fb:] == SENT).all() and (body[:, count:] == SENT).all(), "wrote outside [0, count) of a pair"
    return body[:, :count].copy(), clip.cpu().numpy()


def _pack24(x, plane_stride, out_stride, offs, start):
    L = _lib()
    pairs, _, count = x.shape

    def call(pp, po, pc):
        assert L.srtPcm24Pack(None, pp, plane_stride, pairs, count, po, out_stride, pc) == 0, L.srtLastError()
    body, clip = pack_harness(call, x, plane_stride, out_stride, offs, start, 3)
    return body.reshape(pairs, count, 2, 3), clip


def _check_pack24(x, plane_stride, out_stride, offs):
    pairs = x.shape[0]
    start = [3 + 5 * p for p in range(pairs)]
    got, clip = _pack24(x, plane_stride, out_stride, offs, start)
    rq, rc = rule24(x)                                                           # [pairs, 2, count]
    assert np.array_equal(got, to_bytes(rq.transpose(0, 2, 1))), (x.shape, plane_stride, out_stride, offs)
    assert clip.tolist() == [start[p] + int(rc[p].sum()) for p in range(pairs)], (x.shape, plane_stride, out_stride, offs)      # exact, and ADDED to what was there
    return clip


def strides_of(count):
    """count + pad for pad in {0, 1, 8}, and a stride of whole 16-byte units with room behind it (the vector path for every pair at any count)"""
    return (count, count + 1, count + 8, (count + 7) // 8 * 8 + 8)


@pytest.mark.gpu
def test_every_24_bit_code_unpacks_exactly_and_packs_back():
    import torch
    import spleeterrt_amd as srt
    q = np.arange(-8388608, 8388608, dtype=np.int32)
    b = to_bytes(q).reshape(-1, 2, 3)                                            # 2^23 stereo frames, 48 MiB
    Lt, Rt = srt.pcm24_unpack(torch.from_numpy(b).cuda())
    want = q.astype(np.float32) * np.float32(2.0 ** -23)
    got = torch.stack([Lt, Rt], 1).reshape(-1).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    back, clip = srt.pcm24_pack(torch.stack([Lt, Rt])[None])
    assert back.dtype == torch.uint8 and tuple(back.shape) == (1, 1 << 23, 2, 3)
    assert np.array_equal(back.cpu().numpy().reshape(-1, 2, 3), b) and clip.cpu().tolist() == [0]


@pytest.mark.gpu
def test_unpack_equals_the_rule_at_every_size_and_alignment():
    rng = np.random.default_rng(24)
    for n in COUNTS + (MAX_WGS * 256 * 8 // 64 + 13,):
        q = rng.integers(-8388608, 8388608, (n, 2)).astype(np.int32)
        q[0] = (-8388608, 8388607)
        b = to_bytes(q)
        ref = q.astype(np.float32) * np.float32(2.0 ** -23)
        for offs in [(a, l, r) for a in (0, 1) for l in (0, 1) for r in (0, 1)]:
            gl, gr = _unpack24(b, offs)
            assert np.array_equal(gl.view(np.uint32), ref[:, 0].copy().view(np.uint32)), (n, offs)
            assert np.array_equal(gr.view(np.uint32), ref[:, 1].copy().view(np.uint32)), (n, offs)


@pytest.mark.gpu
@pytest.mark.parametrize("pairs", [1, 3, 5])
def test_pack_equals_the_rule_at_every_size_stride_and_alignment(pairs):
    rng = np.random.default_rng(240 + pairs)
    x, q, c = edge_list24()
    for count in COUNTS:
        v = (0.5 * rng.standard_normal((pairs, 2, count))).astype(np.float32)      # |x| >= 1 about once in 22 samples
        v.reshape(-1)[:min(v.size, x.size)] = x[:min(v.size, x.size)]              # the tie-and-edge list in front
        for stride in strides_of(count):
            for offs in ((0, 0), (1, 0), (0, 1), (1, 1)):
                a = _check_pack24(v, stride, stride, offs)
                if offs == (0, 0):
                    assert np.array_equal(a, _check_pack24(v, stride, stride, offs))      # two runs: the same counts (and the same bytes: both equal the rule)


@pytest.mark.gpu
def test_pack_and_unpack_past_the_grid_cap():
    rng = np.random.default_rng(77)
    x = (0.5 * rng.standard_normal((1, 2, BIG24))).astype(np.float32)
    x[0, 0, ::1000] = np.nan
    stride = (BIG24 + 7) // 8 * 8
    assert BIG24 > 8 * 256 * MAX_WGS
    clip = _check_pack24(x, stride, stride, (0, 0))                                # vector path, second trip of the grid-stride loop, a five-frame tail
    assert clip[0] > 100000
    b = to_bytes(rule24(x[0].T)[0])
    gl, gr = _unpack24(b, (0, 0, 0))
    ref = from_bytes(b).astype(np.float32) * np.float32(2.0 ** -23)
    assert np.array_equal(gl, ref[:, 0]) and np.array_equal(gr, ref[:, 1])


# ------------------------------------------------------------------------------------------------ GPU: the pipelines
N_RATE = 300000                                  # frames at 48 kHz: 275625 at 44.1 kHz, three pieces at max_tiles = 2
REFS = {}                                        # float outputs of the calls below on the signal below, computed once by whichever test asks first (read-only)
PATHS = ("stream", "overlap", "rate", "wiener", "wiener_overlap", "cli")


def signal24():
    """(q int32 [N_PIPE, 2] of 24-bit codes, L, R float32: the same samples) - noise and a tone, about -6 dBFS"""
    if "signal" not in REFS:
        rng = np.random.default_rng(2424)
        t = np.arange(N_PIPE) / 44100.0
        x = np.stack([0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.06 * rng.standard_normal(N_PIPE), 0.3 * np.sin(2 * np.pi * 554.0 * t + 1.0) + 0.06 * rng.standard_normal(N_PIPE)], 1)
        q = rule24(x.astype(np.float32))[0]
        f = q.astype(np.float32) * np.float32(2.0 ** -23)
        REFS["signal"] = (q, np.ascontiguousarray(f[:, 0]), np.ascontiguousarray(f[:, 1]))
    return REFS["signal"]


def run_path(e, path, src, **kw):
    """one call of each entry point that takes flags, on `src` ((L, R) or an integer array) -> (out, clipped)"""
    if path == "stream":
        return e.separate_host_stream_io(src, **kw)
    if path == "overlap":
        return e.separate_host_overlap(src, 16, **kw)
    if path == "rate":
        cut = (src[0][:N_RATE], src[1][:N_RATE]) if isinstance(src, tuple) else src[:N_RATE]
        return e.separate_host_rate(cut, 48000, 48000, **kw)
    if path == "wiener":
        return e.separate_host_wiener(src, **kw)
    if path == "wiener_overlap":
        return e.separate_host_wiener_overlap(src, 16, **kw)
    return e.separate_cli_host_io(src, 2, keep_staging=True, **kw)


def float_ref(e, path):
    """the float output of `path` on the signal (engine of max_tiles = 2)"""
    if path not in REFS:
        _, L, R = signal24()
        out, clipped = run_path(e, path, (L, R))
        assert out.dtype == np.float32 and not clipped.any()
        out.setflags(write=False)
        REFS[path] = out
    return REFS[path]


@pytest.fixture(scope="module")
def eng(coeffs):
    e = _engine(coeffs, 2)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True])
def test_stream_pcm24_output_is_the_rule_applied_to_the_float_output(eng, pinned):
    import torch
    q, L, R = signal24()
    ref = float_ref(eng, "stream")
    assert np.array_equal(ref, eng.separate_host_stream(L, R))                    # the Io call without flags is the float call
    want, wclip = as_pcm24(ref)
    if pinned:
        mk = lambda a: torch.from_numpy(a.copy()).pin_memory()
        src = (mk(L), mk(R))
        buf = torch.full(want.shape, SENT, dtype=torch.uint8).pin_memory()
    else:
        src = (L, R)
        buf = np.full(want.shape, SENT, np.uint8)                                # every byte must be overwritten
    out, clipped = eng.separate_host_stream_io(src, out_bits=24, out=buf, pinned=pinned)
    got = out.numpy() if pinned else out
    assert got.shape == (2, N_PIPE + 469 + 3072, 2, 3)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first mismatch (stem, sample, channel, byte) %s of %d" % (bad[0], len(bad))      # both chunk seams (131072, 262144) included
    assert clipped.tolist() == wclip
    # 24-bit in and out together
    b = to_bytes(q)
    bin_ = torch.from_numpy(b.copy()).pin_memory() if pinned else b
    both, clipped = eng.separate_host_stream_io(bin_, out_bits=24, pinned=pinned)
    assert np.array_equal(both, want) and clipped.tolist() == wclip


@pytest.mark.gpu
def test_stream_pcm24_input_equals_the_float_call_on_the_unpacked_samples(eng):
    q, L, R = signal24()
    ref = float_ref(eng, "stream")
    out, clipped = eng.separate_host_stream_io(to_bytes(q))
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)) and clipped.tolist() == [0, 0]
    # 24 bits in, 16 bits out: the formats of the two sides are independent
    import test_pcm16 as P16
    o16, c16 = eng.separate_host_stream_io(to_bytes(q), out_pcm16=True)
    w16, wc16 = P16._as_pcm(ref)
    assert np.array_equal(o16, w16) and c16.tolist() == wc16


@pytest.mark.gpu
def test_stream_pcm24_output_counts_clipped_samples_exactly(eng):
    q, L, R = signal24()
    mags = np.sort(np.abs(float_ref(eng, "stream")).reshape(-1))
    g = np.float32(1.0 / mags[-6000])                                             # about six thousand samples of the float output pass full scale
    Lg, Rg = L * g, R * g
    ref = eng.separate_host_stream(Lg, Rg)
    want, wclip = as_pcm24(ref)
    out, clipped = eng.separate_host_stream_io((Lg, Rg), out_bits=24)
    print("clipped per stem:", clipped.tolist(), "expected", wclip)
    assert np.array_equal(out, want)
    assert clipped.tolist() == wclip and sum(wclip) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS[1:])
def test_every_other_path_packs_its_own_float_output(eng, path):
    _, L, R = signal24()
    ref = float_ref(eng, path)
    want, wclip = as_pcm24(ref)
    out, clipped = run_path(eng, path, (L, R), out_bits=24)
    assert out.dtype == np.uint8 and out.shape == want.shape
    bad = np.argwhere(out != want)
    assert bad.size == 0, "%s: first mismatch (output, sample, channel, byte) %s of %d" % (path, bad[0], len(bad))
    assert clipped.tolist() == wclip
    if path in ("rate", "wiener"):                                              # ... and the 24-bit input in front of the spans kernel / the store
        q = signal24()[0]
        both, clipped = run_path(eng, path, to_bytes(q), out_bits=24)
        assert np.array_equal(both, want) and clipped.tolist() == wclip


@pytest.mark.gpu
def test_refusals_leave_the_output_alone(coeffs):
    e = _engine(coeffs, 2)
    lib = e.L
    n = 40 * 1024
    q = _signal(n, 31)
    x = q.astype(np.float32) / np.float32(32768)
    L, R = np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1])
    b24 = to_bytes(q.astype(np.int32) * 256)
    rows, frames = lib.srtStftRows(n), lib.srtStftFrames(n)
    out = np.full((2, lib.srtIstftLength(rows), 2, 3), SENT, np.uint8)
    clip = np.zeros(2, np.uint64)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    import spleeterrt_amd as srt
    wo = srt.capi._WienerOpts(1, 0, srt.MASK_EXT_CONSTANT, 0, None)
    in2 = lambda a: None if a is None else vp(a)
    calls = {
        "srtSeparateHostStreamIo": lambda a, a2, fl: lib.srtSeparateHostStreamIo(e.h, vp(a), in2(a2), n, frames, rows, vp(out), fl, vp(clip)),
        "srtSeparateCliHostIo": lambda a, a2, fl: lib.srtSeparateCliHostIo(e.h, vp(a), in2(a2), n, 2, vp(out), fl, vp(clip)),
        "srtSeparateHostStreamOverlap": lambda a, a2, fl: lib.srtSeparateHostStreamOverlap(e.h, vp(a), in2(a2), n, 8, vp(out), fl, vp(clip)),
        "srtSeparateHostStreamRate": lambda a, a2, fl: lib.srtSeparateHostStreamRate(e.h, vp(a), in2(a2), n, 44100, 44100, 0, vp(out), fl, vp(clip)),
        "srtSeparateHostWiener": lambda a, a2, fl: lib.srtSeparateHostWiener(e.h, vp(a), in2(a2), n, C.byref(wo), vp(out), fl, vp(clip)),
        "srtSeparateHostWienerOverlap": lambda a, a2, fl: lib.srtSeparateHostWienerOverlap(e.h, vp(a), in2(a2), n, C.byref(wo), vp(out), fl, vp(clip)),
    }
    try:
        for name, call in calls.items():
            for a, a2, fl, word in ((b24, None, IN16 | IN24, "in_pcm"), (L, R, OUT16 | OUT24, "out_pcm"), (L, R, DITHER, "dither"), (L, R, OUT24 | DITHER, "dither"),
                                    (L, R, OUT24 | 8, "flag"), (L, R, OUT24 | 128, "flag"), (L, R, 1 << 20, "flag"), (b24, R, IN24, "h_in2")):
                rc = call(a, a2, fl)
                text = lib.srtLastError().decode()
                assert rc == -1 and word in text.lower() and (name in text or name == "srtSeparateHostStreamIo" and "srtSeparateHostStream" in text), (name, fl, rc, text)
                assert (out == SENT).all() and not clip.any()
        assert calls["srtSeparateHostStreamIo"](b24, None, IN24 | OUT24) == 0, lib.srtLastError()
        first = out.copy()
        assert (first != SENT).any()
        e.release_staging()                                                       # frees the integer staging too; the next call allocates it again
        out[:] = SENT
        assert calls["srtSeparateHostStreamIo"](L, R, OUT24) == 0, lib.srtLastError()
        assert np.array_equal(out, first)                                         # (the 16-bit samples times 256 are the same floats)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ GPU: the CLI program
def cli_runs(tmp_path, oracle, runs):
    """the CLI program on one 16-bit input under each environment of `runs` {tag: env} -> ({tag: {name: (header fields, data bytes)}}, {tag: stdout}, frames)"""
    cli = _cli_path()
    np.concatenate([oracle.synth_coeff_fp16(1), oracle.synth_coeff_fp16(0)]).tofile(tmp_path / "weights.f16")
    n = 200000                                                                    # 204 rows with the pre-shift and padding: 4 tiles of 64, chunks of 2
    data = _signal(n, 47).astype("<i2").tobytes()
    with open(tmp_path / "in.wav", "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, 44100, 44100 * 4, 4, 16) + b"data" + struct.pack("<I", len(data)) + data)
    files, texts = {}, {}
    for tag, extra in runs.items():
        d = tmp_path / tag
        d.mkdir()
        env = {k: v for k, v in os.environ.items() if k not in ("SPLEETERRT_DEVICES", "SPLEETERRT_OUT_BITS", "SPLEETERRT_DITHER")}
        env.update(SPLEETERRT_BATCH_INVARIANT="1", SPLEETERRT_MAX_TILES="2", **extra)
        texts[tag] = subprocess.check_output([cli, "1", "64", "512", "3", str(tmp_path / "in.wav"), str(tmp_path / "weights.f16")], cwd=d, env=env).decode()
        files[tag] = {nm: _wav_fields(d / ("in.wav_%s.wav" % nm)) for nm in ("Drum", "Vocal", "Accompaniment")}
    return files, texts, n


@pytest.mark.gpu
def test_cli_program_writes_24_bit_files(tmp_path, oracle):
    files, texts, n = cli_runs(tmp_path, oracle, {"f32": {}, "i24": {"SPLEETERRT_OUT_BITS": "24"}})
    for nm in ("Drum", "Vocal", "Accompaniment"):
        h, body = files["f32"][nm]
        assert h["format"] == 3 and h["bits"] == 32 and h["data_bytes"] == n * 8
        h24, body24 = files["i24"][nm]
        assert h24 == {"riff": 36 + n * 6, "fmt_size": 16, "format": 1, "channels": 2, "rate": 44100, "byte_rate": 44100 * 6, "align": 6, "bits": 24,
                       "fact": False, "data_bytes": n * 6, "size": 44 + n * 6, "data_at": 44}, h24
        want, wc = rule24(np.frombuffer(body, "<f4"))
        assert np.array_equal(np.frombuffer(body24, np.uint8).reshape(-1, 3), to_bytes(want)), nm
        if wc.any():
            assert ("in.wav_%s.wav: " % nm) in texts["i24"] and "clipped sample" in texts["i24"]
