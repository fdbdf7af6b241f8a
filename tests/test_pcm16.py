"""16-bit PCM at the host-stream boundary: srtPcm16Unpack / srtPcm16Pack, the SRT_HOST_IN_PCM16 / SRT_HOST_OUT_PCM16 flags of
srtSeparateHostStreamIo / srtSeparateCliHostIo, and SPLEETERRT_OUT_BITS=16 of the CLI.

Every comparison is an exact integer or bit equality: the unpack (q / 32768) and the pack's product (x * 32768) are exact in fp32, the float path is
unchanged, and the rounding rule has one answer.  The rule in numpy (`rule` below, self-checked on the CPU against hand-written values):
    v = rint(float32(x) * float32(32768));  q = clip(v, -32768, 32767), NaN -> 0;  clipped = NaN or v outside [-32768, 32767].
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
SIZES = (1, 3, 4, 5, 255, 256, 257, 3079)
BIG = 2048 * 256 * 4 + 2853                  # past the grid cap of both kernels (2048 workgroups x 256 lanes x 4 frames): the grid-stride trips, ragged tail
IN16, OUT16 = 2, 4


def rule(x):
    """-> (int16 q, bool clipped) of float32 x"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(np.asarray(x, np.float32) * np.float32(32768))
        nan = np.isnan(v)
        clipped = nan | (v < -32768) | (v > 32767)
        q = np.clip(v, -32768, 32767)
        q[nan] = 0
        return q.astype(np.int16), clipped


def edge_list():
    """(x float32, expected q, expected clipped)"""
    f = np.float32
    rows = [
        (f(0.0), 0, 0), (f(-0.0), 0, 0),
        (f(0.5) / f(32768), 0, 0), (-f(0.5) / f(32768), 0, 0),                 # ties go to even
        (f(1.5) / f(32768), 2, 0), (-f(1.5) / f(32768), -2, 0),
        (f(2.5) / f(32768), 2, 0), (-f(2.5) / f(32768), -2, 0),
        (f(1.0), 32767, 1), (f(-1.0), -32768, 0),                               # +1 is 32768: clips; -1 is -32768: fits
        (f(1.0) - f(2.0) ** -16, 32767, 1), (f(2.0) ** -16 - f(1.0), -32768, 0),  # 32767.5 rounds to 32768 (even): clips; -32767.5 to -32768: fits
        (f(32767.5) / f(32768), 32767, 1), (f(32767.49) / f(32768), 32767, 0),
        (f(-32768.5) / f(32768), -32768, 0),                                    # the tie rounds to -32768 (even): inside the range
        (f(np.inf), 32767, 1), (f(-np.inf), -32768, 1), (f(np.nan), 0, 1),
        (np.frombuffer(struct.pack("<I", 1), np.float32)[0], 0, 0),             # smallest denormal
        (f(1e30), 32767, 1), (f(-1e30), -32768, 1),
    ]
    return (np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.int16), np.array([r[2] for r in rows], bool))


# ------------------------------------------------------------------------------------------------ CPU
def _lib():
    import spleeterrt_amd as srt
    return srt.load_library()


def test_symbols_exist():
    L = _lib()
    for sym in ("srtPcm16Unpack", "srtPcm16Pack", "srtSeparateHostStreamIo", "srtSeparateCliHostIo"):
        getattr(L, sym)
    import spleeterrt_amd as srt
    assert (srt.HOST_PINNED, srt.HOST_IN_PCM16, srt.HOST_OUT_PCM16) == (1, IN16, OUT16)
    assert callable(srt.pcm16_pack) and callable(srt.pcm16_unpack)
    assert hasattr(srt.Engine, "separate_host_stream_io") and hasattr(srt.Engine, "separate_cli_host_io")


def test_conversion_calls_refuse_bad_arguments_before_any_device_work():
    """no device here: a refusal that came after a HIP call could not return -1 with its own text"""
    L = _lib()
    p = C.c_void_p(4096)                                                      # never dereferenced: every case below is refused first
    bad = [
        L.srtPcm16Unpack(None, None, 8, p, p), L.srtPcm16Unpack(None, p, 8, None, p), L.srtPcm16Unpack(None, p, 8, p, None),
        L.srtPcm16Pack(None, None, 8, 1, 8, p, 8, None), L.srtPcm16Pack(None, p, 8, 1, 8, None, 8, None),
        L.srtPcm16Pack(None, p, 8, 0, 8, p, 8, None), L.srtPcm16Pack(None, p, 8, -1, 8, p, 8, None),
        L.srtPcm16Pack(None, p, 7, 1, 8, p, 8, None), L.srtPcm16Pack(None, p, 8, 1, 8, p, 7, None),
    ]
    assert bad == [-1] * len(bad)
    for call, word in ((lambda: L.srtPcm16Unpack(None, None, 8, p, p), b"null"), (lambda: L.srtPcm16Pack(None, p, 8, 0, 8, p, 8, None), b"pairs"),
                       (lambda: L.srtPcm16Pack(None, p, 7, 1, 8, p, 8, None), b"stride"), (lambda: L.srtPcm16Pack(None, p, 8, 1, 8, p, 7, None), b"stride")):
        assert call() == -1 and word in L.srtLastError()


def test_numpy_rule_on_the_tie_and_edge_list():
    x, q, c = edge_list()
    gq, gc = rule(x)
    assert np.array_equal(gq, q), (gq, q)
    assert np.array_equal(gc, c), (gc, c)
    every = np.arange(-32768, 32768).astype(np.int16)
    rq, rc = rule(every.astype(np.float32) / np.float32(32768))
    assert np.array_equal(rq, every) and not rc.any()


# ------------------------------------------------------------------------------------------------ GPU: the two kernels
GUARD = 8


def _unpack(q, off):
    """q int16 [n, 2] -> (L, R) through srtPcm16Unpack with every pointer `off` elements past a 256-byte aligned base; guard words checked"""
    import torch
    L = _lib()
    n = q.shape[0]
    src = torch.zeros(2 * n + 16, dtype=torch.int16, device="cuda")
    src[off:off + 2 * n] = torch.from_numpy(q.reshape(-1)).cuda()
    dst = torch.full((2, (n + 3) // 4 * 4 + 2 * GUARD + 16), -7.0, dtype=torch.float32, device="cuda")      # rows of whole 16-byte units: off = 0 is the vector path, tail included
    o = GUARD + off
    assert L.srtPcm16Unpack(None, C.c_void_p(src.data_ptr() + 2 * off), n, C.c_void_p(dst[0].data_ptr() + 4 * o), C.c_void_p(dst[1].data_ptr() + 4 * o)) == 0, L.srtLastError()
    d = dst.cpu().numpy()
    assert (d[:, :o] == -7.0).all() and (d[:, o + n:] == -7.0).all(), "guard words overwritten"
    return d[0, o:o + n], d[1, o:o + n]


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1])
def test_unpack_is_q_over_32768_bit_for_bit(off):
    every = np.arange(-32768, 32768).astype(np.int16).reshape(32768, 2)
    rng = np.random.default_rng(5)
    for q in [every] + [rng.integers(-32768, 32768, (n, 2)).astype(np.int16) for n in SIZES + (BIG,)]:
        gl, gr = _unpack(q, off)
        ref = q.astype(np.float32) / np.float32(32768)
        assert np.array_equal(gl.view(np.uint32), ref[:, 0].copy().view(np.uint32)), (q.shape, off)
        assert np.array_equal(gr.view(np.uint32), ref[:, 1].copy().view(np.uint32)), (q.shape, off)


def _pack(x, plane_stride, out_stride, off, start):
    """x float32 [pairs, 2, count] -> (int16 [pairs, count, 2], clipped [pairs]) through srtPcm16Pack with the given strides, the bases `off` elements past an
    aligned one and the counters starting at `start`; whatever lies between and around the outputs must keep its sentinel"""
    import torch
    L = _lib()
    pairs, _, count = x.shape
    planes = np.full((2 * pairs, plane_stride), np.nan, np.float32)                 # stride padding is NaN: reading it would show up in the counts
    planes[:, :count] = x.reshape(2 * pairs, count)
    src = torch.zeros(2 * pairs * plane_stride + 16, dtype=torch.float32, device="cuda")
    src[off:off + planes.size] = torch.from_numpy(planes.reshape(-1)).cuda()
    SENT = 0x5A5A
    dst = torch.full((2 * (pairs * out_stride + 2 * GUARD) + 16,), SENT, dtype=torch.int16, device="cuda")
    o = 2 * GUARD + off
    clip = torch.tensor(start, dtype=torch.int64, device="cuda")
    rc = L.srtPcm16Pack(None, C.c_void_p(src.data_ptr() + 4 * off), plane_stride, pairs, count, C.c_void_p(dst.data_ptr() + 2 * o), out_stride, C.c_void_p(clip.data_ptr()))
    assert rc == 0, L.srtLastError()
    d = dst.cpu().numpy()
    body = d[o:o + 2 * pairs * out_stride].reshape(pairs, out_stride, 2)
    assert (d[:o] == SENT).all() and (d[o + 2 * pairs * out_stride:] == SENT).all() and (body[:, count:] == SENT).all(), "wrote outside [0, count) of a pair"
    return body[:, :count].copy(), clip.cpu().numpy()


def _check_pack(x, plane_stride, out_stride, off):
    pairs = x.shape[0]
    start = [3 + 5 * p for p in range(pairs)]
    got, clip = _pack(x, plane_stride, out_stride, off, start)
    rq, rc = rule(x)                                                             # [pairs, 2, count]
    assert np.array_equal(got, rq.transpose(0, 2, 1)), (x.shape, plane_stride, out_stride, off)
    assert clip.tolist() == [start[p] + int(rc[p].sum()) for p in range(pairs)], (x.shape, plane_stride, out_stride, off)
    return got, clip


@pytest.mark.gpu
def test_pack_round_trip_of_every_value_and_the_edge_list():
    every = (np.arange(-32768, 32768).astype(np.float32) / np.float32(32768)).reshape(1, 32768, 2).transpose(0, 2, 1).copy()
    got, clip = _pack(every, 32768, 32768, 0, [0])
    assert np.array_equal(got.reshape(-1), np.arange(-32768, 32768).astype(np.int16)) and clip.tolist() == [0]
    x, q, c = edge_list()
    for off in (0, 1):
        for reps in (1, 4):                                                      # 21 values: frame-by-frame tail; 84: vector groups
            xe = np.stack([np.tile(x, reps), np.tile(x[::-1], reps)])[None]
            got, clip = _pack(xe, xe.shape[2], xe.shape[2], off, [0])
            assert np.array_equal(got[0, :, 0], np.tile(q, reps)) and np.array_equal(got[0, :, 1], np.tile(q[::-1], reps))
            assert clip.tolist() == [2 * reps * int(c.sum())]


@pytest.mark.gpu
@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("pad", ["equal", "aligned", "odd"])
@pytest.mark.parametrize("off", [0, 1])
def test_pack_equals_the_rule_at_every_size_stride_and_alignment(pairs, pad, off):
    rng = np.random.default_rng(100 * pairs + off)
    for count in SIZES:
        x = (0.5 * rng.standard_normal((pairs, 2, count))).astype(np.float32)      # |x| >= 1 about once in 22 samples
        stride = {"equal": count, "aligned": (count + 3) // 4 * 4 + 8, "odd": count + 3}[pad]
        a = _check_pack(x, stride, stride, off)
        b = _check_pack(x, stride, stride, off)                                     # two runs: the same bits, the same counts
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
def test_pack_past_the_grid_cap():
    rng = np.random.default_rng(77)
    x = (0.5 * rng.standard_normal((3, 2, BIG))).astype(np.float32)
    x[1, 0, ::1000] = np.nan
    _, clip = _check_pack(x, BIG + 3, BIG + 3, 0)                                   # BIG + 3 is a multiple of 4: vector path with a one-frame tail
    assert (BIG + 3) % 4 == 0 and min(clip.tolist()) > 100000
    _check_pack(x[:1], BIG, BIG, 1)                                                 # frame by frame


@pytest.mark.gpu
def test_python_tensor_functions():
    import torch
    import spleeterrt_amd as srt
    rng = np.random.default_rng(9)
    q = rng.integers(-32768, 32768, (1001, 2)).astype(np.int16)
    Lt, Rt = srt.pcm16_unpack(torch.from_numpy(q).cuda())
    assert np.array_equal(Lt.cpu().numpy(), q[:, 0] / np.float32(32768)) and np.array_equal(Rt.cpu().numpy(), q[:, 1] / np.float32(32768))
    x = (0.6 * rng.standard_normal((2, 2, 1001))).astype(np.float32)
    out, clip = srt.pcm16_pack(torch.from_numpy(x).cuda())
    rq, rc = rule(x)
    assert out.dtype == torch.int16 and np.array_equal(out.cpu().numpy(), rq.transpose(0, 2, 1))
    assert clip.cpu().tolist() == [int(rc[p].sum()) for p in range(2)] and min(clip.cpu().tolist()) > 0


# ------------------------------------------------------------------------------------------------ GPU: the pipeline
F, T = 512, 64
N_PIPE = 358 * 1024 - 469                  # 358 rows: chunks of 128, 128 and 102 rows at max_tiles = 2, a ragged last tile
N_CLI = 200 * 1024 - 123                   # two chunks


def _engine(coeffs, max_tiles):
    import spleeterrt_amd as srt
    e = srt.Engine(F=F, T=T, stem_modes=(1, 0), variant=srt.VARIANT_EXE, max_tiles=max_tiles, device="cuda:0")
    for s in range(2):
        e.set_coeff(s, coeffs(s))
    return e


def _signal(n, seed):
    """int16 [n, 2]: noise and a tone, about -6 dBFS"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    x = np.stack([0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.06 * rng.standard_normal(n), 0.3 * np.sin(2 * np.pi * 554.0 * t + 1.0) + 0.06 * rng.standard_normal(n)], 1)
    return rule(x.astype(np.float32))[0]


def _as_pcm(ref):
    """float stems [S, 2, len] -> (int16 [S, len, 2], clipped per stem) by the rule"""
    q, c = rule(ref)
    return np.ascontiguousarray(q.transpose(0, 2, 1)), [int(c[s].sum()) for s in range(ref.shape[0])]


@pytest.fixture(scope="module")
def pipe(coeffs):
    """the small engine, the 16-bit input, its float form and the float call's output on it (computed once, read-only)"""
    e = _engine(coeffs, 2)
    q = _signal(N_PIPE, 11)
    x = q.astype(np.float32) / np.float32(32768)
    L, R = np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1])
    ref = e.separate_host_stream(L, R)
    ref.setflags(write=False)
    yield {"e": e, "q": q, "L": L, "R": R, "ref": ref}
    e.close()


@pytest.mark.gpu
def test_stream_pcm16_input_equals_the_float_call(pipe):
    out, clipped = pipe["e"].separate_host_stream_io(pipe["q"])
    assert out.dtype == np.float32 and out.shape == pipe["ref"].shape
    assert np.array_equal(out.view(np.uint32), pipe["ref"].view(np.uint32)) and clipped.tolist() == [0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True])
def test_stream_pcm16_output_is_the_rule_applied_to_the_float_output(pipe, pinned):
    import torch
    want, wclip = _as_pcm(pipe["ref"])
    if pinned:
        mk = lambda a: torch.from_numpy(a.copy()).pin_memory()
        src = (mk(pipe["L"]), mk(pipe["R"]))
        buf = torch.full(want.shape, 0x5A5A, dtype=torch.int16).pin_memory()
    else:
        src = (pipe["L"], pipe["R"])
        buf = np.full(want.shape, 0x5A5A, np.int16)                            # every element must be overwritten
    out, clipped = pipe["e"].separate_host_stream_io(src, out_pcm16=True, out=buf, pinned=pinned)
    got = out.numpy() if pinned else out
    assert got.shape == (2, N_PIPE + 469 + 3072, 2)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first mismatch (stem, sample, channel) %s of %d" % (bad[0], len(bad))      # both chunk seams (131072, 262144) included
    assert clipped.tolist() == wclip
    # 16-bit in and out together: the 16-bit input call followed by the rule
    qin = torch.from_numpy(pipe["q"].copy()).pin_memory() if pinned else pipe["q"]
    both, clipped = pipe["e"].separate_host_stream_io(qin, out_pcm16=True, pinned=pinned)
    assert np.array_equal(both, want) and clipped.tolist() == wclip


@pytest.mark.gpu
def test_stream_pcm16_output_counts_clipped_samples_exactly(pipe):
    mags = np.sort(np.abs(pipe["ref"]).reshape(-1))
    g = np.float32(1.0 / mags[-6000])                                             # about six thousand samples of the float output pass full scale
    L, R = pipe["L"] * g, pipe["R"] * g
    ref = pipe["e"].separate_host_stream(L, R)
    want, wclip = _as_pcm(ref)
    out, clipped = pipe["e"].separate_host_stream_io((L, R), out_pcm16=True)
    print("clipped per stem:", clipped.tolist(), "expected", wclip)
    assert np.array_equal(out, want)
    assert clipped.tolist() == wclip and sum(wclip) > 0
    again, clipped2 = pipe["e"].separate_host_stream_io((L, R), out_pcm16=True)
    assert np.array_equal(again, out) and clipped2.tolist() == wclip


@pytest.mark.gpu
def test_stream_pcm16_output_at_another_chunk_size(pipe, coeffs):
    e3 = _engine(coeffs, 3)                                                       # chunks of 192 and 166 rows: held to ITS float call
    try:
        want, wclip = _as_pcm(e3.separate_host_stream(pipe["L"], pipe["R"]))
        out, clipped = e3.separate_host_stream_io(pipe["q"], out_pcm16=True)
        assert np.array_equal(out, want) and clipped.tolist() == wclip
    finally:
        e3.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stems", [2, 3])
def test_cli_flows_pcm16_output(pipe, stems):
    e = pipe["e"]
    q = _signal(N_CLI, 23)
    x = q.astype(np.float32) / np.float32(32768)
    L, R = np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1])
    ref = e.separate_cli_host(L, R, stems, keep_staging=True)
    want, wclip = _as_pcm(ref)
    out, clipped = e.separate_cli_host_io((L, R), stems, out_pcm16=True, keep_staging=True)
    assert out.shape == (stems, ref.shape[2], 2) and np.array_equal(out, want) and clipped.tolist() == wclip
    both, clipped = e.separate_cli_host_io(q, stems, out_pcm16=True, keep_staging=True)
    assert np.array_equal(both, want) and clipped.tolist() == wclip
    flt, clipped = e.separate_cli_host_io(q, stems, keep_staging=True)
    assert np.array_equal(flt.view(np.uint32), ref.view(np.uint32)) and clipped.tolist() == [0] * stems


@pytest.mark.gpu
def test_refusals_leave_the_output_alone(coeffs):
    e = _engine(coeffs, 2)
    lib = e.L
    n = 40 * 1024
    q = _signal(n, 31)
    x = q.astype(np.float32) / np.float32(32768)
    L, R = np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1])
    rows, frames = lib.srtStftRows(n), lib.srtStftFrames(n)
    out = np.full((2, lib.srtIstftLength(rows), 2), 0x5A5A, np.int16)
    clip = np.zeros(2, np.uint64)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def stream(h_in, h_in2, flags):
        return lib.srtSeparateHostStreamIo(e.h, vp(h_in), None if h_in2 is None else vp(h_in2), n, frames, rows, vp(out), flags, vp(clip))

    def cli(h_in, h_in2, flags):
        return lib.srtSeparateCliHostIo(e.h, vp(h_in), None if h_in2 is None else vp(h_in2), n, 2, vp(out), flags, vp(clip))

    def refused(rc, word):
        text = lib.srtLastError().decode()
        assert rc == -1 and word in text.lower(), (rc, text)
        assert (out == 0x5A5A).all()
    try:
        for call in (stream, cli):
            refused(call(q, None, IN16 | OUT16 | 8), "flag")                     # unknown bits
            refused(call(q, R, IN16 | OUT16), "h_in2")                            # an interleaved buffer and a second one
            e.set_overlap(8)
            refused(call(q, None, IN16 | OUT16), "overlap")
            e.set_overlap(0)
            e.set_wiener(1)
            refused(call(q, None, IN16 | OUT16), "wiener")
            e.set_wiener(0)
        assert stream(q, None, IN16 | OUT16) == 0, lib.srtLastError()
        first = out.copy()
        assert (first != 0x5A5A).any()
        e.release_staging()                                                       # frees the 16-bit staging too; the next call allocates it again
        out[:] = 0x5A5A
        assert stream(L, R, OUT16) == 0, lib.srtLastError()
        assert np.array_equal(out, first)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ GPU: the CLI program
def _wav_fields(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt "
    fsz = struct.unpack("<I", b[16:20])[0]
    fmt, ch, rate, brate, align, bits = struct.unpack("<HHIIHH", b[20:36])
    i = b.index(b"data", 20 + fsz)
    n = struct.unpack("<I", b[i + 4:i + 8])[0]
    return {"riff": struct.unpack("<I", b[4:8])[0], "fmt_size": fsz, "format": fmt, "channels": ch, "rate": rate, "byte_rate": brate, "align": align, "bits": bits,
            "fact": b.find(b"fact", 20 + fsz, i) >= 0, "data_bytes": n, "size": len(b), "data_at": i + 8}, b[i + 8:i + 8 + n]


@pytest.mark.gpu
def test_cli_program_writes_16_bit_files(tmp_path, oracle):
    cli = os.path.join(HOST, "spleeterrt_cli")
    subprocess.check_call(["make", "-s", "-C", HOST, "spleeterrt_cli"])
    np.concatenate([oracle.synth_coeff_fp16(1), oracle.synth_coeff_fp16(0)]).tofile(tmp_path / "weights.f16")
    n = 200000                                                                    # 204 rows with the pre-shift and padding: 4 tiles of 64, chunks of 2
    q = _signal(n, 47)
    data = q.astype("<i2").tobytes()
    with open(tmp_path / "in.wav", "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, 44100, 44100 * 4, 4, 16) + b"data" + struct.pack("<I", len(data)) + data)
    files, texts = {}, {}
    for tag, extra in (("f32", {}), ("f32x", {"SPLEETERRT_OUT_BITS": "32"}), ("i16", {"SPLEETERRT_OUT_BITS": "16"})):
        d = tmp_path / tag
        d.mkdir()
        env = dict(os.environ, SPLEETERRT_BATCH_INVARIANT="1", SPLEETERRT_MAX_TILES="2", **extra)
        env.pop("SPLEETERRT_DEVICES", None)
        texts[tag] = subprocess.check_output([cli, "1", "64", "512", "3", str(tmp_path / "in.wav"), str(tmp_path / "weights.f16")], cwd=d, env=env).decode()
        files[tag] = {nm: _wav_fields(d / ("in.wav_%s.wav" % nm)) for nm in ("Drum", "Vocal", "Accompaniment")}
    for nm in ("Drum", "Vocal", "Accompaniment"):
        h, body = files["f32"][nm]
        assert h == {"riff": 50 + n * 8, "fmt_size": 18, "format": 3, "channels": 2, "rate": 44100, "byte_rate": 44100 * 8, "align": 8, "bits": 32,
                     "fact": True, "data_bytes": n * 8, "size": 58 + n * 8, "data_at": 58}, h           # the float files as they have always been
        assert files["f32x"][nm] == files["f32"][nm]
        h16, body16 = files["i16"][nm]
        assert h16 == {"riff": 36 + n * 4, "fmt_size": 16, "format": 1, "channels": 2, "rate": 44100, "byte_rate": 44100 * 4, "align": 4, "bits": 16,
                       "fact": False, "data_bytes": n * 4, "size": 44 + n * 4, "data_at": 44}, h16
        want, wc = rule(np.frombuffer(body, "<f4"))
        assert np.array_equal(np.frombuffer(body16, "<i2"), want), nm
        if wc.any():
            assert ("in.wav_%s.wav: " % nm) in texts["i16"] and "clipped sample" in texts["i16"]
    # several workers: refused with a message, nothing written
    d = tmp_path / "multi"
    d.mkdir()
    r = subprocess.run([cli, "1", "64", "512", "3", str(tmp_path / "in.wav"), str(tmp_path / "weights.f16")], cwd=d, capture_output=True,
                       env=dict(os.environ, SPLEETERRT_OUT_BITS="16", SPLEETERRT_DEVICES="0,0"))
    assert r.returncode != 0 and b"single-engine" in r.stderr and not os.listdir(d)
