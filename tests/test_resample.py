"""Sample-rate conversion (csrc/srt_resample.hip, srtResample* in include/spleeterrt_amd.h, spleeterrt_amd.Resampler, the CLI's
$SPLEETERRT_RESAMPLE).  Pinned to the reference program's own converter (main.c:264-271 -> libsamplerate src_sinc.c) through
tests/golden/resample_reference.npz (tests/golden/gen_resample_golden.py): its 22 438-point table, seeded clips and their outputs."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "resample_reference.npz")


@pytest.fixture(scope="module")
def lib():
    from spleeterrt_amd import build as b
    b.build(verbose=False)
    import spleeterrt_amd
    return spleeterrt_amd.load_library()


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    cases = [(int(a), int(b), z["in%d" % k], z["out%d" % k], int(z["gen%d" % k])) for k, (a, b) in enumerate(z["rates"])]
    return z["table"], int(z["index_inc"]), cases


def restate(x, fs_in, fs_out, table, index_inc=491, frames=None):
    """The converter's arithmetic in numpy (float64 sums, like the reference): x [n, 2] float32 -> [len(frames), 2] float32."""
    n_in = x.shape[0]
    nout = int(math.ceil(n_in * (fs_out / float(fs_in))))
    r = fs_out / float(fs_in)
    fi = index_inc * min(r, 1.0)
    inc, mx = int(np.rint(fi * 4096)), (table.size - 2) << 12
    g = math.gcd(fs_in, fs_out)
    P, Q = fs_in // g, fs_out // g
    n = np.arange(nout, dtype=np.int64) if frames is None else np.asarray(frames, np.int64)
    pos = n * P
    i, frac = pos // Q, (pos % Q) / float(Q)
    start = np.rint(frac * fi * 4096).astype(np.int64)
    c = table.astype(np.float64)
    kk = np.arange(mx // inc + 1, dtype=np.int64)[None, :]

    def half(f, d):
        ok = (f >= 0) & (f <= mx)
        fk = np.where(ok, f, 0)
        k, fr = fk >> 12, (fk & 4095) / 4096.0
        w = np.where(ok, c[k] + fr * (c[k + 1] - c[k]), 0.0)
        inside = (d >= 0) & (d < n_in)
        xs = x[np.where(inside, d, 0)].astype(np.float64) * inside[..., None]
        return np.einsum("nk,nkc->nc", w, xs)
    left = half(start[:, None] + kk * inc, i[:, None] - kk)                     # src_sinc.c:375-394
    fr0 = (inc - start)[:, None] + kk * inc
    right = half(np.where(fr0 > 0, fr0, -1), i[:, None] + 1 + kk)              # :397-412 (index 0 is not a right-half tap)
    return ((fi / index_inc) * (left + right)).astype(np.float32)


def _rel_rms(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)) / (np.sqrt(np.mean(b.astype(np.float64) ** 2)) + 1e-30))


def _write_wav_f32(path, x, rate):
    x = np.ascontiguousarray(x, "<f4")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + x.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 2, rate, rate * 8, 8, 32))
        f.write(b"data" + struct.pack("<I", x.nbytes) + x.tobytes())


def _read_wav_f32(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE"
    rate = int.from_bytes(b[24:28], "little")
    i = b.index(b"data")
    n = int.from_bytes(b[i + 4:i + 8], "little")
    return np.frombuffer(b[i + 8:i + 8 + n], "<f4").reshape(-1, 2), rate


def _tones(n, fs, freqs, amp):
    t = np.arange(n) / fs
    x = np.zeros((n, 2))
    for k, f in enumerate(freqs):
        x[:, 0] += amp * np.sin(2 * np.pi * f * t + 0.3 * k)
        x[:, 1] += amp * np.sin(2 * np.pi * f * t + 1.1 * k + 0.5)
    return x.astype(np.float32)


# ---------------------------------------------------------------- CPU

def test_length_is_main_c_arithmetic(lib, golden):
    _, _, cases = golden
    rates = sorted({a for a, _, _, _, _ in cases} | {48000, 88200, 384000})
    for fs_in in rates:
        for fs_out in (44100, 48000, 8000, 384000):
            for n in (0, 1, 2, 3, 4095, 4096, 44100 * 60 + 7, 10 ** 9 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 5):
                assert lib.srtResampleLength(n, fs_in, fs_out) == int(math.ceil(n * (fs_out / float(fs_in)))), (n, fs_in, fs_out)
    for fs_in, fs_out, x, y, _ in cases:
        assert lib.srtResampleLength(x.shape[0], fs_in, fs_out) == y.shape[0]


def test_numpy_restatement_reproduces_reference(golden):
    """The arithmetic the kernel implements, restated in numpy, against libsamplerate's output (both directions, every fixture rate),
    on the frames the reference generated."""
    table, inc, cases = golden
    assert table.size == 22438 and inc == 491
    assert any(gen < y.shape[0] for _, _, _, y, gen in cases)          # the fixture does record the reference's short last frame
    for fs_in, fs_out, x, y, gen in cases:
        got = restate(x, fs_in, fs_out, table, inc)
        assert got.shape == y.shape
        peak = np.abs(y[:gen]).max()
        assert np.abs(got[:gen] - y[:gen]).max() <= 1e-6 * peak, (fs_in, fs_out)


def test_create_checks_arguments_before_any_hip_call(lib):
    import torch
    h = C.c_void_p()
    tab = np.ones(100, np.float32)
    for args, msg in (((4000, 44100, None, 0, 0), b"8000..384000"), ((44100, 400000, None, 0, 0), b"8000..384000"),
                      ((48000, 44100, tab.ctypes.data, 1, 491), b"table_len"), ((48000, 44100, tab.ctypes.data, 100, 0), b"index_inc")):
        assert lib.srtResamplerCreate(*args, None, C.byref(h)) < 0, args
        assert msg in lib.srtLastError(), (args, lib.srtLastError())
    assert lib.srtResamplerCreate(48000, 44100, None, 0, 0, None, None) < 0 and b"null" in lib.srtLastError()
    assert lib.srtResample(None, None, None, 0, 0, 1, None, None) < 0 and b"null" in lib.srtLastError()
    assert lib.srtResampleHost(None, None, None, 0, None, None) < 0
    assert lib.srtResamplerDestroy(None) == 0
    if torch.cuda.is_available():
        pytest.skip("GPU present: a valid create succeeds here")
    assert lib.srtResamplerCreate(48000, 44100, None, 0, 0, None, C.byref(h)) < 0 and b"no HIP device" in lib.srtLastError()


def test_cli_rate_gate_with_resampling_switch(tmp_path):
    """$SPLEETERRT_RESAMPLE=1 lets a 48 kHz file through the rate gate (it then fails at the weights, before any GPU work); bogus
    values and rates outside 8000..384000 Hz are refused with their own messages."""
    cli = os.path.join(HOST, "spleeterrt_cli")
    subprocess.check_call(["make", "-s", "-C", HOST, "spleeterrt_cli"])
    env = {k: v for k, v in os.environ.items() if k not in ("SPLEETERRT_WEIGHTS", "SPLEETERRT_RESAMPLE")}
    w = tmp_path / "w.f16"
    w.write_bytes(b"")
    wav48, wav4 = tmp_path / "a48.wav", tmp_path / "a4.wav"
    _write_wav_f32(wav48, np.zeros((100, 2), np.float32), 48000)
    _write_wav_f32(wav4, np.zeros((100, 2), np.float32), 4000)
    run = lambda wav, **e: subprocess.run([cli, "1", "64", "512", "2", str(wav), str(w)], capture_output=True, env=dict(env, **e))
    r = run(wav48)
    assert r.returncode != 0 and b"only 44.1 kHz" in r.stderr and b"SPLEETERRT_RESAMPLE" in r.stderr
    r = run(wav48, SPLEETERRT_RESAMPLE="0")
    assert r.returncode != 0 and b"only 44.1 kHz" in r.stderr
    for mode in ("1", "source"):
        r = run(wav48, SPLEETERRT_RESAMPLE=mode)
        assert r.returncode != 0 and b"cannot read" in r.stderr and b"only 44.1 kHz" not in r.stderr, r.stderr
    r = run(wav48, SPLEETERRT_RESAMPLE="yes")
    assert r.returncode != 0 and b"expected 0, 1 or source" in r.stderr
    r = run(wav4, SPLEETERRT_RESAMPLE="1")
    assert r.returncode != 0 and b"8000..384000" in r.stderr and b"cannot read" not in r.stderr


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_reference_cases_on_gpu(golden):
    """Every fixture case through the kernel with the reference's table: libsamplerate's output on the frames it generated."""
    import torch
    import spleeterrt_amd as srt
    table, inc, cases = golden
    for fs_in, fs_out, x, y, gen in cases:
        rs = srt.Resampler(fs_in, fs_out, table=table, index_inc=inc)
        Lo, Ro = rs.resample(torch.from_numpy(x[:, 0].copy()).cuda(), torch.from_numpy(x[:, 1].copy()).cuda())
        got = np.stack([Lo.cpu().numpy(), Ro.cpu().numpy()], 1)
        assert got.shape == y.shape
        peak = np.abs(y[:gen]).max()
        d = np.abs(got[:gen] - y[:gen]).max()
        rel = _rel_rms(got[:gen], y[:gen])
        print("%6d -> %6d Hz: max-abs/peak %.2e rel-RMS %.2e bit-identical %.4f" % (fs_in, fs_out, d / peak, rel, np.mean(got[:gen] == y[:gen])))
        assert d <= 1e-5 * peak and rel <= 2e-6, (fs_in, fs_out, d / peak, rel)
        # the last frame the reference leaves at 0 is computed here: equal to the restatement
        if gen < y.shape[0]:
            tail = restate(x, fs_in, fs_out, table, inc, frames=np.arange(gen, y.shape[0]))
            assert np.abs(got[gen:] - tail).max() <= 1e-5 * peak
        host = rs.resample_host(x[:, 0], x[:, 1])
        assert np.array_equal(host[0], got[:, 0]) and np.array_equal(host[1], got[:, 1])
        rs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fs_in,fs_out", [(48000, 44100), (96000, 44100), (44100, 48000), (22050, 44100), (8000, 44100), (44056, 44100), (192000, 44100)])
def test_any_partition_gives_the_same_bits(fs_in, fs_out):
    """A frame depends on its index only: one frame at a time, 7 uneven chunks and chunks that start at 0 / end at n_out all equal one
    call, bit for bit; mono (d_R == d_L, d_Ro == d_Lo) equals the stereo call on L; the on-the-fly weights equal the bank's."""
    import torch
    import spleeterrt_amd as srt
    rng = np.random.default_rng(fs_in + fs_out)
    n = 20011
    x = (0.5 * rng.standard_normal((2, n))).astype(np.float32)
    L, R = torch.from_numpy(x[0]).cuda(), torch.from_numpy(x[1]).cuda()
    rs = srt.Resampler(fs_in, fs_out)
    m = rs.length(n)
    Lf, Rf = rs.resample(L, R)
    Lf, Rf = Lf.cpu().numpy(), Rf.cpu().numpy()
    assert np.all(np.isfinite(Lf)) and np.abs(Lf).max() > 0
    for f in (0, 1, m // 3, m - 1):
        a, b = rs.resample(L, R, out0=f, n_out=1)
        assert a.item() == Lf[f] and b.item() == Rf[f], f
    cuts = np.sort(rng.choice(np.arange(1, m), 6, replace=False))
    bounds = [0] + cuts.tolist() + [m]
    Lc, Rc = np.empty(m, np.float32), np.empty(m, np.float32)
    for a, b in zip(bounds[:-1], bounds[1:]):
        lo, ro = rs.resample(L, R, out0=a, n_out=b - a)
        Lc[a:b], Rc[a:b] = lo.cpu().numpy(), ro.cpu().numpy()
    assert np.array_equal(Lc, Lf) and np.array_equal(Rc, Rf)
    for a, b in ((0, 777), (0, m - 5), (5, m), (m - 1000, m)):
        lo, ro = rs.resample(L, R, out0=a, n_out=b - a)
        assert np.array_equal(lo.cpu().numpy(), Lf[a:b]) and np.array_equal(ro.cpu().numpy(), Rf[a:b]), (a, b)
    mono = torch.empty(m, device="cuda", dtype=torch.float32)
    rs.resample(L, L, Lo=mono, Ro=mono)
    LL, _ = rs.resample(L, L.clone())
    assert np.array_equal(mono.cpu().numpy(), Lf) and np.array_equal(LL.cpu().numpy(), Lf)
    rs.close()
    os.environ["SPLEETERRT_RESAMPLE_ONFLY"] = "1"
    try:
        fly = srt.Resampler(fs_in, fs_out)
    finally:
        del os.environ["SPLEETERRT_RESAMPLE_ONFLY"]
    a, b = fly.resample(L, R)
    assert np.array_equal(a.cpu().numpy(), Lf) and np.array_equal(b.cpu().numpy(), Rf)
    a, b = fly.resample(L, R, out0=m // 2, n_out=m - m // 2)
    assert np.array_equal(a.cpu().numpy(), Lf[m // 2:])
    fly.close()


@pytest.mark.gpu
def test_ten_minute_stream_past_32_bit_positions(golden):
    """10 minutes of 48 kHz stereo: n * fs_in passes 2^32 after ~1.5 minutes.  4096 random output frames against the restatement."""
    import torch
    import spleeterrt_amd as srt
    table, inc, _ = golden
    n = 48000 * 600 + 17
    rng = np.random.default_rng(600)
    x = _tones(n, 48000, (311.0, 4400.0, 15100.0), 0.2)
    x += (0.1 * rng.standard_normal((n, 2))).astype(np.float32)
    rs = srt.Resampler(48000, 44100, table=table, index_inc=inc)
    m = rs.length(n)
    assert (m - 1) * 48000 > 2 ** 40
    Lo, Ro = rs.resample(torch.from_numpy(x[:, 0].copy()).cuda(), torch.from_numpy(x[:, 1].copy()).cuda())
    frames = np.concatenate([rng.choice(m, 4090, replace=False), [0, 1, m - 2, m - 1, (2 ** 32) // 48000, (2 ** 32) // 48000 + 1]])
    got = np.stack([Lo.cpu().numpy()[frames], Ro.cpu().numpy()[frames]], 1)
    ref = restate(x, 48000, 44100, table, inc, frames=frames)
    peak = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-5 * peak and _rel_rms(got, ref) <= 2e-6
    rs.close()


@pytest.mark.gpu
def test_builtin_filter_quality():
    """The built-in filter at 48 k -> 44.1 k: flat passband, deep stopband, close to the reference's filter below 16 kHz, and a
    48 k -> 44.1 k -> 48 k round trip that returns the input."""
    import spleeterrt_amd as srt
    z = np.load(GOLDEN)
    n = 24000
    down = srt.Resampler(48000, 44100)
    mid = slice(600, -600)
    for f in (100.0, 1000.0, 5000.0, 10000.0, 15000.0, 17000.0):
        y, _ = down.resample_host(*_tones(n, 48000, (f,), 1.0).T)
        k = np.arange(y.size)[mid]
        A = np.stack([np.sin(2 * np.pi * f * k / 44100), np.cos(2 * np.pi * f * k / 44100)], 1)
        gain = 20 * np.log10(np.hypot(*np.linalg.lstsq(A, y[mid].astype(np.float64), rcond=None)[0]))
        assert abs(gain) <= 1e-3, (f, gain)
    for f in (22500.0, 23000.0, 23500.0):
        y, _ = down.resample_host(*_tones(n, 48000, (f,), 1.0).T)
        level = 20 * np.log10(np.sqrt(np.mean(y[mid].astype(np.float64) ** 2)) / np.sqrt(0.5) + 1e-30)
        assert level <= -100.0, (f, level)
    rng = np.random.default_rng(16)
    x = _tones(n, 48000, rng.uniform(50.0, 16000.0, 24), 0.05)
    ref = srt.Resampler(48000, 44100, table=z["table"], index_inc=491)
    a = np.stack(down.resample_host(x[:, 0], x[:, 1]), 1)[mid]
    b = np.stack(ref.resample_host(x[:, 0], x[:, 1]), 1)[mid]
    assert _rel_rms(a, b) <= 1e-4, _rel_rms(a, b)
    up = srt.Resampler(44100, 48000)
    x = _tones(n, 48000, (440.0, 3000.0, 9000.0, 14000.0, 18000.0), 0.15)
    y = down.resample_host(x[:, 0], x[:, 1])
    back = np.stack(up.resample_host(*y), 1)[:n]
    assert _rel_rms(back[mid], x[mid]) <= 1e-4, _rel_rms(back[mid], x[mid])
    for r in (down, ref, up):
        r.close()


@pytest.mark.gpu
def test_cli_resamples_on_the_gpu(tmp_path, oracle):
    """SPLEETERRT_RESAMPLE=1 on a 48 kHz clip writes 44.1 kHz stems of srtResampleLength frames, bit-identical to the 44.1 kHz run on the
    clip Resampler.resample_host converted; =source writes the input's rate and frame count, equal to those stems converted back."""
    import spleeterrt_amd as srt
    cli = os.path.join(HOST, "spleeterrt_cli")
    subprocess.check_call(["make", "-s", "-C", HOST, "spleeterrt_cli"])
    np.concatenate([oracle.synth_coeff_fp16(1), oracle.synth_coeff_fp16(0)]).tofile(tmp_path / "weights.f16")
    n = 48000 * 3 + 101
    L, R = oracle.synth_audio(n, 4848, True)
    x = np.stack([L, R], 1).astype(np.float32)
    _write_wav_f32(tmp_path / "clip.wav", x, 48000)
    down = srt.Resampler(48000, 44100)
    x44 = np.stack(down.resample_host(x[:, 0], x[:, 1]), 1)
    n44 = down.length(n)
    assert x44.shape == (n44, 2)
    _write_wav_f32(tmp_path / "conv.wav", x44, 44100)
    env = {k: v for k, v in os.environ.items() if k not in ("SPLEETERRT_RESAMPLE", "SPLEETERRT_WEIGHTS")}
    runs = {"one": ("clip.wav", "1"), "plain": ("conv.wav", "0"), "source": ("clip.wav", "source")}
    for tag, (wav, mode) in runs.items():
        d = tmp_path / tag
        d.mkdir()
        subprocess.check_call([cli, "1", "64", "512", "2", str(tmp_path / wav), str(tmp_path / "weights.f16")], cwd=d,
                              env=dict(env, SPLEETERRT_RESAMPLE=mode), stdout=subprocess.DEVNULL)
    up = srt.Resampler(44100, 48000)
    for nm in ("Vocal", "Accompaniment"):
        one, r1 = _read_wav_f32(tmp_path / "one" / ("clip.wav_%s.wav" % nm))
        plain, r2 = _read_wav_f32(tmp_path / "plain" / ("conv.wav_%s.wav" % nm))
        src, r3 = _read_wav_f32(tmp_path / "source" / ("clip.wav_%s.wav" % nm))
        assert r1 == r2 == 44100 and r3 == 48000
        assert one.shape == (n44, 2) and src.shape == (n, 2)
        assert np.abs(one).max() > 0
        assert np.array_equal(one, plain), nm
        back = np.stack(up.resample_host(one[:, 0].copy(), one[:, 1].copy()), 1)[:n]
        assert np.array_equal(src, back), nm
    down.close()
    up.close()
