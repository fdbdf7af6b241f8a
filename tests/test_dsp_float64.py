"""The offline STFT / iSTFT kernels (csrc/srt_dsp.hip: srt_stft_kernel, srt_istft_ola3_kernel for F <= 1024, srt_istft_ola_kernel for F > 1024)
against a float64 numpy restatement of the reference's transforms, frame by frame and hop by hop.

The restatement (stft64 / istft_frames64 / gains) uses the oracle's own fp32 window tables cast to float64 - the tables are part of the specification.
Norms:
  forward, per frame f:     E(f) = max_k |got - ref| / max_k |ref_f|  (and the same ratio in l2), for the spectrum and for the magnitudes
  inverse, per (stem, output hop s): E(s) = max over the hop's 1024 samples of |got - ref|, over the largest max_p |H_f[p] post[p]| of the frames
                            f in [s - 3, s] that contribute to it (float64)
A frame / a hop is both channels' (the maxima run over L and R): the kernels transform z = L + iR in ONE complex FFT and separate the two spectra
afterwards, so the rounding of a channel is relative to the larger of the two in that frame - a channel far below the other one carries the other one's
rounding.  The same ratio per channel over the channel's OWN scale is printed next to it ("/ch") and not asserted: on the staircased signal, whose channels
differ by up to 60 dB within a frame, it reaches 25 x e_cpu for the forward kernel (5.6e-6 of the quiet channel's peak; 44 x in l2) and 74 x e_cpu for the
inverse kernels (1.3e-5), in every launch regime and with no pattern in the frame index modulo fpb or G: the level ratio times the fp32 rounding, not a
wrong frame, hop or bin.  The oracle, which transforms each channel alone, holds
its 1e-6 per channel as well, and the CPU tests assert that.  So that a fault confined to one channel of a frame has no louder channel to hide under, the
"matched" cases (the same staircase in both channels, R at half the gain) assert the per-channel ratio too, against the same bound times the worst level
ratio of the case, measured on the float64 reference (report, per_channel).
The hop norm divides by a WINDOWED scale, while the rounding of an fp32 transform follows the frame's unwindowed peak.  A frame whose content sits where the
synthesis window vanishes (an impulse at sample 0 or 4095 of the frame and nothing else: frame 4 of the 37-row impulse signal, in the channel that holds
sample 4096) has a windowed peak of 1e-7 of its unwindowed one, and a hop made of such a frame alone measures the fp32 oracle itself at 9.5e-6.  A large E
on such a hop is the norm's corner, not a kernel fault (e_cpu rises with it); no GPU case of the inverse has such a frame, and the CPU check of the inverse
on impulses uses a 7-row impulse signal for that reason.
A NaN or an infinity anywhere in a device result fails the case: results are checked for finiteness first, and a NaN in an error is kept by every merge.
Bound: every frame and hop of the GPU result within 4 x e_cpu, e_cpu = the WORST E of the fp32 CPU oracle on the same input in the same norm (computed
here, from the reference alone).  Both are fp32 evaluations of the same 4096-point transform in different factorisations; the oracle's own error scatters by
about 2x across signal kinds (0.87e-7 .. 1.7e-7), hence 4.  The three-per-CU inverse kernel rebuilds the synthesis window from two registers instead of
reading the table, so its bound gets the derived term 4 x delta_w (four frames overlap in a sample; ola3_window_delta).  The older 2e-6 x global peak against
the oracle stays asserted as an outer cap.  Where the float64 reference of a frame / hop is exactly zero (silence of >= 4 hops in both channels, rows the
reference leaves calloc'ed) the GPU result must be exactly zero.

The CPU tests hold the restatement to oracle.stft / oracle.istft at 1e-6 of each frame's / hop's own scale (the tolerance tests/test_oracle.py uses between
the oracle and the real reference), and show on perturbed restatements (one hop, one sample, one bin, swapped channels, re + im at bin 2048, the mask at
k = F) that the norms see the errors they are meant for."""
import functools
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

FFT, HOP, HALF, SPEC_LD = 4096, 1024, 2049, 2052
MARGIN = 4.0                 # E_gpu <= MARGIN * e_cpu (reasoned above, not measured)
CAP = 2e-6                   # outer cap: max |got - oracle| <= CAP * the oracle result's global peak
RESTATE_TOL = 1e-6           # restatement vs oracle, per frame / hop
CHUNK = 128                  # frames / hops handled at a time (keeps the float64 intermediates of the long cases small)


# ---------------------------------------------------------------- float64 restatement
@functools.lru_cache(maxsize=None)
def tables64():
    """(pre, post): the oracle's fp32 analysis / synthesis windows (stftFix.c:302-313), as float64"""
    from oracle import pyoracle as O
    t = O.tables()
    return (np.ctypeslib.as_array(t.pre).astype(np.float64), np.ctypeslib.as_array(t.post).astype(np.float64))


def stft_rows(n):
    return -(-n // HOP)


def stft_nfull(n):
    """the last row the reference computes (stftFix.c: rangeM / 1024 whole frames and one zero-padded tail frame); rows above it stay zero"""
    return (n - FFT + HOP // 4) // HOP


def stft64(L, R, f0=0, f1=None, shift=0, bin_shift=0, swap=False):
    """rows [f0, f1) of the forward transform: (re, im), each float64 [2][f1 - f0][2049].
    shift / bin_shift / swap perturb it for the negative controls (frame start in samples, bins rolled, channels swapped)."""
    pre, _ = tables64()
    n = L.size
    rows, nfull = stft_rows(n), stft_nfull(n)
    f1 = rows if f1 is None else f1
    re = np.zeros((2, f1 - f0, HALF))
    im = np.zeros((2, f1 - f0, HALF))
    fc = min(f1, nfull + 1)                                # rows [f0, fc) are computed
    if fc > f0:
        a, b = f0 * HOP + shift, (fc - 1) * HOP + shift + FFT                     # the samples these frames see, zero padded past n (stftFix.c:460-472)
        x = np.zeros((2, b - a))
        x[0, :max(min(b, n) - a, 0)] = (R if swap else L)[a:b]
        x[1, :max(min(b, n) - a, 0)] = (L if swap else R)[a:b]
        fr = np.lib.stride_tricks.sliding_window_view(x, FFT, axis=1)[:, ::HOP]
        X = np.fft.rfft(fr * pre, axis=-1)
        re[:, :fc - f0] = 2.0 * X.real
        im[:, :fc - f0] = -2.0 * X.imag
        im[:, :, 0] = 0.0
        im[:, :, 2048] = 0.0
    if bin_shift:
        re, im = np.roll(re, bin_shift, axis=-1), np.roll(im, bin_shift, axis=-1)
    return re, im


def mag64(re, im, F):
    """magnitude rows [2][rows][F] (main.c:462-471)"""
    return 4096.0 * np.hypot(re[..., :F], im[..., :F])


def mag_rows(mag):
    """tile layout [ntiles][2][T][F] -> rows [2][ntiles * T][F]"""
    nt, _, T, F = mag.shape
    return mag.transpose(1, 0, 2, 3).reshape(2, nt * T, F)


def gains(mask_rows, oob, nrows, F, dtype=np.float64, edge_at_f=False):
    """the gain of every bin of rows: the mask below F, the stem's out-of-band weight from F on (main.c:473-494).  mask_rows: [2][nrows][F] or None (all ones).
    oob: the stem's scalar weight (rounded to fp32, as the engine holds it), or [2][nrows] gains per (channel, row).
    edge_at_f: the negative control that lets the mask reach bin F."""
    if np.ndim(oob) == 0:
        g = np.full((2, nrows, HALF), np.float32(oob), dtype)
    else:                                                  # one gain per (channel, row), taken as it is: a row of the average extension's table, or a chain over such rows
        g = np.empty((2, nrows, HALF), dtype)
        g[...] = np.asarray(oob).reshape(2, nrows, 1)
    g[:, :, :F] = 1.0 if mask_rows is None else mask_rows
    if edge_at_f and F < HALF:
        g[:, :, F] = g[:, :, F - 1]
    return g


def istft_frames64(re, im, plus_at_2048=False):
    """the windowed inverse frames H_f[p] post[p], float64 [...][4096], from the reference's Hartley packing (stftFix.c:554-576).
    plus_at_2048: the negative control that packs re + im at bin 2048."""
    _, post = tables64()
    a = np.empty(re.shape[:-1] + (FFT,))
    a[..., 0] = re[..., 0]
    a[..., 1:2048] = re[..., 1:2048] + im[..., 1:2048]
    a[..., 2048] = re[..., 2048] + im[..., 2048] if plus_at_2048 else re[..., 2048] - im[..., 2048]
    a[..., 2049:] = (re[..., 1:2048] - im[..., 1:2048])[..., ::-1]
    A = np.fft.rfft(a, axis=-1)                            # a is real: fft(a)[4096 - p] = conj(fft(a)[p])
    H = np.empty_like(a)
    H[..., :2049] = A.real - A.imag
    H[..., 2049:] = (A.real + A.imag)[..., 1:2048][..., ::-1]
    return H * post


def overlap_add64(hf):
    """[...][nf][4096] -> output hops [...][nf + 3][1024] and each hop's scale [...][nf + 3] (largest frame peak among the frames f in [s - 3, s])"""
    nf = hf.shape[-2]
    segs = np.zeros(hf.shape[:-2] + (nf + 3, HOP))
    scale = np.zeros(hf.shape[:-2] + (nf + 3,))
    peak = np.abs(hf).max(axis=-1)
    for q in range(4):
        segs[..., q:q + nf, :] += hf[..., q * HOP:(q + 1) * HOP]
        scale[..., q:q + nf] = np.maximum(scale[..., q:q + nf], peak)
    return segs, scale


def ola3_window_delta():
    """delta_w of srt_istft_ola3_kernel: its synthesis-window taps, restated in float32, against the post table; + 2^-24 for the device sincospif's couple
    of ulp on values <= 1.  The kernel forms tap tid + 256 k2 as fmaf(-wc3, cos(k2 pi/8), fmaf(ws3, sin(k2 pi/8), 1/3)) with ws3 / wc3 the sine / cosine of
    2 pi (tid + 1/2) / 4096, correctly rounded, times float(1/3)."""
    _, post = tables64()
    f32 = np.float32
    tid = np.arange(256)
    th = 2.0 * np.pi * (tid + 0.5) / FFT
    third = f32(1.0 / 3.0)
    ws3 = (np.sin(th).astype(f32) * third).astype(f32).astype(np.float64)
    wc3 = (np.cos(th).astype(f32) * third).astype(f32).astype(np.float64)
    k2 = np.arange(16)
    c8 = np.cos(k2 * np.pi / 8).astype(f32).astype(np.float64)
    s8 = np.sin(k2 * np.pi / 8).astype(f32).astype(np.float64)
    inner = (ws3[None, :] * s8[:, None] + np.float64(third)).astype(f32).astype(np.float64)     # a product of two floats is exact in float64: one rounding, as fmaf
    w32 = (-wc3[None, :] * c8[:, None] + inner).astype(f32).astype(np.float64)                  # [k2][tid] = tap tid + 256 k2
    return float(np.abs(w32.reshape(-1) - post).max()) + 2.0 ** -24


# ---------------------------------------------------------------- signals (deterministic, non-periodic, a scale that differs from frame to frame)
def hop_gains(nhops, irr, silent_from=None):
    """a 60 dB staircase 10^(-3 u_h), u_h = frac(h * irr) for an irrational irr: not monotone, repeats with no period; five silent hops from silent_from"""
    g = 10.0 ** (-3.0 * ((np.arange(nhops) * irr) % 1.0))
    if silent_from is not None:
        g[silent_from:silent_from + 5] = 0.0
    return g


GOLD, ROOT2 = 0.6180339887498949, 0.41421356237309515
SILENT_HOP = 11              # hops 11..15 of the staircased signals are silent: frames 11 and 12 lie inside


def _staircased(L, R, matched=False):
    """matched: the SAME sequence in both channels, R half as loud - the channels of a frame stay within a small factor of each other (report, per_channel)"""
    n = L.size
    gl = np.repeat(hop_gains(stft_rows(n), GOLD, SILENT_HOP), HOP)[:n]
    gr = np.repeat(0.5 * hop_gains(stft_rows(n), GOLD if matched else ROOT2, SILENT_HOP), HOP)[:n]       # another sequence and another level: a channel swap shows
    return (L * gl).astype(np.float32), (R * gr).astype(np.float32)


@functools.lru_cache(maxsize=4)
def signal(kind, n):
    from oracle import pyoracle as O
    if kind in ("staircase", "matched"):
        L, R = O.synth_audio(n, 777, True)
        return _staircased(L.astype(np.float64), R.astype(np.float64), kind == "matched")
    if kind == "impulses":
        L, R = np.zeros(n, np.float32), np.zeros(n, np.float32)
        for pos, v in ((0, 1.0), (1024, -0.5), (4095, 0.25), (n - 1, 0.75)):
            L[pos] = v
        for pos, v in ((1023, -1.0), (4096, 0.5), (n - 1, -0.25)):
            R[pos] = v
        return L, R
    if kind == "tones":
        t = np.arange(n, dtype=np.float64)
        w = 2.0 * np.pi / FFT
        L = 0.3 * np.sin(w * 1.0 * t) + 0.2 * np.sin(w * 1023.5 * t + 0.3)
        R = 0.3 * np.sin(w * 2047.0 * t + 0.1) + 0.2 * np.sin(w * 1.5 * t)
        return _staircased(L, R)
    raise KeyError(kind)


def signal_rows(kind, rows):
    """a signal of `rows` spectrum rows whose zero-padded tail frame is computed (and holds sample n - 1)"""
    return signal(kind, (rows - 1) * HOP + 900)


ZERO_ROW = 7                 # rows 7..11 of the inverse tests' spectra are zero: output hops 10 and 11 are silent


def spectrum_input(rows, seed, matched=False):
    """an arbitrary complex spectrum, NOT the transform of a signal (non-zero imaginary parts at bins 0 and 2048): float32 [2][rows][2052][2], seeded
    normal values under a per-row staircase (its own sequence per channel) with five zero rows"""
    rng = np.random.default_rng(seed)
    spec = np.zeros((2, rows, SPEC_LD, 2), np.float32)
    spec[:, :, :HALF, :] = rng.standard_normal((2, rows, HALF, 2), dtype=np.float32)
    z = ZERO_ROW if rows >= ZERO_ROW + 6 else None
    spec[0] *= hop_gains(rows, ROOT2, z).astype(np.float32)[:, None, None]
    spec[1] *= ((0.5 if matched else 0.25) * hop_gains(rows, ROOT2 if matched else GOLD, z)).astype(np.float32)[:, None, None]     # matched: as _staircased
    return spec


def mask_input(S, ntiles, T, F, seed):
    """seeded masks in [0, 1), independent at every (stem, tile, channel, row, bin)"""
    return np.random.default_rng(seed).random((S, ntiles, 2, T, F), dtype=np.float32)


# ---------------------------------------------------------------- the launchers' rules at HEAD, restated for the printed report only
def launcher_fpb(rows):
    if rows >= 4096:
        rounds = -(-rows // (768 * 24))
        return -(-rows // (768 * rounds))
    return 2 if rows >= 1024 else 1


def launcher_G(frames, S, F):
    nseg = frames + 3
    runs = max((1024 if F > 1024 else 768) // S, 1)
    return max(-(-nseg // runs), 13 if nseg * S >= 4096 else 5)


# ---------------------------------------------------------------- forward: errors per frame
ALL_NAMES = ("spec max", "spec l2", "mag max", "mag l2")       # asserted: per frame over both channels
CH_NAMES = ("spec max/ch", "mag max/ch")                        # reported: per (channel, frame) over the channel's own scale
class Worst:
    """the worst value of a per-row error and where it is"""

    def __init__(self):
        self.v, self.at = 0.0, None

    def take(self, err, base=0, prefix=()):
        """a NaN anywhere in err becomes the worst value and stays it (every comparison against a bound then fails)"""
        if err.size and not np.isnan(self.v):
            i = np.unravel_index(int(np.argmax(err)), err.shape)                 # (argmax returns the first NaN's index)
            if self.at is None or np.isnan(err[i]) or err[i] > self.v:
                self.v, self.at = float(err[i]), tuple(prefix) + tuple(int(j) for j in i[:-1]) + (int(i[-1]) + base,)


def _row_errors(got, ref):
    """got, ref [2 channels][rows][K].  Per row, over BOTH channels: the max and the l2 error over the row's own scale, and which rows are silent (reference
    all zero: the error there must be exactly zero and reports 0); then the max error of each channel over that CHANNEL's own scale (reported, not asserted:
    see the module docstring), and each (channel, row)'s largest absolute error."""
    d = got - ref
    dmax, smax = np.abs(d).max(axis=-1), np.abs(ref).max(axis=-1)                # [2][rows]
    dsq, ssq = (d ** 2).sum(axis=-1), (ref ** 2).sum(axis=-1)
    silent = smax.max(axis=0) == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        emax = np.where(silent, 0.0, dmax.max(axis=0) / smax.max(axis=0))
        el2 = np.where(silent, 0.0, np.sqrt(dsq.sum(axis=0) / ssq.sum(axis=0)))
        ech = np.where(smax == 0, 0.0, dmax / smax)
        lvl = np.where(smax == 0, 0.0, smax.max(axis=0) / smax)                  # how far each channel's scale is below the row's
    return emax, el2, ech, silent, dmax, lvl


def _worse(u, v):
    """max that keeps a NaN (Python's max(u, nan) keeps u)"""
    return float("nan") if np.isnan(u) or np.isnan(v) else max(u, v)


def _chunks(total, tail):
    """[a, b) pieces of CHUNK; the last one keeps at least `tail` items"""
    starts = list(range(0, total, CHUNK))
    if len(starts) > 1 and total - starts[-1] < tail:
        starts.pop()
    return [(a, starts[i + 1] if i + 1 < len(starts) else total) for i, a in enumerate(starts)]


def _run(piece, items):
    """the pieces of a long case on a few threads (numpy releases the interpreter lock; the oracle's own loops are OpenMP-parallel already, so two workers
    are enough to keep the numpy part of one piece under the oracle part of another); results are merged under a lock, in any order"""
    if len(items) <= 2:
        for it in items:
            piece(it)
        return
    with ThreadPoolExecutor(max_workers=2) as pool:
        list(pool.map(piece, items))


def stft_case(oracle, L, R, F, spec=None, mag=None, **perturb):
    """Errors of the fp32 oracle (and, when given, of a device result: spec [2][rows][2052][2], mag [ntiles][2][T][F]) against stft64 on (L, R), per
    frame (and, for the report, per channel and frame).  Returns {"cpu": {name: Worst}, "gpu": {...}, "silent": rows whose reference is zero, "cap": (max |got - oracle|, oracle peak)}.
    A device result that is not exactly zero where the reference is raises at once."""
    n = L.size
    rows, nfull = stft_rows(n), stft_nfull(n)
    names = ALL_NAMES + CH_NAMES
    res = {"cpu": {k: Worst() for k in names}, "gpu": {k: Worst() for k in names}, "silent": 0, "cap": [0.0, 0.0, 0.0, 0.0], "rows": rows, "nfull": nfull, "level": 0.0}
    gmag = mag_rows(mag) if mag is not None else None
    if spec is not None:
        assert spec.shape == (2, rows, SPEC_LD, 2)
        assert np.isfinite(spec).all(), "spectrum not finite, first at %r" % (tuple(np.argwhere(~np.isfinite(spec))[0]),)
        assert np.all(spec[:, :, HALF:, :] == 0), "spectrum columns 2049..2051 must be zero"
    if gmag is not None:
        assert np.isfinite(gmag).all(), "magnitudes not finite, first at (channel, row, bin) %r" % (tuple(np.argwhere(~np.isfinite(gmag))[0]),)
        assert gmag.shape[1] >= rows and np.all(gmag[:, rows:] == 0), "magnitude rows of the tail tile past the signal's rows must be zero"
    lock = threading.Lock()

    def piece(span):
        f0, f1 = span
        re, im = stft64(L, R, f0, f1, **perturb)
        ref = np.concatenate([re, im], axis=-1)                                  # a frame's error is taken over re and im together
        rmag = mag64(re, im, F)
        # the oracle on the samples these frames see: to the end of the signal for the last piece (its tail rule), else up to the last frame's last sample
        end = n if f1 == rows else (f1 - 1) * HOP + FFT
        ore, oim = oracle.stft(L[f0 * HOP:end], R[f0 * HOP:end])
        ore, oim = ore[:, :f1 - f0], oim[:, :f1 - f0]
        omag = oracle.magnitude_tile(ore, oim, 0, f1 - f0, F)
        sets = [("cpu", np.concatenate([ore[..., :HALF], oim[..., :HALF]], axis=-1), omag)]
        cap = [0.0, float(np.abs(ore).max()), 0.0, float(np.abs(omag).max())]
        if spec is not None:
            g = spec[:, f0:f1]
            sets.append(("gpu", np.concatenate([g[:, :, :HALF, 0], g[:, :, :HALF, 1]], axis=-1), gmag[:, f0:f1] if gmag is not None else None))
            cap[0] = float(np.abs(sets[1][1] - sets[0][1]).max())
            if gmag is not None:
                cap[2] = float(np.abs(sets[1][2] - omag).max())
        errs = []
        for who, x, m in sets:
            emax, el2, ech, silent, dmax, lvl = _row_errors(x, ref)
            if who == "gpu":
                assert np.all(dmax[:, silent] == 0), "spectrum rows %s are not exactly zero where the reference is" % (np.flatnonzero(silent & (dmax.max(axis=0) > 0))[:4] + f0).tolist()
            errs += [(who, "spec max", emax), (who, "spec l2", el2), (who, "spec max/ch", ech)]
            if m is not None:
                emax, el2, ech, msilent, dmax, mlvl = _row_errors(m, rmag)
                lvl = np.maximum(lvl, mlvl)
                if who == "gpu":
                    assert np.all(dmax[:, msilent] == 0), "magnitude rows %s are not exactly zero where the reference is" % (np.flatnonzero(msilent & (dmax.max(axis=0) > 0))[:4] + f0).tolist()
                errs += [(who, "mag max", emax), (who, "mag l2", el2), (who, "mag max/ch", ech)]
        with lock:
            for who, k, e in errs:
                res[who][k].take(e, f0)
            res["cap"] = [_worse(u, v) for u, v in zip(res["cap"], cap)]
            res["silent"] += int(silent.sum())
            res["level"] = max(res["level"], float(lvl.max()))
    _run(piece, _chunks(rows, 16))
    return res


MATCHED_LEVEL = 6.0          # the matched-level cases keep every channel's scale within this factor of its frame's / hop's, checked on the reference
                             # (R at half of L's gain, and spectral peaks of the two channels' different content up to ~3 x apart: measured 5.1 / 3.0)


def report(tag, res, names, extra=0.0, period=None, per_channel=False):
    """print E_gpu, e_cpu and their ratio per norm; assert E_gpu <= MARGIN * e_cpu + extra over every row (the worst row stands for all of them; a NaN fails).
    The per-channel figures ("/ch") are printed; per_channel asserts them too, for the matched-level cases: the packed transform's rounding is relative to
    the frame's larger channel, so a channel whose scale is `level` times below it may show `level` times the error over its own scale - the bound is
    level x (MARGIN * e_cpu + extra) with level the worst such ratio of the case, measured on the float64 reference and at most MATCHED_LEVEL."""
    bad = []
    chs = tuple(k for k in res["gpu"] if k not in names and k.endswith("/ch"))
    level = res["level"]
    if per_channel:
        print("%s | a channel's scale is at most %.2f x below its frame's / hop's" % (tag, level))
        assert 1.0 <= level <= MATCHED_LEVEL, tag
    for k in tuple(names) + chs:
        g, c = res["gpu"][k], res["cpu"][k]
        ratio = g.v / c.v if c.v > 0 else (0.0 if g.v == 0 else float("inf"))
        where = "" if g.at is None else " worst at %r" % (g.at,) + (" (index mod %d = %d)" % (period, g.at[-1] % period) if period else "")
        asserted = k in names or per_channel
        print("%s | %-11s E_gpu %.3g  e_cpu %.3g  ratio %.2f%s%s" % (tag, k, g.v, c.v, ratio, where, "" if asserted else " (reported, not asserted)"))
        bound = (MARGIN * c.v + extra) * (level if k in chs else 1.0)
        if asserted and not g.v <= bound:
            bad.append("%s: E_gpu %.3g > bound %.3g (e_cpu %.3g)%s" % (k, g.v, bound, c.v, where))
    assert not bad, tag + ": " + "; ".join(bad)


# ---------------------------------------------------------------- inverse: errors per (stem, output hop)
HOP_NAMES, HOP_CH_NAMES = ("hop max",), ("hop max/ch",)


def _hop_errors(x, segs, scale):
    """x, segs [2][hops][1024], scale [2][hops]: per hop over both channels, the largest error over the hop's scale (the larger channel's); the same per
    channel over that channel's own scale; the silent hops where x is not exactly zero; and the largest ratio of a hop's scale to a channel's"""
    d = np.abs(x - segs).max(axis=-1)
    silent = scale.max(axis=0) == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(silent, 0.0, d.max(axis=0) / scale.max(axis=0))
        ech = np.where(scale == 0, 0.0, d / scale)
        lvl = np.where(scale == 0, 0.0, scale.max(axis=0) / scale)
    return e, ech, np.flatnonzero(silent & ~(d.max(axis=0) == 0)), float(lvl.max())


def _oob_rows(o, c0, c1):
    """an out-of-band gain for frames [c0, c1): the scalar as it is, or those columns of a [2][rows] array"""
    return o if np.ndim(o) == 0 else np.asarray(o)[:, c0:c1]


def istft_case(oracle, spec, masks, oob, T, F, got=None, masks64=None, chain=None, oob64=None, seam_hops=None, **perturb):
    """Errors of the fp32 oracle (and of a device result got [S][2][(rows + 3) * 1024]) against the float64 inverse of spec [2][rows][2052][2] under
    masks [S][ntiles][2][T][F] (None: all ones) and the out-of-band weights, per (stem, output hop).  The oracle multiplies in fp32, as the
    reference does (main.c:473-494); the float64 side uses masks64 where given (the ratio test), else the same masks.
    oob: per stem a scalar weight or a [2][rows] array of gains per (channel, row) (gains); oob64: the float64 side's, where it differs (else oob).
    seam_hops: output hops whose frames a chunked path adds in another association than one pass does (tests/test_dsp_float64_forms.py).  The device's
    error on those hops - and on no other - is reduced by the derived term 3 x 2^-24 x (sum of the peaks of frames s - 3 .. s) / scale(s) before it is merged
    (three fp32 additions in any order; from the float64 reference alone); res["seam"] lists (stem, hop, error before the reduction, term).
    chain = (L, R) instead of spec (the round trip): the float64 side inverts stft64 of the signal, the oracle its own stft of it.
    perturb: edge_at_f (gains), plus_at_2048 (istft_frames64) for the negative controls."""
    rows = stft_rows(chain[0].size) if chain is not None else spec.shape[1]
    S, nseg = len(oob), rows + 3
    names = HOP_NAMES + HOP_CH_NAMES
    res = {"cpu": {k: Worst() for k in names}, "gpu": {k: Worst() for k in names}, "silent": 0, "cap": [0.0, 0.0], "level": 0.0, "seam": []}
    edge = {k: v for k, v in perturb.items() if k == "edge_at_f"}
    pack = {k: v for k, v in perturb.items() if k == "plus_at_2048"}
    if got is not None:
        assert got.shape == (S, 2, nseg * HOP)
        assert np.isfinite(got).all(), "output not finite, first at (stem, channel, sample) %r" % (tuple(np.argwhere(~np.isfinite(got))[0]),)
    if chain is None:
        sre, sim = spec[:, :, :HALF, 0], spec[:, :, :HALF, 1]
    lock = threading.Lock()
    m32s = [mag_rows(masks[s]) if masks is not None else None for s in range(S)]            # [2][ntiles * T][F] per stem
    m64s = [mag_rows(masks64[s]) if masks64 is not None else None for s in range(S)]

    def piece(item):
        s, s0, s1 = item
        m32, m64 = m32s[s], m64s[s]
        c0, c1 = max(s0 - 3, 0), min(s1, rows)                                   # the frames these hops are made of
        g32 = gains(None if m32 is None else m32[:, c0:c1], _oob_rows(oob[s], c0, c1), c1 - c0, F, np.float32)
        g64 = gains(m64[:, c0:c1] if m64 is not None else None if m32 is None else m32[:, c0:c1], _oob_rows((oob if oob64 is None else oob64)[s], c0, c1), c1 - c0, F, **edge)
        ore = np.zeros((2, c1 - c0, FFT), np.float32)
        oim = np.zeros((2, c1 - c0, FFT), np.float32)
        if chain is not None:
            L, R = chain
            re, im = stft64(L, R, c0, c1)
            end = L.size if c1 == rows else (c1 - 1) * HOP + FFT                 # (as in stft_case)
            cre, cim = oracle.stft(L[c0 * HOP:end], R[c0 * HOP:end])
            cre, cim = cre[:, :c1 - c0, :HALF], cim[:, :c1 - c0, :HALF]
        else:
            cre, cim = sre[:, c0:c1], sim[:, c0:c1]
            re, im = cre.astype(np.float64), cim.astype(np.float64)
        hf = istft_frames64(re * g64, im * g64, **pack)
        segs, scale = overlap_add64(hf)                                          # hops c0 .. c1 + 3 (the first three partial unless c0 = 0)
        lo, hi = s0 - c0, s1 - c0
        segs, scale = segs[:, lo:hi], scale[:, lo:hi]
        term = np.zeros(s1 - s0)
        if seam_hops is not None:
            psum, peak = np.zeros(c1 - c0 + 3), np.abs(hf).max(axis=-1).max(axis=0)
            for q in range(4):
                psum[q:q + c1 - c0] += peak
            at = np.array([h - s0 for h in seam_hops if s0 <= h < s1 and scale[:, h - s0].max() > 0], int)
            term[at] = 3.0 * 2.0 ** -24 * psum[lo:hi][at] / scale.max(axis=0)[at]
        ore[:, :, :HALF] = cre * g32
        oim[:, :, :HALF] = cim * g32
        o = oracle.istft(ore, oim).reshape(2, c1 - c0 + 3, HOP)[:, lo:hi]        # frames are added in frame order: the hops from s0 on are complete
        silent = scale.max(axis=0) == 0                                          # hops made of zero frames alone, in both channels
        cap = [0.0, float(np.abs(o).max())]
        sets = [("cpu", o)]
        if got is not None:
            g = got[s].reshape(2, nseg, HOP)[:, s0:s1]
            sets.append(("gpu", g))
            cap[0] = float(np.abs(g - o).max())
        errs = []
        for who, x in sets:
            e, ech, bad, lvl = _hop_errors(x, segs, scale)
            assert who == "cpu" or not bad.size, "stem %d: output hops %s are not exactly zero where the reference is" % (s, (bad[:4] + s0).tolist())
            if who == "gpu" and seam_hops is not None:
                seam = [(s, int(h) + s0, float(e[h]), float(term[h])) for h in np.flatnonzero(term)]
                e = e - term
            errs += [(who, "hop max", e), (who, "hop max/ch", ech)]
        with lock:
            for who, k, e in errs:
                res[who][k].take(e, s0, (s,))                                    # (stem, [channel,] hop)
            res["cap"] = [_worse(u, v) for u, v in zip(res["cap"], cap)]
            res["silent"] += int(silent.sum()) if s == 0 else 0
            res["level"] = max(res["level"], lvl)
            if got is not None and seam_hops is not None:
                res["seam"] += seam
    _run(piece, [(s, s0, s1) for s in range(S) for s0, s1 in _chunks(nseg, 4)])
    return res


def check_cap(tag, res, pairs=((0, 1),)):
    for a, b in pairs:
        print("%s | max |got - oracle| %.3g = %.3g of the oracle's peak %.3g" % (tag, res["cap"][a], res["cap"][a] / res["cap"][b] if res["cap"][b] else 0.0, res["cap"][b]))
        assert res["cap"][a] <= CAP * res["cap"][b], tag                         # (false for a NaN as well)


# ================================================================ A. the restatement against the oracle (CPU)


@pytest.mark.parametrize("kind", ["staircase", "impulses", "tones"])
def test_restatement_forward_matches_oracle(oracle, kind):
    L, R = signal_rows(kind, 37)
    res = stft_case(oracle, L, R, 1024)
    for k in ALL_NAMES + CH_NAMES:                        # (the oracle transforms each channel on its own: it holds the bound per channel as well)
        print("forward %s | %-11s oracle vs float64 %.3g at %r" % (kind, k, res["cpu"][k].v, res["cpu"][k].at))
        assert 0 < res["cpu"][k].v <= RESTATE_TOL, (kind, k, res["cpu"][k].v, res["cpu"][k].at)
    assert res["nfull"] == 33 and res["rows"] == 37
    assert res["silent"] >= (2 if kind != "impulses" else 20)                    # frames 11 and 12 (impulses: every frame between the head and the tail)


@pytest.mark.parametrize("kind", ["staircase", "impulses", "tones", "spectrum"])
def test_restatement_inverse_matches_oracle(oracle, kind):
    if kind == "spectrum":
        spec = spectrum_input(37, 5)
        assert np.all(spec[:, :ZERO_ROW, (0, 2048), 1] != 0)                      # imaginary parts no forward transform produces
        masks, oob, F, T = mask_input(2, 2, 32, 576, 6), (1.0, 0.0), 576, 32
    else:
        # (impulses: 7 rows.  At 37 rows the frame that starts at 4096 is computed and holds, in one channel, nothing but the sample at its position 0, where the
        # synthesis window is 1e-7 of its peak: the hop made of that frame alone has a windowed scale of 1e-7 of the frame's unwindowed peak, while the rounding of
        # any fp32 transform is relative to the unwindowed peak - the oracle itself is 9.5e-6 off there in this norm.  The 7-row signal has every listed position
        # and no such frame.)
        L, R = signal(kind, 7000) if kind == "impulses" else signal_rows(kind, 37)
        ore, oim = oracle.stft(L, R)
        spec = np.zeros((2, ore.shape[1], SPEC_LD, 2), np.float32)
        spec[:, :, :HALF, 0], spec[:, :, :HALF, 1] = ore[:, :, :HALF], oim[:, :, :HALF]
        masks, oob, F, T = None, (1.0, 0.25), 1024, 64
    res = istft_case(oracle, spec, masks, oob, T, F)
    for k in HOP_NAMES + HOP_CH_NAMES:
        w = res["cpu"][k]
        print("inverse %s | %-10s oracle vs float64 %.3g at (stem, [channel,] hop) %r; %d silent hops" % (kind, k, w.v, w.at, res["silent"]))
        assert 0 < w.v <= RESTATE_TOL, (kind, k, w.v, w.at)
    assert res["silent"] >= (2 if kind in ("impulses", "spectrum") else 0)       # (two zero frames of a staircased signal do not make a silent hop)


def test_ola3_window_delta():
    d = ola3_window_delta()
    print("delta_w = %.3g (of which 2^-24 = %.3g for the device sincospif)" % (d, 2.0 ** -24))
    assert 2.0 ** -24 < d < 2.0 ** -24 + 1.2e-7              # two fp32 roundings of values <= 2/3 and the table's own rounding: a few 1e-8


@pytest.mark.parametrize("name,perturb", [("one hop", dict(shift=HOP)), ("one sample", dict(shift=1)), ("one bin", dict(bin_shift=1)), ("channels swapped", dict(swap=True))])
def test_forward_norms_see_a_perturbed_restatement(oracle, name, perturb):
    """negative control: the restatement off by one hop / sample / bin, or with L and R swapped, is far outside the bound it passes unperturbed"""
    L, R = signal_rows("staircase", 21)
    res = stft_case(oracle, L, R, 1024, **perturb)
    print("forward, %s | oracle vs perturbed float64: %s" % (name, ", ".join("%s %.3g" % (k, res["cpu"][k].v) for k in ALL_NAMES)))
    for k in ALL_NAMES:
        assert res["cpu"][k].v > 1e3 * RESTATE_TOL, (name, k)


@pytest.mark.parametrize("name,perturb", [("re + im at bin 2048", dict(plus_at_2048=True)), ("mask applied at k = F", dict(edge_at_f=True))])
def test_inverse_norm_sees_a_perturbed_restatement(oracle, name, perturb):
    """negative control: the two quirks the mask prologue must get right - perturbed, the restatement leaves the bound by orders of magnitude"""
    spec = spectrum_input(21, 5)
    res = istft_case(oracle, spec, mask_input(1, 1, 32, 576, 6), (0.25,), 32, 576, **perturb)
    w = res["cpu"]["hop max"]
    print("inverse, %s | oracle vs perturbed float64 %.3g at %r" % (name, w.v, w.at))
    assert w.v > 1e3 * RESTATE_TOL


def _as_device_spec(ore, oim):
    spec = np.zeros((2, ore.shape[1], SPEC_LD, 2), np.float32)
    spec[:, :, :HALF, 0], spec[:, :, :HALF, 1] = ore[:, :, :HALF], oim[:, :, :HALF]
    return spec


def test_a_nan_in_a_late_piece_fails_the_checks(oracle):
    """negative control: a "device" result equal to the oracle's except for one NaN in a late piece (row 200 of 300, CHUNK = 128) is refused at the door,
    and - with the door taken away - the NaN still reaches report and check_cap through Worst.take and the cap merge, whatever piece is merged first"""
    L, R = signal_rows("staircase", 300)
    ore, oim = oracle.stft(L, R)
    spec = _as_device_spec(ore, oim)
    mag = np.stack([oracle.magnitude_tile(ore, oim, t * 64, 64, 1024) for t in range(5)])
    good = stft_case(oracle, L, R, 1024, spec, mag)
    report("control", good, ALL_NAMES)
    check_cap("control", good, ((0, 1), (2, 3)))
    bad_spec = spec.copy()
    bad_spec[1, 200, 77, 0] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        stft_case(oracle, L, R, 1024, bad_spec, mag)
    out = np.stack([oracle.istft(ore, oim)])
    bad_out = out.copy()
    bad_out[0, 1, 200 * HOP + 5] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        istft_case(oracle, spec, None, (1.0,), 64, 1024, bad_out)
    # behind the door: the merges themselves
    for first in (0.0, 3e-7):
        w = Worst()
        w.take(np.array([[first, 1e-7]]), 0)
        w.take(np.array([[1e-7, np.nan]]), 128)
        w.take(np.array([[5e-7, 2e-7]]), 256)
        assert np.isnan(w.v) and w.at == (0, 129)
        res = {"gpu": {"spec max": w}, "cpu": {"spec max": good["cpu"]["spec max"]}, "level": 1.0}
        with pytest.raises(AssertionError):
            report("control", res, ("spec max",))
    assert np.isnan(_worse(1.0, float("nan"))) and np.isnan(_worse(float("nan"), 1.0)) and _worse(1.0, 2.0) == 2.0 and _worse(2.0, 1.0) == 2.0
    with pytest.raises(AssertionError):
        check_cap("control", {"cap": [float("nan"), 1.0]})


def test_launcher_rules_put_the_shapes_in_their_regimes():
    """The shapes of the GPU cases were chosen for the launchers' rules at HEAD.  This checks only the Python restatement above (launcher_fpb / launcher_G, used
    for the printed tags and the "index mod" hints) against those shapes: the engine does not expose fpb or G, so nothing here reads srt_launch_stft /
    srt_launch_istft.  Whoever changes either rule edits the restatement by hand and moves the shapes."""
    assert [launcher_fpb(r) for r in (37, 1025, 4099, 9000)] == [1, 2, 6, 12]
    assert 1025 % 2 == 1 and 4099 % 6 == 1                                       # the last workgroup holds one frame
    assert [launcher_G(f, 1, 1024) for f in (1, 4, 13, 17)] == [5, 5, 5, 5] and sorted((f + 3) % 5 for f in range(13, 18)) == [0, 1, 2, 3, 4]
    assert launcher_G(1400, 3, 1024) == 13 and launcher_G(2100, 5, 1024) == 14 and launcher_G(4500, 3, 1088) == 14
    assert -(-2103 // 14) * 5 == 755 and 1403 * 3 >= 4096


# ================================================================ GPU
def _engine(**kw):
    import spleeterrt_amd as srt
    return srt.Engine(**kw)


def _gpu_stft(L, R, T, F, want_mag=True):
    import torch
    rows = stft_rows(L.size)
    eng = _engine(F=F, T=T, stem_modes=(1,), max_tiles=-(-rows // T))
    spec, mag = eng.stft(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), want_mag=want_mag)
    spec = spec.cpu().numpy()
    mag = mag.cpu().numpy() if want_mag else None
    eng.close()
    return spec, mag


def _forward_check(oracle, tag, L, R, T, F, min_silent=0, per_channel=False):
    spec, mag = _gpu_stft(L, R, T, F)
    res = stft_case(oracle, L, R, F, spec, mag)
    fpb = launcher_fpb(res["rows"])
    tag = "stft %s rows %d (computed 0..%d) T %d F %d fpb %d" % (tag, res["rows"], res["nfull"], T, F, fpb)
    assert np.all(spec[:, res["nfull"] + 1:] == 0) and np.all(mag_rows(mag)[:, res["nfull"] + 1:] == 0), tag + ": rows the reference leaves zero"
    assert res["silent"] >= min_silent, tag
    report(tag, res, ALL_NAMES, period=fpb, per_channel=per_channel)
    check_cap(tag, res, ((0, 1), (2, 3)))
    return res


# ---- D. forward
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [37, 1025, 4099, 9000])
def test_stft_regimes(oracle, rows):
    """fpb = 1 / 2 (last workgroup: one frame) / 6 (last workgroup: one frame) / 12: every row of a staircased signal"""
    L, R = signal_rows("staircase", rows)
    _forward_check(oracle, "staircase", L, R, 256, 1024, min_silent=2)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [0, 1, 255, 256, 767, 768, 769, 1023])
def test_stft_tail_rule(oracle, r):
    """both sides of the + HOP/4 in rangeM: the computed rows, the zero-padded last frame, and the rows the reference leaves zero"""
    n = 8 * HOP + r
    L, R = signal("staircase", n)
    res = _forward_check(oracle, "tail r=%d" % r, L, R, 256, 1024)
    assert res["nfull"] == (4 if r < 768 else 5) and res["rows"] == (8 if r == 0 else 9)


@pytest.mark.gpu
@pytest.mark.parametrize("T,F", [(64, 64), (64, 576), (128, 1024), (64, 2048)])
def test_stft_magnitude_layout(oracle, T, F):
    """the [ntiles][2][T][F] magnitude tiles at other (T, F), rows not a multiple of T; F = 2048 keeps bin 2048 out of band"""
    L, R = signal_rows("staircase", 2 * T + 17)
    _forward_check(oracle, "layout", L, R, T, F, min_silent=2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["impulses", "tones"])
def test_stft_impulses_and_tones(oracle, kind):
    L, R = signal_rows(kind, 37)
    _forward_check(oracle, kind, L, R, 256, 1024, min_silent=2)


@pytest.mark.gpu
def test_stft_per_channel_at_matched_levels(oracle):
    """the same staircase in both channels, R at half the gain: each CHANNEL of each frame over its own scale as well (fpb = 2), so that a fault confined to one
    channel of a frame shows without a louder channel to hide under; the bound is report's, scaled by the level ratio measured on the reference"""
    L, R = signal_rows("matched", 1025)
    _forward_check(oracle, "matched", L, R, 256, 1024, min_silent=2, per_channel=True)


# ---- E. inverse
OOB = (1.0, 0.0, 0.25, 0.5, 0.75)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1024, 1088])
def test_istft_per_channel_at_matched_levels(oracle, F):
    """as test_stft_per_channel_at_matched_levels, for both inverse kernels: the same row staircase in both channels of the spectrum, R at half the level"""
    T, S, rows = 64, 3, 145
    eng = _engine(F=F, T=T, stem_modes=(1,) * S, oob_weights=OOB[:S], max_tiles=3)
    _inverse_check(oracle, "matched", eng, spectrum_input(rows, 700 + F, matched=True), mask_input(S, 3, T, F, 800 + F), OOB[:S], T, F, per_channel=True)
    eng.close()


def _inverse_check(oracle, tag, eng, spec, masks, oob, T, F, masks64=None, got=None, per_channel=False, oob64=None, seam_hops=None):
    import torch
    rows = spec.shape[1]
    if got is None:
        md = torch.from_numpy(masks).cuda() if masks is not None else None
        got = eng.istft(torch.from_numpy(spec).cuda(), md).cpu().numpy()
    S = len(oob)
    assert got.shape == (S, 2, (rows + 3) * HOP)
    res = istft_case(oracle, spec, masks, oob, T, F, got, masks64, oob64=oob64, seam_hops=seam_hops)
    G = launcher_G(rows, S, F)
    extra = MARGIN * ola3_window_delta() if F <= 1024 else 0.0                   # only the kernel that rebuilds its window gets the window term
    tag = "istft %s F %d T %d S %d frames %d G %d %s" % (tag, F, T, S, rows, G, "masks" if masks is not None else "no masks")
    if rows >= ZERO_ROW + 6:
        assert res["silent"] >= 2, tag
    report(tag, res, ("hop max",), extra=extra, period=G, per_channel=per_channel)
    check_cap(tag, res)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("F,T,S", [(64, 64, 1), (576, 64, 3), (1024, 128, 5), (1088, 64, 3), (2048, 64, 2)])
def test_istft_geometry_and_band_edge(oracle, F, T, S):
    """an arbitrary spectrum under distinct masks and out-of-band weights, and under no masks: band edge inside a thread's bins (64, 576, 1088), F = 1024 / 2048,
    the stem / tile / channel / row strides, the quirks at bins 0 and 2048 with non-zero imaginary parts"""
    rows = 2 * T + 17
    spec = spectrum_input(rows, 100 + F)
    masks = mask_input(S, 3, T, F, 200 + F)
    eng = _engine(F=F, T=T, stem_modes=(1,) * S, oob_weights=OOB[:S], max_tiles=3)
    _inverse_check(oracle, "geometry", eng, spec, masks, OOB[:S], T, F)
    _inverse_check(oracle, "geometry", eng, spec, None, OOB[:S], T, F)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1024, 1088])
def test_istft_run_seams(oracle, F):
    """G = 5: frames 13..17 give nseg mod G every value (a last run of 1, 2 or 3 drain-only hops, or a mix); 1..3 frames are shorter than the warm-up"""
    T = 64
    eng = _engine(F=F, T=T, stem_modes=(1,), oob_weights=(0.25,), max_tiles=1)
    for frames in (1, 2, 3, 4, 13, 14, 15, 16, 17):
        _inverse_check(oracle, "seams", eng, spectrum_input(frames, 300 + frames), mask_input(1, 1, T, F, 400 + frames), (0.25,), T, F)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F,T,S,frames", [(1024, 64, 3, 1400), (1024, 64, 5, 2100), (1088, 64, 3, 4500)])
def test_istft_long_regimes(oracle, F, T, S, frames):
    """nseg * S >= 4096: G = 13 (minimum run), G = 14 with 755 workgroups of the 768, G = 14 on the table kernel; every hop compared"""
    nt = -(-frames // T)
    eng = _engine(F=F, T=T, stem_modes=(1,) * S, oob_weights=OOB[:S], max_tiles=nt)
    _inverse_check(oracle, "long", eng, spectrum_input(frames, 500 + S), mask_input(S, nt, T, F, 600 + S), OOB[:S], T, F)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F,T,S", [(576, 64, 3), (1088, 64, 3)])
def test_ratio_in_the_prologue(oracle, coeffs, F, T, S):
    """separate() with ratio_mask (srt_ratio_of in the inverse's prologue) equals istft(spec, ratio_mask(forward(mag))) bit for bit, and that chain is within
    the bound of the float64 inverse under a float64 ratio of the GPU's raw masks (the network's tolerance stays out of it)"""
    import torch
    import spleeterrt_amd as srt
    rows = 2 * T + 17
    L, R = signal_rows("staircase", rows)
    oob = OOB[:S]
    eng = _engine(F=F, T=T, stem_modes=(1, 0, 1), oob_weights=oob, variant=srt.VARIANT_VST, max_tiles=3, ratio_mask=True)
    for s in range(S):
        eng.set_coeff(s, coeffs(s))
    Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    out = eng.separate(Ld, Rd).cpu().numpy()
    spec, mag = eng.stft(Ld, Rd)
    raw = eng.forward(mag)
    raw_h = raw.cpu().numpy()
    chain = eng.istft(spec, eng.ratio_mask(raw)).cpu().numpy()
    bad = np.argwhere(out != chain)
    assert bad.size == 0, "%d samples differ, first at %r: %r vs %r" % (len(bad), tuple(bad[0]), out[tuple(bad[0])], chain[tuple(bad[0])])
    sq = raw_h.astype(np.float64) ** 2
    ratio64 = (sq + 1e-10 / S) / (sq.sum(axis=0) + 1e-10)
    _inverse_check(oracle, "ratio", eng, spec.cpu().numpy(), oracle.ratio_mask(raw_h), oob, T, F, masks64=ratio64, got=chain)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1024, 1088])
def test_round_trip_non_periodic(oracle, F):
    """stft -> istft(None), out-of-band weight 1, on the staircased signal at rows = 4099, against the float64 chain per output hop (the oracle's chain sets e_cpu)"""
    import torch
    rows = 4099
    L, R = signal_rows("staircase", rows)
    eng = _engine(F=F, T=64, stem_modes=(1,), oob_weights=(1.0,), max_tiles=1)
    spec, _ = eng.stft(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), want_mag=False)
    got = eng.istft(spec, None).cpu().numpy()
    eng.close()
    res = istft_case(oracle, None, None, (1.0,), 64, F, got, chain=(L, R))
    tag = "round trip F %d rows %d fpb %d G %d" % (F, rows, launcher_fpb(rows), launcher_G(rows, 1, F))
    report(tag, res, ("hop max",), extra=MARGIN * ola3_window_delta() if F <= 1024 else 0.0, period=launcher_G(rows, 1, F))
    check_cap(tag, res)
