"""The converter over spans of a stream (srtResampleSpans, Resampler.resample_spans): frames computed from two consecutive spans of the input and
for several stereo pairs per launch have srtResample's bits.

GPU, about 20 000 frames per case: the rate pairs of tests/test_resample.py::test_any_partition_gives_the_same_bits, 1 / 3 / 5 pairs, the signal cut into (A, B) at
several points (b_len = 0 and a negative a0 included), the weight bank and the on-the-fly weights; a range whose spans start after frame 0, the widest such range
accepted and one frame more refused; positions above 2^40 (shift invariance); NaN-filled memory around both spans."""
import os

import numpy as np
import pytest

RATES = [(48000, 44100), (96000, 44100), (44100, 48000), (22050, 44100), (8000, 44100), (44056, 44100), (192000, 44100)]
N = 20011
PLANES = 10                        # five stereo pairs
PAD = 64                           # NaN frames on either side of every span


def _resampler(fs_in, fs_out, onfly):
    import spleeterrt_amd as srt
    if not onfly:
        return srt.Resampler(fs_in, fs_out)
    os.environ["SPLEETERRT_RESAMPLE_ONFLY"] = "1"
    try:
        return srt.Resampler(fs_in, fs_out)
    finally:
        del os.environ["SPLEETERRT_RESAMPLE_ONFLY"]


@pytest.fixture(scope="module")
def signal():
    x = np.random.default_rng(23).standard_normal((PLANES, N)).astype(np.float32)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def whole(signal):
    """srtResample of every pair, whole stream, per rate pair: computed once, read-only"""
    cache = {}

    def get(fs_in, fs_out):
        import torch
        if (fs_in, fs_out) not in cache:
            r = _resampler(fs_in, fs_out, False)
            x = torch.from_numpy(signal.copy()).cuda()
            ref = np.stack([y.cpu().numpy() for p in range(PLANES // 2) for y in r.resample(x[2 * p], x[2 * p + 1])])
            r.close()
            ref.setflags(write=False)
            cache[(fs_in, fs_out)] = ref
        return cache[(fs_in, fs_out)]
    return get


def _span(x, lo, hi, planes, lead=0):
    """frames [lo, hi) of the first `planes` planes as a view with PAD NaN frames (and `lead` more, in front) around each plane's frames"""
    import torch
    buf = torch.full((planes, lead + hi - lo + 2 * PAD), float("nan"), device="cuda")
    buf[:, PAD + lead:PAD + lead + hi - lo] = x[:planes, lo:hi]
    return buf[:, PAD:PAD + lead + hi - lo]


@pytest.mark.gpu
@pytest.mark.parametrize("fs_in,fs_out", RATES)
def test_spans_give_the_whole_calls_bits(signal, whole, fs_in, fs_out):
    import torch
    import spleeterrt_amd as srt
    from spleeterrt_amd import stream
    ref = whole(fs_in, fs_out)
    m = ref.shape[1]
    g = stream.rs_geometry(fs_in, fs_out)
    x = torch.from_numpy(signal.copy()).cuda()
    for onfly in (False, True):
        r = _resampler(fs_in, fs_out, onfly)
        assert r.length(N) == m
        for pairs in (1, 3, 5):
            pl = 2 * pairs
            for cut in (1, N // 3, N - 1, N):
                a, b = _span(x, 0, cut, pl), (_span(x, cut, N, pl) if cut < N else None)
                out = _span(torch.zeros(pl, m, device="cuda"), 0, m, pl)
                got = r.resample_spans(a, 0, b, N, 0, m, out=out).cpu().numpy()
                assert np.array_equal(got, ref[:pl]), (onfly, pairs, cut, int((got != ref[:pl]).sum()))
            # a negative a0: 37 frames of NaN in front of frame 0 belong to span A and are never staged
            got = r.resample_spans(_span(x, 0, 5000, pl, lead=37), -37, _span(x, 5000, N, pl), N, 0, m).cpu().numpy()
            assert np.array_equal(got, ref[:pl]), (onfly, pairs, "negative a0")
            # spans [a0, end) inside the signal: the frames whose taps 0 .. 2 LO + 1 they hold, and not one more on either side
            a0, mid, end = 3001, 9000, 15002
            j0 = -(-(a0 + g["LO"]) * g["Q"] // g["P"])                                      # first j with floor(j P / Q) - LO >= a0
            j1 = -(-(end - g["LO"] - 1) * g["Q"] // g["P"])                                 # first j with floor(j P / Q) + LO + 1 >= end
            assert j0 * g["P"] // g["Q"] - g["LO"] >= a0 > (j0 - 1) * g["P"] // g["Q"] - g["LO"]
            assert (j1 - 1) * g["P"] // g["Q"] + g["LO"] + 1 < end <= j1 * g["P"] // g["Q"] + g["LO"] + 1 and j1 - j0 > 1000
            a, b = _span(x, a0, mid, pl), _span(x, mid, end, pl)
            got = r.resample_spans(a, a0, b, N, j0, j1 - j0).cpu().numpy()
            assert np.isfinite(got).all() and np.array_equal(got, ref[:pl, j0:j1]), (onfly, pairs, "interior")
            for o0, cnt in ((j0 - 1, 5), (j1 - 4, 5)):
                out = torch.full((pl, cnt), 7.0, device="cuda")
                with pytest.raises(srt.EngineError, match="srtResampleSpans.*neither span holds"):
                    r.resample_spans(a, a0, b, N, o0, cnt, out=out)
                assert bool((out == 7.0).all())                                           # refused before any launch
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fs_in,fs_out", [(48000, 44100), (44100, 48000)])
def test_shift_invariance_above_2_pow_40(signal, whole, fs_in, fs_out):
    """a0' = a0 + k P, n_in' = n_in + k P, out0' = out0 + k Q with out0' P > 2^40: the frames whose weighted taps lie inside the signal keep their bits"""
    import torch
    from spleeterrt_amd import stream
    ref = whole(fs_in, fs_out)
    g = stream.rs_geometry(fs_in, fs_out)
    P, Q, LO = g["P"], g["Q"], g["LO"]
    k = (1 << 40) // (P * Q) + 12345
    j0 = -(-LO * Q // P)
    j1 = -(-(N - LO - 1) * Q // P)
    assert (j0 + k * Q) * P > 1 << 40 and j1 - j0 > 15000
    x = torch.from_numpy(signal.copy()).cuda()
    for onfly in (False, True):
        r = _resampler(fs_in, fs_out, onfly)
        a, b = _span(x, 0, 7001, 6), _span(x, 7001, N, 6)
        base = r.resample_spans(a, 0, b, N, j0, j1 - j0).cpu().numpy()
        far = r.resample_spans(a, k * P, b, N + k * P, j0 + k * Q, j1 - j0).cpu().numpy()
        r.close()
        assert np.array_equal(base, ref[:6, j0:j1])
        assert np.array_equal(far, base), (onfly, int((far != base).sum()))


@pytest.mark.gpu
def test_argument_refusals(signal):
    import torch
    import spleeterrt_amd as srt
    r = srt.Resampler(48000, 44100)
    x = torch.from_numpy(signal.copy()).cuda()
    m = r.length(N)
    out = torch.full((2, m), 7.0, device="cuda")
    L = r.L
    p = lambda t: t.data_ptr()
    cases = [("null resampler", (None, 1, p(x), N, 0, N, None, 0, 0, N, 0, m, p(out), m), "null"),
             ("no pairs", (r.h, 0, p(x), N, 0, N, None, 0, 0, N, 0, m, p(out), m), "pairs"),
             ("too many pairs", (r.h, 9, p(x), N, 0, N, None, 0, 0, N, 0, m, p(out), m), "pairs"),
             ("null span", (r.h, 1, None, N, 0, N, None, 0, 0, N, 0, m, p(out), m), "null"),
             ("null second span", (r.h, 1, p(x), N, 0, 100, None, N, N - 100, N, 0, m, p(out), m), "null"),
             ("null output", (r.h, 1, p(x), N, 0, N, None, 0, 0, N, 0, m, None, m), "null"),
             ("stride below the span", (r.h, 1, p(x), N - 1, 0, N, None, 0, 0, N, 0, m, p(out), m), "stride"),
             ("stride below the output", (r.h, 1, p(x), N, 0, N, None, 0, 0, N, 0, m, p(out), m - 1), "stride"),
             ("range too large", (r.h, 1, p(x), N, 0, N, None, 0, 0, N, 1 << 44, m, p(out), m), "too large"),
             ("signal longer than the spans", (r.h, 1, p(x), N, 0, N, None, 0, 0, N + 1000, 0, m, p(out), m), "neither span")]
    for name, args, word in cases:
        assert L.srtResampleSpans(*args) == -1, name
        text = L.srtLastError().decode()
        assert "srtResampleSpans" in text and word in text, (name, text)
    assert L.srtResampleSpans(r.h, 1, p(x), N, 0, N, None, 0, 0, N, 0, 0, None, 0) == 0      # nothing asked for
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    r.close()
