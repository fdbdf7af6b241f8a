"""The fp16-storage network, layer by layer, against a float64 evaluation of each layer ALONE fed with the tensors the engine itself stored as that layer's inputs.

The existing fp16 evidence is the final mask within 2e-2 of the fp32 oracle and our C8 kernels against our planar kernels (tests/test_gpu_parity.py): an error common
to both kernel families, or one worth less than 2e-2 of mask, passes.  Here nothing propagates between layers, so the bound per element is what the number formats
give (tests/fp16_layer_ref.py states what each kernel rounds and derives every allowance; nothing is tuned to what the kernels return):

  A  per element, no exceptions   |got - ref| <= ulp16(max(|got|, |ref|)) / 2 + E,  E = K 2^-24 sum|w||a| + E_epi + E_flip
  B  share of got != RN16(ref)    <= 2 x the rate of the emulation of a correct kernel (sequential fp32, tap-major) on the same layer and inputs + 3 standard errors
  C  RMS of (got - ref) in ulp16  <= 1.05 x the emulation's

Tensors stored fp32 (up6, the masks, every tensor when F % 256 != 0) get A without the half-ulp term and no B / C.

One thing the kernels do differently from what a reading of the taps suggests, found while writing this file: in the fp16-storage mode the operand of an encoder layer
is not RN16(act(bn(stored conv))).  The producing kernel rounds act(bn(v)) of its own fp32 v = acc + bias into a second tensor, and the tap keeps only RN16(v).  The
operand is therefore known up to the halves the rounding cell of the tap maps to (61 % - 90 % of the operands have more than one candidate, not the ~2^-11 share of
a tie-only model), E_flip = sum |w| d carries that in check A, check B cannot be held there (most elements are not the nearest half of the centre's value) and
check C is measured in units of the element's own standard deviation under that spread, against an emulation of the PAIR of layers (LayerLocal.enc).  Decoder
layers, down1, up6 and the head read what the taps return and are held to A, B and C exactly as stated above.

Coefficients: the synthetic set with every value moved by up to 2^-12 of itself, so that the conv weights are no fp16 values and RN16(w) in the packing is checked too.
"""
import numpy as np
import pytest

import fp16_layer_ref as R

ENC = ["down%d" % i for i in range(1, 7)]
DEC = ["up%d" % i for i in range(1, 7)]
ALL = ENC + DEC + ["head"]


def _mag_input(oracle, ntiles, T, F, seed=4242):
    """tests/test_gpu_parity.py's recipe: magnitude-like, positive, with sparse peaks"""
    x = np.abs(oracle.lcg(seed, ntiles * 2 * T * F, 6.0)).reshape(ntiles, 2, T, F)
    x[:, :, ::7, ::13] *= 8.0
    return np.ascontiguousarray(x, np.float32)


_coeff_cache = {}


def _coeff(oracle, stem, small=None):
    """synthetic coefficients of a stem, every value scaled by 1 + 2^-12 u, u in [-1/2, 1/2): weights that the fp16 packing has to round.
    small: biases and BN shifts times that factor (with the input scaled alike every tensor of the network shrinks by about the same factor)"""
    key = (stem, small)
    if key not in _coeff_cache:
        c = oracle.synth_coeff(stem)
        c = (c * (np.float32(1) + oracle.lcg(31337 + stem, c.size, 2.0 ** -12))).astype(np.float32)
        if small is not None:
            lo = oracle.layout()
            for i in range(6):
                for L, bn in ((lo.down[i], i < 5), (lo.up[i], True)):
                    c[L.b:L.b + L.cout] *= np.float32(small)
                    if bn:
                        c[L.bn:L.bn + L.cout] *= np.float32(small)
            c[lo.head_b:lo.head_b + 2] *= np.float32(small)
        _coeff_cache[key] = np.ascontiguousarray(c)
    return _coeff_cache[key]


def _layers(LL, taps, mask, layers):
    """-> {layer: judge(...)} for the layers asked for"""
    out = {}
    for n in layers:
        if n == "head":
            ref, yard = LL.head()
            got = mask
        elif n.startswith("down"):
            ref, yard = LL.enc(int(n[-1]))
            got = taps["conv" + n[-1]]
        else:
            ref, yard = LL.dec(int(n[-1]))
            got = taps[n]
        out[n] = R.judge(got, ref, yard)
    return out


def _fmt(tag, n, j):
    s = "%s %-5s A: %d over, worst %.3f of the bound" % (tag, n, j["a_viol"], j["a_worst"])
    if j["share"]:
        s += ", operands with more than one candidate %.4f" % j["share"]
    if j["subnormal"] > 0.001:
        s += ", %.3f of the tensor below 2^-14" % j["subnormal"]
    if "b" in j:
        s += "; B %.5f (emulation %.5f, cap %.5f); C %.4f (emulation %.4f, cap %.4f); flushed %d" % (j["b"], j["b_emu"], j["b_cap"], j["c"], j["c_emu"], j["c_cap"], j["flushed"])
    return s + ("   FAILS " + "".join(j["fail"]) if j["fail"] else "")


# =========================================================================================== CPU part
@pytest.mark.parametrize("T,F", [(64, 512), (64, 256)])
def test_float64_layers_match_the_oracle(oracle, T, F):
    """operand_half off: each float64 layer against the oracle's own fp32 layer function on the same operands, per element within the worst case of the oracle's
    sequential fp32 accumulation ((K + 2) 2^-24 sum|w||a|), and the float64 chain against orc_forward's taps at the suite's fp32 tap tolerance (2e-5 of the tensor's
    RMS, 1e-4 of its peak): fixes padding, parity, the concat order and activation-before-BN for both stem modes."""
    x = _mag_input(oracle, 1, T, F, seed=515)[0]
    for stem, mode in ((0, 0), (1, 1)):
        coeff = _coeff(oracle, stem)
        C = R.Coeff(oracle, coeff)
        y, otaps = oracle.forward(coeff, x, mode, oracle.VARIANT_VST, want_taps=True)
        taps, mask = R.forward64(C, mode, x, operand_half=False)
        for n, ref in otaps.items():
            got = taps[n]
            rms = float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref.astype(np.float64) ** 2)))
            mx = float(np.abs(got - ref).max() / np.abs(ref).max())
            assert rms < 2e-5 and mx < 1e-4, (stem, n, rms, mx)
        assert float(np.abs(mask - y).max()) <= 2e-4
        # the layer functions alone, on the oracle's own tensors
        for i in (1, 3, 6):
            a = x if i == 1 else otaps["act%d" % (i - 1)]
            L = C.enc[i - 1]
            w32 = np.ascontiguousarray(L["w"], np.float32).ravel()
            want = oracle.conv5x5_s2(a, w32, L["w"].shape[0])
            got = R.contract64("conv", a, L["w"])
            A = R.contract64("conv", np.abs(a), np.abs(L["w"]))
            assert (np.abs(got - want) <= (25 * a.shape[0] + 2) * R.EPS32 * A).all(), (stem, "conv", i)
        for i in (1, 4, 6):
            xin = otaps["conv6"] if i == 1 else np.concatenate([otaps["conv%d" % (7 - i)], otaps["up%d" % (i - 1)]])
            L = C.dec[i - 1]
            want = oracle.tconv5x5_s2(xin, np.ascontiguousarray(L["w"], np.float32).ravel(), L["w"].shape[1])
            got = R.contract64("tconv", xin, L["w"])
            A = R.contract64("tconv", np.abs(xin), np.abs(L["w"]))
            assert (np.abs(got - want) <= (25 * xin.shape[0] + 2) * R.EPS32 * A).all(), (stem, "tconv", i)
        want = oracle.conv4x4_d2(otaps["up6"][0], np.ascontiguousarray(C.head_w, np.float32).ravel())
        got = R.contract64("head", otaps["up6"], C.head_w.reshape(2, 1, 4, 4))
        A = R.contract64("head", np.abs(otaps["up6"]), np.abs(C.head_w.reshape(2, 1, 4, 4)))
        assert (np.abs(got - want) <= 18 * R.EPS32 * A).all(), (stem, "head")


def test_number_format_helpers():
    """RN16 / the truncating store / ulp16 on the values where they can go wrong: ties, the binade edge, the subnormal range"""
    assert R.rn16(1 + 2.0 ** -11) == 1.0 and R.rn16(1 + 3 * 2.0 ** -11) == 1 + 2.0 ** -9          # ties to even
    assert R.rn16(2.0 ** -25) == 0.0 and R.rn16(2.0 ** -25 * 1.01) == 2.0 ** -24                  # subnormals kept
    assert R.trunc16(1 + 2.0 ** -10 - 2.0 ** -30) == 1.0 and R.trunc16(-(1 + 2.0 ** -10 - 2.0 ** -30)) == -1.0
    assert R.ulp16(1.0) == 2.0 ** -10 and R.ulp16(0.999) == 2.0 ** -11 and R.ulp16(2.0 ** -14) == 2.0 ** -24 and R.ulp16(0.0) == 2.0 ** -24 and R.ulp16(-3.0) == 2.0 ** -9


@pytest.fixture(scope="module")
def emulated(oracle):
    """the emulation of a correct fp16-storage network on two tiles x two stems of 64 x 512 and one 64 x 256 instance: the stand-in for the GPU, computed once"""
    out = {}
    x = _mag_input(oracle, 2, 64, 512, seed=616)
    for stem, mode in ((0, 0), (1, 1)):
        C = R.Coeff(oracle, _coeff(oracle, stem))
        for t in (0, 1):
            if stem == 0 and t == 1:
                continue
            out[(512, stem, t)] = (C, mode, x[t]) + R.emulate_network(C, mode, x[t], down1_f16=(stem == 1))
    x = _mag_input(oracle, 1, 64, 256, seed=617)
    C = R.Coeff(oracle, _coeff(oracle, 0))
    out[(256, 0, 0)] = (C, 0, x[0]) + R.emulate_network(C, 0, x[0])
    return out


@pytest.mark.parametrize("key", [(512, 0, 0), (512, 1, 0), (256, 0, 0)])
def test_a_correct_kernel_passes(emulated, key):
    """the unperturbed emulation passes A, B and C on every layer (both stem modes, both down1 forms, the one-pixel-high deep layers of F = 256); the encoder
    layers' yardstick comes from its own emulation of the layer pair, not from the values under test"""
    C, mode, x, taps, mask, _ = emulated[key]
    LL = R.LayerLocal(C, mode, x, taps, act16=True, down1_f16=(key[1] == 1))
    res = _layers(LL, taps, mask, ALL)
    for n, j in res.items():
        print(_fmt("emulation %r" % (key,), n, j))
    assert not [n for n, j in res.items() if j["fail"]], {n: j["fail"] for n, j in res.items() if j["fail"]}
    for n in DEC[:5] + ["down1"]:
        assert res[n]["b"] <= 0.01 and 0.15 <= res[n]["c"] <= 0.35, (n, res[n])     # the issue's CPU model: rates of 0.1 % - 0.7 %, RMS near 1 / sqrt(12)


def test_tensors_kept_fp32_have_few_ambiguous_operands(oracle):
    """F % 256 != 0: the consuming encoder rounds act(bn(stored fp32 conv)) itself, so an operand is ambiguous only within the fp32 evaluation allowance of a rounding
    tie: at most 1 % of a layer's operands (measured: 0.40 % - 0.45 %), on the fp32 oracle's tensors of the 64 x 576 case"""
    x = _mag_input(oracle, 1, 64, 576, seed=606)[0]
    for stem, mode in ((0, 0), (1, 1)):
        coeff = _coeff(oracle, stem)
        C = R.Coeff(oracle, coeff)
        _, otaps = oracle.forward(coeff, x, mode, oracle.VARIANT_VST, want_taps=True)
        for i in range(1, 6):
            _, _, d, _ = R.enc_operand(otaps["conv%d" % i], C.enc[i - 1]["scale"], C.enc[i - 1]["shift"], R.ELU if mode else R.LEAKY, cell=False)
            assert float((d > 0).mean()) <= 0.01, (stem, i, float((d > 0).mean()))


PLANTED = ["tap_first_col", "tap_last_col", "concat_halves", "one_weight", "bn_next_channel", "truncated", "weights_unrounded", "neighbour_instance"]


def _plant(err, run, x, w, store, swapped, bn_next, neighbour):
    """the stored tensor of a layer with one error planted.  run(x, w, **kw) -> the emulation's fp32 value before the store; store: RN16, or the identity for a
    tensor kept fp32; swapped: the operands with their channel halves exchanged; bn_next(): that fp32 value with the BN parameters of channel c + 1"""
    if err in ("tap_first_col", "tap_last_col"):
        col, kx = (0, 1) if err == "tap_first_col" else (-1, 2)  # a tap that reads image columns there, not padding
        w2 = w.copy()
        w2[:, :, 2, kx] = 0
        v = run(x, w)
        v[:, :, col] = run(x, w2)[:, :, col]
        return store(v)
    if err == "concat_halves":
        return store(run(swapped, w))
    if err == "one_weight":
        w2 = w.copy()
        w2[5, 1, 2, 2] = 0
        return store(run(x, w2))
    if err == "bn_next_channel":
        return store(bn_next())
    if err == "truncated":
        return R.trunc16(run(x, w))
    if err == "weights_unrounded":
        return store(run(x, w, w_half=False))
    return np.asarray(neighbour, np.float64)


def _halves_swapped(x):
    h = x.shape[0] // 2
    return np.concatenate([x[h:], x[:h]])


def _planted(emulated, layer, err):
    """(got with the error, Ref, yard) for a layer of the 64 x 512 ELU stem (tile 0; tile 1 is the neighbour instance)"""
    C, mode, x, taps, _, hid = emulated[(512, 1, 0)]
    _, _, _, taps_n, _, hid_n = emulated[(512, 1, 1)]
    i = int(layer.split("_")[0][-1])
    fp32 = layer.endswith("_fp32")         # the layer on tensors kept fp32: the stored conv + bias before it is the fp32 value itself, and so is its output
    if fp32:
        taps = dict(taps, **{"conv%d" % (i - 1): hid["v%d" % (i - 1)]})
    LL = R.LayerLocal(C, mode, x, taps, act16=not fp32, down1_f16=True)
    store = (lambda v: np.asarray(v, np.float64)) if fp32 else R.rn16
    if layer.startswith("up"):
        L = C.dec[i - 1]
        ref, yard = LL.dec(i)
        xin = LL.dec_input(i)
        run = lambda x_, w_, sc=L["scale"], sh=L["shift"], **kw: R.dec_emulate(x_, w_, L["b"], sc, sh, R.ELU, **kw)
        return _plant(err, run, xin, L["w"], store, _halves_swapped(xin), lambda: run(xin, L["w"], np.roll(L["scale"], -1), np.roll(L["shift"], -1)), taps_n[layer]), ref, yard
    L = C.enc[i - 1]
    ref, yard = LL.enc(i)
    run = lambda a_, w_, **kw: R.enc_emulate(a_, w_, L["b"], None, None, R.ELU, **kw)[0]
    if i == 1:
        a = R.rn16(np.minimum(x, R.HMAX))
        bn_next = lambda: run(a, L["w"]) + (np.roll(L["b"], -1) - L["b"]).astype(np.float32)[:, None, None]   # its only per-channel parameter: the bias of channel c + 1
        return _plant(err, run, a, L["w"], store, a[::-1], bn_next, taps_n["conv1"]), ref, yard
    a, P = hid["act%d" % (i - 1)], C.enc[i - 2]                  # the operand the emulated producer stored; the error goes into the operand's BN
    sc, sh = np.roll(P["scale"], -1).astype(np.float32)[:, None, None], np.roll(P["shift"], -1).astype(np.float32)[:, None, None]
    bn_next = lambda: run(R.rn16(R.act32(sc * hid["v%d" % (i - 1)] + sh, R.ELU)), L["w"])
    return _plant(err, run, a, L["w"], store, _halves_swapped(a), bn_next, hid_n["v%d" % i] if fp32 else taps_n["conv%d" % i]), ref, yard


# down3 in the fp16-storage mode: its operands are known only up to the rounding cell of the tap, a spread of about 2^-11 of each operand.  Weights left unrounded
# (moved by <= 2^-13 of themselves here) change the result by less than that spread does: the one planted error no layer-local check can see THERE (measured: C
# 0.950 against 0.919, cap 0.981); on tensors kept fp32 only check A applies, and the worst case of the fp32 accumulation in it is wider than that change too.  The
# same packing line rounds the weights of every encoder and decoder layer (srt_pack16_kernel), and the error is caught on the decoder and on down1 (checks B and C).
@pytest.mark.parametrize("layer,err", [(l, e) for l in ("down1", "down3", "up3", "down3_fp32") for e in PLANTED
                                       if (l, e) not in (("down3", "weights_unrounded"), ("down3_fp32", "weights_unrounded"), ("down3_fp32", "truncated"))])
def test_planted_errors_are_caught(emulated, layer, err):
    """each error applied to the emulation's output of a decoder layer (up3), of an encoder layer whose operands the taps give exactly (down1), of one whose
    operands they give only up to the rounding cell (down3) and of that layer on tensors kept fp32 (check A alone) must fail at least one of A, B, C"""
    got, ref, yard = _planted(emulated, layer, err)
    j = R.judge(got, ref, yard)
    print(_fmt("planted %s" % err, layer, j))
    assert j["fail"], (layer, err, j)


# =========================================================================================== GPU part
CASES = {
    # name: T, F, tiles, stem modes, sampled (stem, tile), layers, {launch name: kernel prefix}, environment
    "planar":            (64, 512, 1, (0, 1), [(0, 0), (1, 0)], ALL, {"down3": "srt_enc_f16<", "down6": "srt_enc_f16<", "up2": "srt_dec_f16<", "up5": "srt_dec_f16<"}, {}),
    "planar_one_pixel":  (64, 256, 1, (0,), [(0, 0)], ALL, {"down3": "srt_enc_f16<", "down6": "srt_enc_f16<", "up1": "srt_dec_f16<", "up2": "srt_dec_f16<"}, {}),
    # (W = 18 and 9 are no multiples of 4: down6, up1 and up2 run on the fp32 MFMA kernels)
    "tensors_fp32":      (64, 576, 1, (1,), [(0, 0)], ALL, dict([("down%d" % i, "srt_enc_f16<") for i in (2, 3, 4, 5)] + [("up%d" % i, "srt_dec_f16<") for i in (3, 4, 5)] +
                                                                [("down6", "srt_enc_mfma<"), ("up1", "srt_dec_mfma<"), ("up2", "srt_dec_mfma<")]), {}),
    "c8":                (64, 512, 9, (1, 0), [(s, t) for s in (0, 1) for t in (0, 4, 8)], ALL, "c8", {}),
    "c8_partial_tiles":  (64, 256, 17, (0,), [(0, t) for t in (0, 8, 16)], ALL, "c8", {}),
    "c8_odd_tile_counts": (192, 768, 6, (1, 1, 0), [(0, 5), (2, 5)], ALL, "c8", {}),
    "c8_bench_geometry": (256, 1024, 5, (0, 1, 1, 1), [(3, 4)], ENC[2:] + DEC[:4], "c8", {}),
    "down1_c8":          (64, 512, 96, (1,), [(0, 0), (0, 47), (0, 95)], ENC[:3], {"down1": "srt_down1_f16_kernel<1>", "down2": "srt_enc_c8<", "down3": "srt_enc_c8<"}, {}),
    # five stems: down1 goes out as a group of four stems and the fifth alone.  At 4 tiles both groups are below the streamed kernels' launch condition
    # ((F / 2 / 64) * tiles * 2 >= 768, srt_launch_enc2) and run the tiled fp32-MFMA kernel with fp16 outputs ...
    "fifth_stem":        (64, 512, 4, (1, 0, 1, 1, 0), [(0, 3), (4, 3)], ENC[:2], {"down1": ["srt_enc_mfma2<", "srt_enc_mfma2<"], "down2": "srt_enc_f16<"}, {}),
    # ... and the two-wave streamed down1 with fp16 C8 outputs runs for a fifth stem at 96 tiles with down1 kept off the fp16 MFMA.  A batch of this size also runs
    # the streamed up6 and the row-walking head: checked here too
    "fifth_stem_streamed": (64, 512, 96, (1, 0, 1, 1, 0), [(0, 95), (4, 95)], ENC[:2] + ["up6", "head"],
                            {"down1": ["srt_down1_stream_kernel<0, true, 4, true", "srt_down1_stream_kernel<0, true, 2, true"], "down2": "srt_enc_c8<",
                             "up6": "srt_up6_stream_kernel<64, 2, 0, true", "up7": "srt_head_rows_kernel<false"}, {"SPLEETERRT_D1F16": "0"}),
    # every tensor about 2^-13 of its usual size (input, biases and BN shifts scaled): the deep tensors lie in the fp16 subnormal range; a store that flushes shows in A
    "subnormal":         (64, 512, 1, (0, 1), [(0, 0), (1, 0)], ALL, {"down3": "srt_enc_f16<", "up2": "srt_dec_f16<"}, {}),
    "subnormal_c8":      (64, 512, 9, (1, 0), [(0, 8), (1, 8)], ALL, "c8", {}),
}
C8_KERNELS = dict([(n, "srt_enc_c8<") for n in ENC[2:]] + [(n, "srt_dec_c8<") for n in DEC[:5]])
SMALL = 2.0 ** -13


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_fp16_layers_against_float64(oracle, case):
    """One forward per case, the taps of the sampled instances, and for every layer checks A, B, C against the float64 layer fed with the fetched input taps.
    The cases are the smallest shapes at which each kernel form of the fp16-storage mode occurs; the kernel symbols are asserted."""
    import os
    import torch
    import spleeterrt_amd as srt
    T, F, ntiles, modes, sample, layers, kernels, env = CASES[case]
    small = SMALL if case.startswith("subnormal") else None
    S = len(modes)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = srt.Engine(F=F, T=T, stem_modes=modes, variant=srt.VARIANT_VST, max_tiles=ntiles, precision=srt.PREC_F16)
        for s in range(S):
            eng.set_coeff(s, _coeff(oracle, s, small))
        x = _mag_input(oracle, ntiles, T, F, seed=606)
        if small is not None:
            x *= np.float32(small)
        xd = torch.from_numpy(x).cuda()
        eng.forward(xd)
        eng.set_timing(True)
        masks = eng.forward(xd).cpu().numpy()
        ks = eng.get_timing_kernels()
        eng.set_timing(False)
        need = {"conv%d" % i for i in range(1, 7)} | {"up%d" % i for i in range(1, 7)}
        if layers is not ALL:                                    # a subset of layers: only the tensors they and their yardsticks read
            need = set()
            for n in layers:
                if n == "head":
                    need |= {"up6"}
                    continue
                i = int(n[-1])
                need |= {"conv%d" % j for j in (i - 2, i - 1, i) if j >= 1} if n.startswith("down") else ({"conv6", "up1"} if i == 1 else {"conv%d" % (7 - i), "up%d" % (i - 1), "up%d" % i})
        fetched = {(s, t): {n: eng.tensor(n, s, t) for n in sorted(need)} for (s, t) in sample}
        eng.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert np.isfinite(masks).all()
    launched = {}
    for n, k in ks:
        launched.setdefault(n, []).append(k)
    print("\n%s: %s" % (case, "; ".join("%s = %s" % (n, " + ".join(k)) for n, k in launched.items())))
    for n, want in (C8_KERNELS if kernels == "c8" else kernels).items():
        want = want if isinstance(want, list) else [want]
        assert len(launched[n]) == len(want) and all(k.startswith(w) for k, w in zip(launched[n], want)), (n, launched[n], want)
    act16 = F % 256 == 0                                         # srtCreate: fp16 activation storage needs F % 256 == 0; otherwise the tensors stay fp32
    d1f16 = launched["down1"][0].startswith("srt_down1_f16_kernel")
    f32_layers = [n for n in ENC[1:] + DEC[:5] if not launched[n][0].startswith(("srt_enc_f16<", "srt_dec_f16<", "srt_enc_c8<", "srt_dec_c8<"))]
    assert not (act16 and f32_layers), f32_layers
    failed = []
    for (s, t) in sample:
        LL = R.LayerLocal(R.Coeff(oracle, _coeff(oracle, s, small)), modes[s], x[t], fetched[(s, t)], act16=act16, down1_f16=d1f16, f32_layers=f32_layers)
        res = _layers(LL, fetched[(s, t)], masks[s, t], layers)
        for n, j in res.items():
            print(_fmt("%s stem %d tile %d" % (case, s, t), n, j))
        for n, j in res.items():
            if j["fail"]:
                failed.append((s, t, n, "".join(j["fail"]), j["a_viol"], j["a_worst"], j["a_where"]))
            if not act16 and n.startswith("down"):
                assert j["share"] <= 0.01, (s, t, n, j["share"])  # the condition of the tie-only E_flip
            assert j.get("flushed", 0) == 0, (s, t, n, "stored zeros where the reference is a subnormal half", j["flushed"])
            if small is not None and "b" in j:
                assert j["subnormal"] >= 0.02, (s, t, n, j["subnormal"])    # values of order 1 scaled by 2^-13 are of order 2 x 2^-14: the case is in the range it is about
    assert not failed, failed
