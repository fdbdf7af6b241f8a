"""float64 layer-local reference, fp32 emulation of a correct kernel and the checks A / B / C of tests/test_fp16_layer_local.py.

Every layer of the U-Net is evaluated ALONE, fed with the tensors the engine itself stored as that layer's inputs, so nothing propagates between layers.
The layer definitions are the oracle's (oracle/spleeter_oracle.c, orc_forward); what each kernel family rounds is read from the kernels and stated here.

What the fp16-storage mode (Engine(precision=PREC_F16), F % 256 == 0) rounds
  conv weights     RN16(w) for every layer on v_mfma_f32_32x32x16_f16 (srt_pack16_kernel, the class-stacked up5 pack, up6's a16 registers, srt_down1_f16_kernel);
                   bias and BN parameters stay fp32.  down1 on the fp32 MFMA (srt_enc_mfma2, srt_down1_stream_kernel) and the head use the fp32 weights.
  decoder operand  the stored halves themselves: up1 reads conv6, up_i reads concat(raw conv_{7-i}, up_{i-1}), staged without arithmetic.  half x half is exact in fp32.
  encoder operand  NOT a function of the stored conv_{i-1}.  The producing kernel evaluates BOTH of its outputs from the fp32 value v = acc + bias:
                   raw = RN16(v) (the tap, the decoder's skip operand) and act = RN16(act_E(bn(v))) (a second fp16 tensor, the next encoder layer's operand,
                   which no tap returns).  All that the tap says about v is that it lies in the rounding cell of raw, |v - raw| <= ulp16(raw) / 2, so the operand
                   is known up to the halves that act_E(bn(.)) maps that cell to.  `enc_operand(..., cell=True)` returns the centre RN16(act_E(bn(raw))) and
                   the largest distance d to any half in that image; check A carries sum |w| d as E_flip.  (On tensors kept fp32, F % 256 != 0, the consuming
                   encoder does compute RN16(act_E(bn(raw))) from the stored fp32 raw: there d is non-zero only next to a rounding tie, `cell=False`.)
  down1 operand    srt_down1_f16_kernel: RN16(min(x, 65504)); the fp32-MFMA forms: x itself, products rounded in fp32.
  up6              halves x RN16(w) on the fp16 MFMA (one product row per tap, gathered in fp32), fp32 epilogue, fp32 store: no output rounding term.
  head             fp32 FMA chain over up6 (fp32), + bias, logistic from v_exp_f32 and v_rcp_f32, fp32 masks.
  stores           (_Float16)float: round to nearest even, subnormals kept (no flush).

Allowances
  accumulation     K * 2^-24 * A with K the number of accumulated terms (25 * Cin; 16 for the head) and A = sum |w| |a|: the textbook worst case of fp32
                   accumulation in any order.  Layers that multiply in fp32 get one more 2^-24 A for the product roundings.
  epilogue         C_EPI * 2^-24 times the magnitudes involved, C_EPI = 4.  Every add / multiply of the epilogue is one fp32 rounding (2^-24 relative).  The
                   exponential is v_exp_f32(x * log2e): the instruction is documented to 1 ulp (2 * 2^-24 relative) and the rounded argument adds
                   <= 2 |x| e^x 2^-24, together <= 2 * 2^-24 * e^x (1 + |x|) <= 2 * 2^-24 on x <= 0; times a BN scale <= 1.5 that is below 4 * 2^-24.
"""
import numpy as np

EPS32 = 2.0 ** -24
C_EPI = 4.0
ENC_CH = [(2, 16), (16, 32), (32, 64), (64, 128), (128, 256), (256, 512)]
DEC_CH = [(512, 256), (512, 128), (256, 64), (128, 32), (64, 16), (32, 1)]
LEAKY, RELU, ELU = 0, 1, 2
HMAX = 65504.0


# ------------------------------------------------------------------------------------------- number formats
def rn16(x):
    """round to the nearest half, ties to even, subnormals kept; returned as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def trunc16(x):
    """round towards zero to a half (the planted 'stored by truncation' error)"""
    x = np.asarray(x, np.float64)
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h.astype(np.float64)


def ulp16(x):
    """2^(max(floor(log2 |x|), -14) - 10): the spacing of halves at |x| (the subnormal spacing 2^-24 below 2^-14)"""
    ax = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(ax)                                          # |x| = m 2^e, m in [0.5, 1): floor(log2 |x|) = e - 1
    return np.ldexp(1.0, np.maximum(np.where(ax == 0, -14, e - 1), -14) - 10)


def act64(x, kind):
    if kind == LEAKY:
        return np.where(x >= 0, x, 0.2 * x)
    if kind == RELU:
        return np.maximum(x, 0.0)
    return np.where(x >= 0, x, np.expm1(np.minimum(x, 0.0)))    # VARIANT_VST: no clamp at -15


def act32(x, kind):
    """the device's fp32 evaluation order (srt_device.h, contraction off)"""
    x = np.asarray(x, np.float32)
    if kind == LEAKY:
        return np.maximum(x, np.float32(0.2) * x)
    if kind == RELU:
        return np.maximum(x, np.float32(0.0) * x)
    return np.maximum(x, np.float32(0)) + (np.exp(np.minimum(x, np.float32(0))) - np.float32(1))


# ------------------------------------------------------------------------------------------- coefficients
class Coeff:
    """views into one stem's coefficient blob, as float64 (layout: oracle.layout())"""

    def __init__(self, oracle, coeff):
        lo = oracle.layout()
        c = np.asarray(coeff, np.float64)
        self.enc, self.dec = [], []
        for i, (ci, co) in enumerate(ENC_CH):
            L = lo.down[i]
            d = dict(w=c[L.w:L.w + 25 * ci * co].reshape(co, ci, 5, 5), b=c[L.b:L.b + co])
            if i < 5:
                d["shift"], d["scale"] = c[L.bn:L.bn + co], c[L.bn + co:L.bn + 2 * co]
            self.enc.append(d)
        for i, (ci, co) in enumerate(DEC_CH):
            L = lo.up[i]
            self.dec.append(dict(w=c[L.w:L.w + 25 * ci * co].reshape(ci, co, 5, 5), b=c[L.b:L.b + co],
                                 shift=c[L.bn:L.bn + co], scale=c[L.bn + co:L.bn + 2 * co]))
        self.head_w = c[lo.head_w:lo.head_w + 32].reshape(2, 4, 4)
        self.head_b = c[lo.head_b:lo.head_b + 2]


# ------------------------------------------------------------------------------------------- contractions
# kind "conv":  y[co][ho][wo] = sum w[co][ci][ky][kx] x[ci][2ho+ky-1][2wo+kx-1]          (orc_conv5x5_s2)
# kind "tconv": y[co][2h+ky-1][2w+kx-1] += sum_ci w[ci][co][ky][kx] x[ci][h][w]          (orc_tconv5x5_s2)
# kind "head":  y[s][h][w] = sum w[s][ky][kx] x[h+2ky-3][w+2kx-3]                        (orc_conv4x4_d2; x [1][H][W], w [2][1][4][4])
def _taps(kind, x, w, dtype):
    """-> (out buffer, crop, [(weights [Cout][Cin], input view [Cin][h][w], output view [Cout][h][w])] in tap order)"""
    x = np.asarray(x, dtype)
    w = np.asarray(w, dtype)
    cin, H, W = x.shape
    if kind == "conv":
        Ho, Wo = H // 2, W // 2
        xp = np.zeros((cin, H + 3, W + 3), dtype)
        xp[:, 1:1 + H, 1:1 + W] = x
        y = np.zeros((w.shape[0], Ho, Wo), dtype)
        return y, (slice(None), slice(None), slice(None)), [(w[:, :, ky, kx], xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], y) for ky in range(5) for kx in range(5)]
    if kind == "tconv":
        y = np.zeros((w.shape[1], 2 * H + 3, 2 * W + 3), dtype)
        return y, (slice(None), slice(1, 1 + 2 * H), slice(1, 1 + 2 * W)), [(w[:, :, ky, kx].T, x, y[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2]) for ky in range(5) for kx in range(5)]
    xp = np.zeros((1, H + 6, W + 6), dtype)
    xp[:, 3:3 + H, 3:3 + W] = x
    y = np.zeros((2, H, W), dtype)
    return y, (slice(None), slice(None), slice(None)), [(w[:, :, ky, kx], xp[:, 2 * ky:2 * ky + H, 2 * kx:2 * kx + W], y) for ky in range(4) for kx in range(4)]


def contract64(kind, x, w):
    """the contraction in float64"""
    y, crop, taps = _taps(kind, x, w, np.float64)
    for wt, xs, ys in taps:
        ys += (np.ascontiguousarray(wt) @ np.ascontiguousarray(xs).reshape(xs.shape[0], -1)).reshape(ys.shape)
    return y[crop]


def contract32_seq(kind, x, w, reverse=False):
    """the same products accumulated in fp32 one term at a time, tap-major (channel inner): the pessimistic order among fp32 orders.  Each product is rounded to fp32
    first (a no-op when both factors are halves).  reverse: the terms in the opposite order (another correct kernel, for the CPU tests)."""
    if kind == "tconv":
        return _tconv32_seq(x, w, reverse)
    y, crop, taps = _taps(kind, x, w, np.float32)
    tmp = np.empty_like(y)
    for wt, xs, ys in (taps[::-1] if reverse else taps):
        xs = np.ascontiguousarray(xs)
        for ci in (range(xs.shape[0] - 1, -1, -1) if reverse else range(xs.shape[0])):
            np.multiply(wt[:, ci, None, None], xs[ci], out=tmp)
            ys += tmp
    return y[crop]


def _tconv32_seq(x, w, reverse):
    """contract32_seq for the transposed convolution: an output element belongs to one parity class (ky & 1, kx & 1), so each class accumulates in a buffer of its own
    (contiguous rows) in the same tap-major order, and the classes are interleaved at the end"""
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    cin, H, W = x.shape
    cout = w.shape[1]
    cls = [[np.zeros((cout, H + 2, W + 2), np.float32) for _ in range(2)] for _ in range(2)]      # class (py, px): padded output row 2 r + py, column 2 c + px
    tmp = np.empty((cout, H, W), np.float32)
    order = [(ky, kx) for ky in range(5) for kx in range(5)]
    for ky, kx in (order[::-1] if reverse else order):
        ys = cls[ky & 1][kx & 1][:, ky >> 1:(ky >> 1) + H, kx >> 1:(kx >> 1) + W]
        wt = np.ascontiguousarray(w[:, :, ky, kx])
        for ci in (range(cin - 1, -1, -1) if reverse else range(cin)):
            np.multiply(wt[ci][:, None, None], x[ci], out=tmp)
            ys += tmp
    y = np.empty((cout, 2 * H + 4, 2 * W + 4), np.float32)
    for py in range(2):
        for px in range(2):
            y[:, py::2, px::2] = cls[py][px]
    return y[:, 1:1 + 2 * H, 1:1 + 2 * W]


def n_terms(kind, cin):
    return 16 if kind == "head" else 25 * cin


# ------------------------------------------------------------------------------------------- operands
def enc_operand(raw, scale, shift, kind, cell):
    """Operand of an encoder layer from the stored conv + bias of the layer before it.
    -> (f, a, d, eps): f = act_E(bn(raw)) in float64, eps the allowance of its fp32 evaluation, a = RN16(f), d >= |true operand - a| for every operand a correct
    kernel could have staged:
    cell=False  the kernel rounds f32(act_E(bn(raw))) of the stored fp32 raw: d != 0 only where f lies within the fp32 evaluation allowance of a rounding tie
    cell=True   the kernel rounded f32(act_E(bn(v))) of its own fp32 v, of which the tap keeps RN16(v) = raw: v anywhere in the rounding cell of raw"""
    raw = np.asarray(raw, np.float64)
    sc, sh = scale[:, None, None], shift[:, None, None]
    assert (scale > 0).all()                                     # monotone: the cell's image is bounded by the images of its ends
    r = ulp16(raw) / 2 if cell else 0.0
    f = act64(sc * raw + sh, kind)
    a = rn16(f)
    lo, hi = act64(sc * (raw - r) + sh, kind), act64(sc * (raw + r) + sh, kind)
    eps = C_EPI * EPS32 * (np.abs(sc) * (np.abs(raw) + r) + np.abs(sh) + np.maximum(np.abs(lo), np.abs(hi)) + (1.0 if kind == ELU else 0.0))
    d = np.maximum(rn16(hi + eps) - a, a - rn16(lo - eps))
    return f, a, d, eps


# ------------------------------------------------------------------------------------------- reference layers
class Ref:
    """float64 value of one layer, its allowance E, and whether the output is stored as a half.
    u: the per-element unit of tests/fp32_layer_ref.py - the same allowance evaluated with ONE accumulated term (K = 1), so that z = (got - ref) / u measures an
    error in roundings of the element's own accumulation scale; acc: the part of E that the accumulation contributes (K 2^-24 A, BN-scaled in the decoder), which
    the Winograd kernels replace by the bound of their bilinear algorithm"""

    def __init__(self, ref, E, half, share=0.0, sigma=None, u=None, acc=None):
        self.ref, self.E, self.half, self.share, self.sigma, self.u, self.acc = ref, E, half, share, sigma, u, acc


def enc_ref(a, d, w, b, *, w_half=True, fp32_products=False, out_half=True):
    """conv5x5_s2(a, w) + b; a = operands (float64), d = their ambiguity (or None), stored output = raw conv + bias"""
    w = rn16(w) if w_half else np.asarray(w, np.float64)
    bb = b[:, None, None]
    ref = contract64("conv", a, w) + bb
    A = contract64("conv", np.abs(a), np.abs(w)) + np.abs(bb)
    K = n_terms("conv", a.shape[0]) + (1 if fp32_products else 0)
    E = (K + C_EPI) * EPS32 * A
    u, acc = (1 + C_EPI) * EPS32 * A, K * EPS32 * A
    share, sigma = 0.0, None
    if d is not None:
        E = E + contract64("conv", d, np.abs(w))
        share = float((d > 0).mean())
        if out_half and share > 0.01:
            # operands known only up to d: the error's scale is no longer the output's own ulp.  Standard deviation of one element under operands spread evenly
            # over +-d and an evenly spread output rounding; check C then measures in these units (see LayerLocal.enc)
            sigma = np.sqrt(contract64("conv", d * d, w * w) / 3 + ulp16(ref) ** 2 / 12)
    return Ref(ref, E, out_half, share, sigma, u, acc)


def dec_ref(x, w, b, scale, shift, kind, *, w_half=True, fp32_products=False, out_half=True):
    """bn(act_D(tconv5x5_s2(x, w) + b)): activation BEFORE BN"""
    w = rn16(w) if w_half else np.asarray(w, np.float64)
    bb, sc, sh = b[:, None, None], scale[:, None, None], shift[:, None, None]
    t = contract64("tconv", x, w) + bb
    A = contract64("tconv", np.abs(x), np.abs(w)) + np.abs(bb)
    v = act64(t, kind)
    ref = sc * v + sh
    K = n_terms("tconv", x.shape[0]) + (1 if fp32_products else 0)
    e_t = (K + 1) * EPS32 * A                                    # the activations' slopes are <= 1
    e_epi = C_EPI * EPS32 * ((1.0 if kind == ELU else 0.0) + np.abs(v) + np.abs(sc * v) + np.abs(sh) + np.abs(ref))
    E = np.abs(sc) * e_t + e_epi
    return Ref(ref, E, out_half, u=np.abs(sc) * (1 + 1) * EPS32 * A + e_epi, acc=np.abs(sc) * K * EPS32 * A)


def head_ref(up6, w, b):
    """sigmoid(conv4x4_d2(up6, w) + b), fp32 throughout: the pre-activation's allowance passes through the logistic's slope <= 1/4; the logistic itself is one
    v_exp_f32, one add, one v_rcp_f32 (1 ulp) and one multiply on values <= 2: 8 * 2^-24"""
    x = np.asarray(up6, np.float64).reshape(1, *up6.shape[-2:])
    w4 = np.asarray(w, np.float64).reshape(2, 1, 4, 4)
    bb = b[:, None, None]
    pre = contract64("head", x, w4) + bb
    A = contract64("head", np.abs(x), np.abs(w4)) + np.abs(bb)
    with np.errstate(over="ignore"):
        ref = 1.0 / (1.0 + np.exp(-pre))
    return Ref(ref, (16 + 2) * EPS32 * A / 4 + 8 * EPS32, False, u=(1 + 2) * EPS32 * A / 4 + 8 * EPS32, acc=16 * EPS32 * A / 4)


# ------------------------------------------------------------------------------------------- emulation of a correct kernel
def enc_emulate(a, w, b, scale, shift, kind, *, w_half=True, reverse=False):
    """-> (v, raw, act): v = fp32 conv + bias; the two tensors a correct fp16-storage kernel stores from it: raw = RN16(v), act = RN16(f32 act_E(bn(v)))"""
    w = rn16(w) if w_half else w
    v = contract32_seq("conv", a, w, reverse) + np.asarray(b, np.float32)[:, None, None]
    act = None
    if scale is not None:
        act = rn16(act32(np.asarray(scale, np.float32)[:, None, None] * v + np.asarray(shift, np.float32)[:, None, None], kind))
    return v, rn16(v), act


def dec_emulate(x, w, b, scale, shift, kind, *, w_half=True, reverse=False):
    """-> fp32 bn(act_D(tconv + b)) before the store's rounding"""
    w = rn16(w) if w_half else w
    t = contract32_seq("tconv", x, w, reverse) + np.asarray(b, np.float32)[:, None, None]
    return np.asarray(scale, np.float32)[:, None, None] * act32(t, kind) + np.asarray(shift, np.float32)[:, None, None]


# ------------------------------------------------------------------------------------------- the checks
def check_a(got, r):
    """per element, no exceptions: |got - ref| <= ulp16(max(|got|, |ref|)) / 2 + E (without the half-ulp term for a tensor stored fp32)
    -> (number of violations, worst |got - ref| / bound, index of the worst)"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - r.ref)
    bound = r.E + (ulp16(np.maximum(np.abs(got), np.abs(r.ref))) / 2 if r.half else 0.0)
    ratio = err / bound
    ratio[~np.isfinite(got)] = np.inf
    k = int(np.argmax(ratio))
    return int((ratio > 1).sum()), float(ratio.flat[k]), np.unravel_index(k, ratio.shape)


def rate_b(got, ref):
    """share of elements that are not the half nearest to the reference"""
    return float((np.asarray(got, np.float64) != rn16(ref)).mean())


def rms_c(got, ref, sigma=None):
    """RMS of (got - ref) / ulp16(ref) over |ref| >= 2^-14; with sigma: RMS of (got - ref) / sigma over every element"""
    if sigma is not None:
        return float(np.sqrt(np.mean(((np.asarray(got, np.float64) - ref) / sigma) ** 2)))
    m = np.abs(ref) >= 2.0 ** -14
    if not m.any():
        return 0.0
    return float(np.sqrt(np.mean(((np.asarray(got, np.float64)[m] - ref[m]) / ulp16(ref[m])) ** 2)))


def cap_b(rate_emu, n):
    """twice the emulation's own rate plus three standard errors of that rate at the sample size (the factor 2: the MFMA's order is not the emulation's)"""
    p = max(rate_emu, 1.0 / n)
    return 2.0 * rate_emu + 3.0 * np.sqrt(p * (1.0 - min(p, 1.0)) / n)


CAP_C = 1.05


def flushed(got, r):
    """elements stored as zero whose reference is further from zero than half the subnormal spacing plus the allowance: a store that flushes subnormals"""
    return int(((np.asarray(got) == 0) & (np.abs(r.ref) - r.E > 2.0 ** -25)).sum())


# ------------------------------------------------------------------------------------------- one instance, layer by layer
class LayerLocal:
    """References and yardsticks of one instance (stem, tile) from the tensors stored for it.
    taps: name -> array (conv1..conv6, up1..up6) as Engine.tensor returns them; x [2][T][F] the instance's input; mode: the stem mode (0: LeakyReLU / ReLU, 1: ELU / ELU)
    act16: the tensors are stored as halves (fp16-storage mode on F % 256 == 0); down1_f16: down1 ran on the fp16 MFMA (srt_down1_f16_kernel)
    f32_layers: layers (down2..down6, up1..up5) that ran on the fp32 MFMA kernels (srt_enc_mfma / srt_dec_mfma: widths the fp16 kernels do not take, tensors kept
    fp32 only): fp32 operands - the encoder's act_E(bn(raw)) evaluated in fp32 and not rounded - fp32 weights, products rounded in fp32
    enc(i) / dec(i) -> (Ref, yard): yard = (rate B, RMS C) of the emulation of a correct kernel on the same layer and inputs, None for a tensor stored fp32."""

    def __init__(self, C, mode, x, taps, act16, down1_f16, f32_layers=()):
        self.C, self.x, self.taps, self.act16, self.d1f16 = C, np.asarray(x, np.float64), taps, act16, down1_f16
        self.f32 = set(f32_layers) | (set() if down1_f16 else {"down1"}) | (set() if act16 else {"up6"})
        assert not (act16 and self.f32 - {"down1"})
        self.actE, self.actD = (ELU, ELU) if mode else (LEAKY, RELU)
        self._centre = {}

    def _enc_args(self, i):
        return dict(w_half="down%d" % i not in self.f32)

    def _operand(self, i, raw_prev=None):
        """(a, d) of encoder layer i; raw_prev overrides the tap (the yardstick's own chain)"""
        if i == 1:
            return (rn16(np.minimum(self.x, HMAX)) if self.d1f16 else self.x), None
        L = self.C.enc[i - 2]
        raw = self.taps["conv%d" % (i - 1)] if raw_prev is None else raw_prev
        f, a, d, eps = enc_operand(raw, L["scale"], L["shift"], self.actE, cell=self.act16)
        return (f, eps) if "down%d" % i in self.f32 else (a, d)

    def _emu_centre(self, i):
        """layer i emulated from the operands at the centre of what the taps allow: (v, raw, act) with the joint statistics of a correct kernel's two outputs"""
        if i not in self._centre:
            L = self.C.enc[i - 1]
            self._centre[i] = enc_emulate(self._operand(i)[0], L["w"], L["b"], L.get("scale"), L.get("shift"), self.actE, **self._enc_args(i))
        return self._centre[i]

    def enc(self, i):
        L = self.C.enc[i - 1]
        a, d = self._operand(i)
        f32p = "down%d" % i in self.f32
        ref = enc_ref(a, d, L["w"], L["b"], fp32_products=f32p, out_half=self.act16, **self._enc_args(i))
        if f32p:
            ref.share = 0.0                                      # (d is the evaluation allowance of an unrounded operand there, not an ambiguity)
        if not self.act16:
            return ref, None
        if i == 1:
            got_e, ref_e = self._emu_centre(i)[1], ref.ref
        else:
            # the operand a correct kernel stages is not a function of the tap: the yardstick runs the PAIR of layers - layer i - 1 emulated from its own operands
            # gives (raw', act') as a kernel stores them, layer i is emulated on act' and held to the float64 layer fed raw', exactly as the GPU's is
            _, raw_p, act_p = self._emu_centre(i - 1)
            got_e = enc_emulate(act_p, L["w"], L["b"], None, None, self.actE)[1]
            r_e = enc_ref(*self._operand(i, raw_p), L["w"], L["b"])
            return ref, (rate_b(got_e, r_e.ref), rms_c(got_e, r_e.ref, r_e.sigma))
        return ref, (rate_b(got_e, ref_e), rms_c(got_e, ref_e))

    def dec_input(self, i):
        if i == 1:
            x = self.taps["conv6"]
        else:
            x = np.concatenate([self.taps["conv%d" % (7 - i)], self.taps["up%d" % (i - 1)]])      # the raw skip tensor is the LOW channels
        x = np.asarray(x, np.float64)
        if not self.act16 and "up%d" % i not in self.f32:
            x = rn16(x)                                          # srt_dec_f16 on fp32 tensors rounds while staging
        return x

    def dec(self, i, x=None):
        L = self.C.dec[i - 1]
        x = self.dec_input(i) if x is None else x
        f32 = "up%d" % i in self.f32                             # (up6 on fp32 tensors: the fp32 MFMA, fp32 weights)
        half = self.act16 and i < 6
        ref = dec_ref(x, L["w"], L["b"], L["scale"], L["shift"], self.actD, w_half=not f32, fp32_products=f32, out_half=half)
        if not half:
            return ref, None
        got_e = rn16(dec_emulate(x, L["w"], L["b"], L["scale"], L["shift"], self.actD))
        return ref, (rate_b(got_e, ref.ref), rms_c(got_e, ref.ref))

    def head(self):
        return head_ref(self.taps["up6"], self.C.head_w, self.C.head_b), None


def judge(got, ref, yard):
    """-> dict of the measured figures and the list of failed checks"""
    n, worst, where = check_a(got, ref)
    out = dict(a_viol=n, a_worst=worst, a_where=where, share=ref.share, fail=[], subnormal=float((np.abs(ref.ref) < 2.0 ** -14).mean()))
    if n:
        out["fail"].append("A")
    if yard is not None:
        b, c = rate_b(got, ref.ref), rms_c(got, ref.ref, ref.sigma)
        # sigma units: the yardstick's operands are its own draw, not the GPU's, so the two RMS values are independent estimates, each with a relative standard
        # error of 1 / sqrt(2 n) (near-normal errors): three standard errors of their ratio on top of the cap.  In ulp units both see the same operands: no such term.
        c_cap = CAP_C * yard[1] * (1.0 + (3.0 / np.sqrt(ref.ref.size) if ref.sigma is not None else 0.0))
        out.update(b=b, b_emu=yard[0], b_cap=cap_b(yard[0], ref.ref.size), c=c, c_emu=yard[1], c_cap=c_cap, flushed=flushed(got, ref))
        if b > out["b_cap"] and ref.sigma is None:              # (operands known only up to d: most elements are not the nearest half of the centre's value; reported, not held)
            out["fail"].append("B")
        if c > out["c_cap"]:
            out["fail"].append("C")
    return out


def emulate_network(C, mode, x, down1_f16=False, reverse=True):
    """A correct fp16-storage network, layer by layer, on the emulation: the stand-in for the GPU in the CPU tests.  -> (taps, mask, hidden): hidden["actN"] is
    the encoder operand no tap returns, hidden["vN"] the fp32 conv + bias both stored tensors were rounded from.  reverse: accumulate in the opposite order to the
    yardstick's, as a kernel's order is not the yardstick's either."""
    actE, actD = (ELU, ELU) if mode else (LEAKY, RELU)
    taps, hidden = {}, {}
    a = rn16(np.minimum(x, HMAX)) if down1_f16 else np.asarray(x, np.float64)
    for i in range(1, 7):
        L = C.enc[i - 1]
        hidden["v%d" % i], raw, a = enc_emulate(a, L["w"], L["b"], L.get("scale"), L.get("shift"), actE, w_half=not (i == 1 and not down1_f16), reverse=reverse)
        taps["conv%d" % i] = raw.astype(np.float32)
        hidden["act%d" % i] = a
    u = taps["conv6"].astype(np.float64)
    for i in range(1, 7):
        L = C.dec[i - 1]
        u = dec_emulate(u, L["w"], L["b"], L["scale"], L["shift"], actD, reverse=reverse)
        u = rn16(u) if i < 6 else u.astype(np.float64)
        taps["up%d" % i] = u.astype(np.float32)
        if i < 6:
            u = np.concatenate([taps["conv%d" % (6 - i)].astype(np.float64), u])
    pre = contract32_seq("head", taps["up6"].reshape(1, *x.shape[1:]), C.head_w.reshape(2, 1, 4, 4)) + C.head_b.astype(np.float32)[:, None, None]
    mask = (np.float32(1) / (np.float32(1) + np.exp(-pre))).astype(np.float32)
    return taps, mask, hidden


def forward64(C, mode, x, operand_half):
    """The whole network out of the float64 layers above -> (taps, mask).  operand_half=False: the fp32 network in float64, which the oracle's taps pin (padding,
    parity, concat order, activation before BN); True: operands and weights rounded to halves (the chain that drifts from the GPU - not used as a reference)."""
    q = rn16 if operand_half else (lambda v: np.asarray(v, np.float64))
    actE, actD = (ELU, ELU) if mode else (LEAKY, RELU)
    taps = {}
    a = q(x)
    for i in range(1, 7):
        L = C.enc[i - 1]
        raw = contract64("conv", a, q(L["w"])) + L["b"][:, None, None]
        taps["conv%d" % i] = raw
        if i < 6:
            taps["act%d" % i] = act64(L["scale"][:, None, None] * raw + L["shift"][:, None, None], actE)
            a = q(taps["act%d" % i])
    u = q(taps["conv6"])
    for i in range(1, 7):
        L = C.dec[i - 1]
        u = L["scale"][:, None, None] * act64(contract64("tconv", u, q(L["w"])) + L["b"][:, None, None], actD) + L["shift"][:, None, None]
        taps["up%d" % i] = u
        if i < 6:
            u = q(np.concatenate([taps["conv%d" % (6 - i)], u]))
    pre = contract64("head", u, C.head_w.reshape(2, 1, 4, 4)) + C.head_b[:, None, None]
    return taps, 1.0 / (1.0 + np.exp(-pre))
