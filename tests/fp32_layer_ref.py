"""fp32 emulations of a correct kernel for the fp32-class kernel families, the unit z is measured in, and the checks A32 / C32 / D32 of tests/test_fp32_layer_local.py.

The float64 layers, the per-element allowances E and the unit u are those of tests/fp16_layer_ref.py (LayerLocal(act16=False, f32_layers=every layer): fp32 weights,
fp32 products, the encoder's operand act_E(bn(raw)) of the stored fp32 `raw`).  Every layer is evaluated ALONE on the tensors the engine stored as its inputs.

Norm
  u    the layer's allowance with ONE accumulated term (Ref.u): encoder (1 + C_EPI) 2^-24 (sum|w||a| + |b|); decoder |sc| 2 2^-24 (sum|w||x| + |b|) + the C_EPI epilogue
       terms; head 3 2^-24 (sum|w||x| + |b|) / 4 + 8 2^-24.  z = (got - ref64) / u: an error counted in roundings at the element's own accumulation scale.
  A32  |got - ref64| <= E per element, no exceptions (fp16_layer_ref.check_a without the half-ulp term); where a Winograd kernel ran, the accumulation part of E is the
       bound of the bilinear algorithm (below).  A backstop for gross local faults; a non-finite value fails it.
  C32  RMS(z_gpu) <= 1.05 RMS(z_emu)            D32  max|z_gpu| <= 2 max|z_emu|
       z_emu: the emulation below of the family that ran, on the same layer and inputs.  Nothing comes from a GPU result.

What each family rounds, and its emulation (numpy fp32 throughout)
  direct    srt_enc_mfma / srt_enc_mfma2 / srt_dec_mfma / srt_dec_mfma2, their split-K launches, the naive kernels, the streamed down1 and up6, the head kernels.
            Operand: act32(scale * raw + shift) in the device's operation order (srt_device.h, contraction off); down1 reads x, the decoder its stored inputs.
            Products and sums in fp32; emulated one term at a time, every product rounded, in the kernel's own K order (contract32_cm): channel-group-major - the
            naive kernels walk ci outside ky, kx; every v_mfma_f32_32x32x2_f32 kernel walks channel PAIRS outside the 25 taps (srt_enc_mfma2 / srt_dec_mfma2: cp, tap),
            srt_dec16_kernel k-quads; up6 (one MFMA chain over the channels per tap, the taps gathered ascending) is tap-major (contract32_seq).  The order matters:
            two sequential orders of one layer differ by up to 29 % in RMS z.  The kernels do not round their products (FMA / MFMA), the emulation does.  Epilogue: + bias (encoder); bn(act32(. + bias)) (decoder); the logistic of . + bias (head:
            srt_sigmoid_fast in the product kernels, the libm form in the naive one).  The exponential of ELU and of the fast logistic is __expf = v_exp_f32(x * log2e):
            its argument is a rounded fp32 product, which exp_dev models; the instruction itself and v_rcp_f32 are taken correctly rounded (their best case).
  Winograd  srt_dec_wino / srt_dec_wino32 / srt_enc_wino32 (csrc/srt_nn4.hip).  U as srt_pack_wino_kernel forms it: the x transform of every kernel row, then y, with
            wino_w1d's association 0.5f * ((g0 + g2) +- g1); 2-tap class: decoder [g0, 0.5f (g0 + g1), 0.5f (g0 - g1)], encoder [g0, g0 + g1, g1].  V as wino_in3 /
            wino_in2 form it, x then y.  The 49 products accumulated over Cin one channel at a time.  Y as wino_out2d forms it ((m0 + m1) + m2, (m1 - m2) - m3; x then
            y).  Decoder: the direct epilogue per class; encoder: ((C11 + C10) + (C01 + C00)) + bias.  The encoder's operand is the act(bn(raw)) copy the producing
            kernel wrote from its own fp32 v = raw, the same expression as the direct operand.
  f16x2     srt_enc_f16<.., 2> / srt_dec_f16<.., 2> (csrc/srt_nn3.hip, down2..down6 and up1..up5 of PREC_F16X2; down1, up6 and the head stay direct).  srt_split:
            hi = RN16(x), lo = RN16(x - hi) of the fp32 operand (the encoder's: act32(bn(raw)) first); weights RN16(w), which the engine only accepts when that is w
            itself.  Two v_mfma_f32_32x32x16_f16 per tap and 16-channel group, hi then lo: half x half is exact in fp32, the sums are fp32.  Emulated as the direct
            contraction over the 2 Cin operands (hi_0, lo_0, hi_1, lo_1, ..).  Operand precision this leaves: hi + lo keeps 22 significant bits of x,
            |x - (hi + lo)| <= 2^-22 |x| while lo is a normal half, |x| >= 2^-3; below that lo is a subnormal half with spacing 2^-24, so |x - (hi + lo)| <= 2^-25
            absolute: about 12 significant bits at |x| = 2^-13.  (|x| > 65504 overflows hi; the network's tensors stay far below.)  A32 carries sum |w| d for it.

Winograd worst case (A32).  A bilinear algorithm y = A^T [(G g G^T) . (B^T d B)] A evaluated in floating point satisfies
  |y_computed - y| <= (Cin + c) 2^-24 |A|^T [ sum_ci |U| . (|B|^T |d| |B|) ] |A|     (first order; every matrix by absolute value, |G| |g| |G|^T >= |U|)
with c the roundings one term passes through outside the sum over Cin:
  U  2 per axis ((g0 + g2), +- g1; the halving is exact)   4        V  1 per axis                    2        the product                     1
  Y  2 per axis (two additions)                            4        encoder only: the class sums     2
so c = 11 for the decoder and c = 13 for the encoder.  The bias addition and the epilogue keep the terms they have in the direct allowance.
"""
import numpy as np

import fp16_layer_ref as R

EPS32, C_EPI, CAP_C, CAP_D = R.EPS32, R.C_EPI, R.CAP_C, 2.0
ENC = ["down%d" % i for i in range(1, 7)]
DEC = ["up%d" % i for i in range(1, 7)]
C_WINO_DEC, C_WINO_ENC = 11, 13
F32 = np.float32


# ------------------------------------------------------------------------------------------- Winograd, in the kernels' association
def _w1d(p, g, enc, half):
    """wino_w1d: g = the five taps of one axis (arrays); p = 1: 3-tap class, p = 0: 2-tap class"""
    if p:
        g0, g1, g2 = (g[0], g[2], g[4]) if enc else (g[4], g[2], g[0])
        return [g0, half * ((g0 + g2) + g1), half * ((g0 + g2) - g1), g2]
    g0, g1 = (g[1], g[3]) if enc else (g[3], g[1])
    return [g0, g0 + g1, g1] if enc else [g0, half * (g0 + g1), half * (g0 - g1)]


def _in1d(p, d, enc):
    """wino_in3 / wino_in2"""
    if p:
        return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    return [d[0] - d[1], d[1], d[1] - d[2]] if enc else [d[0] - d[2], d[1] + d[2], d[2] - d[1]]


def _out1d(m, enc):
    """wino_out1d"""
    if len(m) == 4:
        return (m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]
    return (m[0] + m[1], m[1] - m[2]) if enc else ((m[0] + m[1]) + m[2], m[1] - m[2])


def _abs1d(kind, p, v, enc):
    """the same three transforms with every matrix entry by absolute value (the worst-case bound)"""
    if kind == "w":
        if p:
            g0, g1, g2 = (v[0], v[2], v[4]) if enc else (v[4], v[2], v[0])
            return [g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 + g1 + g2), g2]
        g0, g1 = (v[1], v[3]) if enc else (v[3], v[1])
        return [g0, g0 + g1, g1] if enc else [g0, 0.5 * (g0 + g1), 0.5 * (g0 + g1)]
    if kind == "in":
        if p:
            return [v[0] + v[2], v[1] + v[2], v[1] + v[2], v[1] + v[3]]
        return [v[0] + v[1], v[1], v[1] + v[2]] if enc else [v[0] + v[2], v[1] + v[2], v[1] + v[2]]
    if len(v) == 4:
        return v[0] + v[1] + v[2], v[1] + v[2] + v[3]
    return (v[0] + v[1], v[1] + v[2]) if enc else (v[0] + v[1] + v[2], v[1] + v[2])


def _two_axes(f, grid):
    """f along x for every row of grid[y][x], then along y for every resulting column -> out[i][j]"""
    rows = [f("x", r) for r in grid]
    cols = [f("y", [r[j] for r in rows]) for j in range(len(rows[0]))]
    return [[cols[j][i] for j in range(len(cols))] for i in range(len(cols[0]))]


def wino(kind, x, w, dtype=F32, reverse=False, bound=False, flip=None, chunk=1):
    """The contraction of `kind` ("conv": encoder, w [Cout][Cin][5][5]; "tconv": decoder, w [Cin][Cout][5][5]) in the Winograd form of csrc/srt_nn4.hip, in `dtype`.
    reverse: the channels accumulated in the opposite order.  bound: every transform by absolute value on |x|, |w| -> |A| (sum |U| . |B||d||B|^T) |A|^T.
    flip = (py, px, i, j, block row): that transform point of that class with the wrong sign on one row of blocks (a planted error).
    chunk > 1: the order of an MFMA chain - `chunk` channels' products summed unrounded, one rounded sum added per step, channels ascending."""
    enc = kind == "conv"
    x = np.asarray(np.abs(x) if bound else x, dtype)
    w = np.asarray(np.abs(w) if bound else w, dtype)
    if not enc:
        w = w.transpose(1, 0, 2, 3)                              # -> [Cout][Cin][ky][kx]
    cout, cin, H, W = w.shape[0], w.shape[1], x.shape[1], x.shape[2]
    half = dtype(0.5)
    if enc:
        assert H % 4 == 0 and W % 4 == 0
        nby, nbx = H // 4, W // 4
        xp = np.zeros((cin, H + 8, W + 8), dtype)
        y = np.zeros((cout, H // 2, W // 2), dtype)
    else:
        assert H % 2 == 0 and W % 2 == 0
        nby, nbx = H // 2, W // 2
        xp = np.zeros((cin, H + 4, W + 4), dtype)
        y = np.empty((cout, 2 * H, 2 * W), dtype)
    xp[:, 1:1 + H, 1:1 + W] = x
    step = 4 if enc else 2
    parts = []
    for py in (1, 0):
        for px in (1, 0):
            pp = {"x": px, "y": py}
            g = [[w[:, :, ky, kx] for kx in range(5)] for ky in range(5)]
            if bound:
                U = _two_axes(lambda ax, v: _abs1d("w", pp[ax], v, enc), g)
            else:
                U = _two_axes(lambda ax, v: _w1d(pp[ax], v, enc, half), g)
            # patch value (i, j) of every block: decoder rows a0 - 1 + i; encoder every second row of the block's 7-row patch, from its first (odd plane) or second
            oy, ox = ((1 - py, 1 - px) if enc else (0, 0))
            d = [[xp[:, oy + (2 if enc else 1) * i: oy + (2 if enc else 1) * i + step * nby: step, ox + (2 if enc else 1) * j: ox + (2 if enc else 1) * j + step * nbx: step]
                  for j in range(4)] for i in range(4)]
            if bound:
                V = _two_axes(lambda ax, v: _abs1d("in", pp[ax], v, enc), d)
            else:
                V = _two_axes(lambda ax, v: _in1d(pp[ax], v, enc), d)
            ny, nx = len(U), len(U[0])
            Us = np.stack([U[i][j] for i in range(ny) for j in range(nx)])                                       # [P][Cout][Cin]
            Vs = np.stack([V[i][j] for i in range(ny) for j in range(nx)]).reshape(ny * nx, cin, nby * nbx)     # [P][Cin][blocks]
            if flip is not None and (py, px) == flip[:2]:
                Vs = Vs.copy().reshape(ny * nx, cin, nby, nbx)
                Vs[flip[2] * nx + flip[3], :, flip[4]] *= -1
                Vs = Vs.reshape(ny * nx, cin, nby * nbx)
            if bound or dtype is np.float64:
                M = np.einsum("poc,pcb->pob", Us, Vs)
            else:
                M = np.zeros((ny * nx, cout, nby * nbx), dtype)
                tmp = np.empty_like(M)
                Ut = np.ascontiguousarray(Us.transpose(2, 0, 1))                                                 # [Cin][P][Cout]
                Vt = np.ascontiguousarray(Vs.transpose(1, 0, 2))                                                 # [Cin][P][blocks]
                if chunk > 1:
                    for c0 in range(0, cin, chunk):
                        M += np.einsum("cpo,cpb->pob", Ut[c0:c0 + chunk].astype(np.float64), Vt[c0:c0 + chunk].astype(np.float64)).astype(dtype)
                else:
                    for ci in (range(cin - 1, -1, -1) if reverse else range(cin)):
                        np.multiply(Ut[ci][:, :, None], Vt[ci][:, None, :], out=tmp)
                        M += tmp
            m = [[M[i * nx + j].reshape(cout, nby, nbx) for j in range(nx)] for i in range(ny)]
            if bound:
                Y = _two_axes(lambda ax, v: _abs1d("out", None, v, enc), m)
            else:
                Y = _two_axes(lambda ax, v: _out1d(v, enc), m)
            if enc:
                parts.append(Y)
            else:
                for da in range(2):
                    for db in range(2):
                        y[:, 2 * da + py::4, 2 * db + px::4] = Y[da][db]
    if enc:
        for da in range(2):
            for db in range(2):
                y[:, da::2, db::2] = (parts[0][da][db] + parts[1][da][db]) + (parts[2][da][db] + parts[3][da][db])
    return y


def keep_bits(v, bits):
    """fp32 values rounded to `bits` significant bits (planted errors: weights / operands kept short)"""
    m, e = np.frexp(np.asarray(v, np.float64))
    return np.ldexp(np.round(np.ldexp(m, bits)), e - bits).astype(F32)


# ------------------------------------------------------------------------------------------- f16x2
def split16(x):
    """srt_split on fp32 values -> (hi, lo) as float32 arrays"""
    x = np.asarray(x, F32)
    hi = x.astype(np.float16).astype(F32)
    lo = (x - hi).astype(np.float16).astype(F32)
    return hi, lo


def split_gap(f, eps=0.0):
    """>= |operand a correct f16x2 kernel stages - f| for an operand known as f +- eps: 2^-22 |f| while lo is a normal half, 2^-25 below"""
    return eps + np.maximum(2.0 ** -22 * (np.abs(f) + eps), 2.0 ** -25)


def _interleave(hi, lo):
    out = np.empty((2 * hi.shape[0],) + hi.shape[1:], F32)
    out[0::2], out[1::2] = hi, lo
    return out


def contract32_chunk(kind, x, w, chunk=4, cmajor=False):
    """another correct kernel: a blocked order.  Channels ascending in steps of `chunk`; the products of a step are summed unrounded (float64, rounded once) and the
    accumulator takes one rounded addition per step.  Tap-major, or (cmajor) the steps outside the taps as in contract32_cm"""
    y, crop, taps = R._taps(kind, x, w, F32)
    taps = [(np.asarray(wt, np.float64), np.ascontiguousarray(xs, np.float64), ys) for wt, xs, ys in taps]
    steps = list(range(0, taps[0][1].shape[0], chunk))
    for c0, (wt, xs, ys) in ([(c, t) for c in steps for t in taps] if cmajor else [(c, t) for t in taps for c in steps]):
        ys += np.einsum("oc,chw->ohw", wt[:, c0:c0 + chunk], xs[c0:c0 + chunk]).astype(F32)
    return y[crop]


def contract32_cm(kind, x, w, group=1, reverse=False):
    """The products accumulated in fp32 one term at a time like contract32_seq, but channel-group-major, the K order of the direct kernels: groups of `group` input
    channels ascending, inside a group the taps ascending, inside a tap the group's channels.  group = 1: the naive kernels (ci outer, ky, kx inner); 2: every
    v_mfma_f32_32x32x2_f32 kernel (cp outer, tap inner, the k-pair = two channels of one tap); 4: srt_dec16_kernel (k-quads).  reverse: everything backwards."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    cin = x.shape[0]
    if kind == "tconv":
        H, W = x.shape[1:]
        cout = w.shape[1]
        cls = [[np.zeros((cout, H + 2, W + 2), F32) for _ in range(2)] for _ in range(2)]
        taps = [(np.ascontiguousarray(w[:, :, ky, kx]), x, cls[ky & 1][kx & 1][:, ky >> 1:(ky >> 1) + H, kx >> 1:(kx >> 1) + W]) for ky in range(5) for kx in range(5)]
        tmp = np.empty((cout, H, W), F32)
        wsel = lambda wt, ci: wt[ci][:, None, None]
    else:
        y, crop, tp = R._taps(kind, x, w, F32)
        taps = [(np.ascontiguousarray(wt), np.ascontiguousarray(xs), ys) for wt, xs, ys in tp]
        tmp = np.empty_like(y)
        wsel = lambda wt, ci: wt[:, ci, None, None]
    groups = [list(range(g0, min(g0 + group, cin))) for g0 in range(0, cin, group)]
    for g in (groups[::-1] if reverse else groups):
        for wt, xs, ys in (taps[::-1] if reverse else taps):
            for ci in (g[::-1] if reverse else g):
                np.multiply(wsel(wt, ci), xs[ci], out=tmp)
                ys += tmp
    if kind != "tconv":
        return y[crop]
    y = np.empty((cout, 2 * H + 4, 2 * W + 4), F32)
    for py in range(2):
        for px in range(2):
            y[:, py::2, px::2] = cls[py][px]
    return y[:, 1:1 + 2 * H, 1:1 + 2 * W]


def contract_f16x2(kind, x, w, reverse=False, drop_lo_tap=None, chunk=1):
    """hi and lo of every operand as two terms of the sequential fp32 contraction.  drop_lo_tap = (ky, kx): that tap reads hi alone (a planted error).
    chunk > 1: the kernel's own order instead - per tap and 16-channel group one step over the 16 hi products, then one over the 16 lo products"""
    hi, lo = split16(x)
    w = np.asarray(w, F32)
    if chunk > 1:
        cin = hi.shape[0]
        order = np.concatenate([np.concatenate([np.arange(c0, min(c0 + 16, cin)), cin + np.arange(c0, min(c0 + 16, cin))]) for c0 in range(0, cin, 16)])
        wo = order % cin
        return contract32_chunk(kind, np.concatenate([hi, lo])[order], w[:, wo] if kind == "conv" else w[wo], 16)
    w2 = np.repeat(w, 2, axis=1 if kind == "conv" else 0)
    if drop_lo_tap is not None:
        w2 = w2.copy()
        if kind == "conv":
            w2[:, 1::2, drop_lo_tap[0], drop_lo_tap[1]] = 0
        else:
            w2[1::2, :, drop_lo_tap[0], drop_lo_tap[1]] = 0
    return R.contract32_seq(kind, _interleave(hi, lo), w2, reverse)


# ------------------------------------------------------------------------------------------- emulated layers
def contract_emu(family, kind, x, w, reverse=False, chunk=1, group=None, **kw):
    """chunk = 1: the yardstick's order, one term at a time (direct: tap-major, or channel-group-major with `group`).  chunk > 1: the blocked order (the CPU tests'
    other correct kernel)"""
    if family == "wino":
        return wino(kind, x, w, F32, reverse, chunk=chunk, **kw)
    if family == "f16x2":
        return contract_f16x2(kind, x, w, reverse, chunk=chunk, **kw)
    if chunk > 1:
        return contract32_chunk(kind, x, w, chunk, cmajor=group is not None)
    return R.contract32_seq(kind, x, w, reverse) if group is None else contract32_cm(kind, x, w, group, reverse)


def exp_dev(x):
    """__expf(x) as hipcc emits it: v_exp_f32(x * log2e).  The argument is one rounded fp32 product - that alone moves the result by up to |x| 2^-24 of itself -
    and the instruction is taken at its best, the correctly rounded 2^arg (it is documented to 1 ulp)"""
    arg = np.asarray(x, F32) * F32(1.4426950408889634)
    return np.exp2(arg.astype(np.float64)).astype(F32)


def act32(x, kind):
    """fp16_layer_ref.act32 with the device's exponential"""
    x = np.asarray(x, F32)
    if kind != R.ELU:
        return R.act32(x, kind)
    return np.maximum(x, F32(0)) + (exp_dev(np.minimum(x, F32(0))) - F32(1))


def operand32(raw, scale, shift, kind):
    """the encoder's fp32 operand act32(scale * raw + shift) of the stored fp32 conv + bias of the layer before it"""
    return act32(np.asarray(scale, F32)[:, None, None] * np.asarray(raw, F32) + np.asarray(shift, F32)[:, None, None], kind)


def enc_emu(family, a, w, b, reverse=False, **kw):
    return contract_emu(family, "conv", a, w, reverse, **kw) + np.asarray(b, F32)[:, None, None]


def dec_emu(family, x, w, b, scale, shift, kind, reverse=False, **kw):
    t = contract_emu(family, "tconv", x, w, reverse, **kw) + np.asarray(b, F32)[:, None, None]
    return np.asarray(scale, F32)[:, None, None] * act32(t, kind) + np.asarray(shift, F32)[:, None, None]


def head_emu(up6, w, b, reverse=False, fast=True):
    """fast: srt_sigmoid_fast of the product head kernels - z = __expf(-|x|), r = v_rcp_f32(1 + z) (taken correctly rounded), x >= 0 ? r : z r;
    otherwise the naive kernel's libm form 1 / (1 + expf(-x)), expf(x) / (1 + expf(x))"""
    pre = R.contract32_seq("head", np.asarray(up6, F32).reshape(1, *up6.shape[-2:]), np.asarray(w, F32).reshape(2, 1, 4, 4), reverse) + np.asarray(b, F32)[:, None, None]
    z = exp_dev(-np.abs(pre)) if fast else np.exp(-np.abs(pre))
    if fast:
        r = F32(1) / (F32(1) + z)
        return np.where(pre >= 0, r, z * r)
    return np.where(pre >= 0, F32(1) / (F32(1) + z), z / (F32(1) + z))


# ------------------------------------------------------------------------------------------- one instance, layer by layer
class Local32:
    """References (float64, allowance E, unit u) and emulations of one instance from the tensors stored for it.
    family: layer name -> "direct" | "wino" | "f16x2" (default "direct"); group: layer name -> channel group of a direct kernel's K order (contract32_cm; default 2,
    the fp32 MFMA kernels; None: tap-major)"""

    def __init__(self, C, mode, x, taps, family=None, head_fast=True, group=None):
        self.C, self.x, self.taps, self.family, self.head_fast, self.group = C, np.asarray(x, np.float64), taps, dict(family or {}), head_fast, dict(group or {})
        self.LL = R.LayerLocal(C, mode, x, taps, act16=False, down1_f16=False, f32_layers=ENC[1:] + DEC[:5])
        self.actE, self.actD = self.LL.actE, self.LL.actD

    def fam(self, n):
        return self.family.get(n, "direct")

    def enc_operand32(self, i):
        if i == 1:
            return np.asarray(self.x, F32)
        P = self.C.enc[i - 2]
        return operand32(self.taps["conv%d" % (i - 1)], P["scale"], P["shift"], self.actE)

    def ref(self, n):
        """float64 layer, with the allowance of the family that ran"""
        fam = self.fam(n)
        if n == "head":
            return self.LL.head()[0]
        i = int(n[-1])
        if n.startswith("down"):
            L = self.C.enc[i - 1]
            if fam == "f16x2":
                f, eps = self.LL._operand(i)
                r = R.enc_ref(f, split_gap(f, eps), L["w"], L["b"], w_half=False, fp32_products=False, out_half=False)
                r.share = 0.0
                return r
            r = self.LL.enc(i)[0]
            if fam == "wino":
                f = self.LL._operand(i)[0]
                r.E = r.E - r.acc + (f.shape[0] + C_WINO_ENC) * EPS32 * wino("conv", f, L["w"], np.float64, bound=True)
            return r
        L = self.C.dec[i - 1]
        x = self.LL.dec_input(i)
        r = self.LL.dec(i)[0]
        sc = np.abs(L["scale"])[:, None, None]
        if fam == "wino":
            r.E = r.E - r.acc + sc * (x.shape[0] + C_WINO_DEC) * EPS32 * wino("tconv", x, L["w"], np.float64, bound=True)
        elif fam == "f16x2":
            r.E = r.E + sc * R.contract64("tconv", split_gap(x), np.abs(L["w"]))
        return r

    def emu(self, n, reverse=False, w_map=None, x_map=None, **kw):
        """the stored tensor of layer n as a correct kernel of its family gives it (fp32).  w_map / x_map: applied to the fp32 weights / operands first (planted errors)"""
        fam = self.fam(n)
        w_map, x_map = w_map or (lambda v: v), x_map or (lambda v: v)
        if fam == "direct" and n != "head":
            kw.setdefault("group", self.group.get(n, None if n == "up6" else 2))
        if n == "head":
            return head_emu(self.taps["up6"], self.C.head_w, self.C.head_b, reverse, self.head_fast)      # (one input channel: the 16 taps are its only terms, an FMA chain on the device)
        i = int(n[-1])
        if n.startswith("down"):
            L = self.C.enc[i - 1]
            return enc_emu(fam, x_map(self.enc_operand32(i)), w_map(np.asarray(L["w"], F32)), L["b"], reverse, **kw)
        L = self.C.dec[i - 1]
        return dec_emu(fam, x_map(np.asarray(self.LL.dec_input(i), F32)), w_map(np.asarray(L["w"], F32)), L["b"], L["scale"], L["shift"], self.actD, reverse, **kw)

    def got(self, n, mask):
        return mask if n == "head" else self.taps["conv" + n[-1] if n.startswith("down") else n]


# ------------------------------------------------------------------------------------------- the checks
def zstats(got, r):
    """-> (RMS z, max |z|); a non-finite value counts as infinite"""
    z = (np.asarray(got, np.float64) - r.ref) / r.u
    if not np.isfinite(z).all():
        return np.inf, np.inf
    return float(np.sqrt(np.mean(z * z))), float(np.abs(z).max())


def judge32(got, r, yard):
    """yard = (RMS z, max |z|) of the emulation -> dict of the figures and the list of failed checks among A, C, D"""
    n, worst, where = R.check_a(got, r)
    rms, mx = zstats(got, r)
    out = dict(a_viol=n, a_worst=worst, a_where=where, n=int(r.ref.size), c=rms, c_emu=yard[0], c_cap=CAP_C * yard[0], d=mx, d_emu=yard[1], d_cap=CAP_D * yard[1], fail=[])
    if n:
        out["fail"].append("A")
    if not rms <= out["c_cap"]:
        out["fail"].append("C")
    if not mx <= out["d_cap"]:
        out["fail"].append("D")
    return out


def fmt32(tag, n, j, extra=""):
    return "%s %-5s n %7d  A: %d over, worst %.3f of E; RMS z %.4f (emulation %.4f, cap %.4f); max|z| %.2f (emulation %.2f, cap %.2f)%s%s" % (
        tag, n, j["n"], j["a_viol"], j["a_worst"], j["c"], j["c_emu"], j["c_cap"], j["d"], j["d_emu"], j["d_cap"], extra, "   FAILS " + "".join(j["fail"]) if j["fail"] else "")
