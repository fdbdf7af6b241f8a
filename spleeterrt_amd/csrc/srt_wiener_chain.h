// srt_wiener_chain.h — the per-(row, bin) chain of the multichannel Wiener filter: the soft-mask start and one EM iteration, in spectrum units (the derivation
// is in srt_wiener.hip's header).  One text for every kernel that evaluates the chain: the statistics / filter kernels of srt_wiener.hip and the live hop's
// filtering inverse (srt_live_wiener_inverse_kernel, srt_dsp.hip).  Device code only; include it at the file's default fp contraction (fast).
#pragma once
#include "srt_internal.h"
#include <math.h>

#define W_EPS      1.1920928955078125e-07f        // 2^-23: fp32 machine epsilon, norbert's default for complex64
#define W_SQRT_EPS 3.4526698300124393e-04f        // 2^-11.5
#define W_EPS_SOFT 2.9103830456733704e-11f        // 2^-35 = eps / 4096: the soft mask's epsilon in spectrum units

// soft-mask start: y_j = v_j / (eps + sum_i v_i) s per channel; m points at stem 0's mask value of this (row, bin), stems sstride apart, R channel + tf
__device__ __forceinline__ void w_start(float2 (&yl)[SRT_MAX_STEMS], float2 (&yr)[SRT_MAX_STEMS], float2 sL, float2 sR,
                                        const float* __restrict__ m, size_t sstride, size_t tf, int S)
{
    const float aL = hypotf(sL.x, sL.y), aR = hypotf(sR.x, sR.y);
    float vl[SRT_MAX_STEMS], vr[SRT_MAX_STEMS], suml = 0.0f, sumr = 0.0f;
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) {
        vl[j] = 0.0f; vr[j] = 0.0f;
        if (j < S) { vl[j] = m[j * sstride] * aL; vr[j] = m[j * sstride + tf] * aR; suml += vl[j]; sumr += vr[j]; }
    }
    const float il = 1.0f / (W_EPS_SOFT + suml), ir = 1.0f / (W_EPS_SOFT + sumr);
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) {
        const float gl = vl[j] * il, gr = vr[j] * ir;
        yl[j] = make_float2(gl * sL.x, gl * sL.y);
        yr[j] = make_float2(gr * sR.x, gr * sR.y);
    }
}

// |y_L|^2 + |y_R|^2 of one stem as the kernels of a plain call form it from w_iter's sum below: the first square, then one fused multiply-add per further
// component, left to right.  Spelled out (contraction off, explicit fmaf) for the option kernels at the end of srt_wiener.hip: there the vectoriser otherwise turns the
// sum into packed products and separate adds in some instantiations and not in others, and the estimates differ in their last bits between kernels that have
// to agree bit for bit (a one-hot remix and the stem; one tile with and without an overlap).
#pragma clang fp contract(off)
__device__ __forceinline__ float w_power(float2 a, float2 b)
{
    float t = a.x * a.x;
    t = fmaf(a.y, a.y, t);
    t = fmaf(b.x, b.x, t);
    return fmaf(b.y, b.y, t);
}
#pragma clang fp contract(fast)

// one EM iteration at (row, bin): R points at stem 0's entry of this bin in the iteration's table, stems F apart; delta = sqrt(eps) al^2
// PIN (the option kernels, the live hop): the stem's power through w_power; false: the statement as it always was, and the plain kernels' code with it
template <bool PIN = false>
__device__ __forceinline__ void w_iter(float2 (&yl)[SRT_MAX_STEMS], float2 (&yr)[SRT_MAX_STEMS], float2 sL, float2 sR,
                                       const float4* __restrict__ R, int F, float delta, int S)
{
    float v[SRT_MAX_STEMS];
    float c00 = delta, c11 = delta, c01r = 0.0f, c01i = 0.0f;
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) {
        if constexpr (PIN) v[j] = 0.5f * w_power(yl[j], yr[j]);
        else v[j] = 0.5f * (yl[j].x * yl[j].x + yl[j].y * yl[j].y + yr[j].x * yr[j].x + yr[j].y * yr[j].y);
        if (j < S) {
            const float4 r = R[(size_t)j * F];
            c00 += v[j] * r.x; c11 += v[j] * r.y; c01r += v[j] * r.z; c01i += v[j] * r.w;
        }
    }
    const float id = 1.0f / (c00 * c11 - (c01r * c01r + c01i * c01i));
    // z = C^-1 s with C^-1 = [c11, -c01; -conj(c01), c00] / det
    const float2 zL = make_float2((c11 * sL.x - (c01r * sR.x - c01i * sR.y)) * id, (c11 * sL.y - (c01r * sR.y + c01i * sR.x)) * id);
    const float2 zR = make_float2((c00 * sR.x - (c01r * sL.x + c01i * sL.y)) * id, (c00 * sR.y - (c01r * sL.y - c01i * sL.x)) * id);
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) {
        if (j < S) {
            const float4 r = R[(size_t)j * F];                 // y_j = v_j R_j z: R = [R00, R01; conj(R01), R11]
            const float2 a = make_float2(r.x * zL.x + (r.z * zR.x - r.w * zR.y), r.x * zL.y + (r.z * zR.y + r.w * zR.x));
            const float2 b = make_float2((r.z * zL.x + r.w * zL.y) + r.y * zR.x, (r.z * zL.y - r.w * zL.x) + r.y * zR.y);
            yl[j] = make_float2(v[j] * a.x, v[j] * a.y);
            yr[j] = make_float2(v[j] * b.x, v[j] * b.y);
        }
    }
}
