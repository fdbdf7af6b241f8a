// srt_dsp.hip — STFT / magnitude / mask-apply / inverse STFT / overlap-add kernels for gfx950.
//
// Replaces, for the hot path only:
//   stft    : Executable/stftFix.c:363-495 (window, bit-reverse, DFT4096 x2, re/im unpack)      K1
//   mag     : Executable/main.c:462-471, :500-514                                              K2
//   mask    : Executable/main.c:473-494                                                        K8
//   istft   : Executable/stftFix.c:496-579 (Hartley pack, DFT4096, post-window, overlap-add)   K9
//   DFT4096 : Executable/codelet.c:2-271  (4096-point fast Hartley transform)
//
// Design (not a translation of the Hartley codelet): one 256-thread workgroup runs a 4096-point COMPLEX FFT
// entirely in registers + LDS as three radix-16 passes (16 values per thread).  Left and right channels ride in
// the real and imaginary parts of the same transform (z = L + iR), so one FFT serves both channels of a frame;
// the two spectra are separated in the epilogue, where the magnitude tile for the network is emitted as well.
// The inverse uses the same FFT (swap trick) on G = F'_L + i F'_R after the per-stem mask multiply (one workgroup
// column per stem).  Overlap-add is fused and register resident: frames are added in frame order, every output
// sample is written once (see srt_istft_ola_kernel).
#include "srt_internal.h"
#include "srt_device.h"
#include "srt_overlap.h"
#include <stdlib.h>
#include <type_traits>

#define FFT_EX1_LD 272      // exchange-1 row stride (cf): 272*2 dwords = 32 (mod 64) -> conflict-free b64 reads
#define FFT_EX2_LD 257      // exchange-2 row stride (cf): odd -> conflict-free strided b64 writes
#define FFT_SMEM_F2 4352    // 16*272 cf scratch (also holds 4096 natural-order points)

// Complex values are 2-wide vectors so the butterflies map onto the packed fp32 VALU (v_pk_add/mul/fma_f32: two lanes per
// instruction).  The two operations the compiler does not fold into one packed instruction by itself — a +/- (-i)b and the
// complex product — are spelled out with their op_sel / neg modifiers (half swaps and sign flips are free on VOP3P);
// with them a radix-4 butterfly is 8 packed adds and a complex multiply is 2 packed ops (2.1x fewer VALU instructions
// per FFT than scalar-component code run through the SLP vectoriser).
typedef float cf __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cf f2(float x, float y) { cf r = { x, y }; return r; }
__device__ __forceinline__ cf add_mi(cf a, cf b)       // a + (-i) b = (a.x + b.y, a.y - b.x)
{
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ cf sub_mi(cf a, cf b)       // a - (-i) b = (a.x - b.y, a.y + b.x)
{
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ cf cmul(cf a, cf w)         // (a.x w.x - a.y w.y, a.y w.x + a.x w.y)
{
    cf t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "v"(w));                                              // (a.x w.x, a.y w.x)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(a), "v"(w), "v"(t));   // (-a.y w.y + t.x, a.x w.y + t.y)
    return r;
}

__device__ __forceinline__ cf herm_hi(cf b, cf a)       // (b.x + a.y, a.x - b.y)
{
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[1,0]" : "=v"(r) : "v"(b), "v"(a));
    return r;
}

// separation of the two real spectra packed in one complex transform (z = L + iR): with zk = Z[k], zm = Z[N-k]
__device__ __forceinline__ cf split_l(cf zk, cf zm)     // (zk.x + zm.x, zm.y - zk.y)
{
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[1,0]" : "=v"(r) : "v"(zk), "v"(zm));
    return r;
}
__device__ __forceinline__ cf split_r(cf zk, cf zm)     // (zk.y + zm.y, zk.x - zm.x)
{
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,0] neg_hi:[0,1]" : "=v"(r) : "v"(zk), "v"(zm));
    return r;
}

// forward 4-point DFT in place (W4 = -i)
__device__ __forceinline__ void dft4(cf& a, cf& b, cf& c, cf& d)
{
    const cf s0 = a + c, s1 = a - c, s2 = b + d, s3 = b - d;
    a = s0 + s2;
    c = s0 - s2;
    b = add_mi(s1, s3);
    d = sub_mi(s1, s3);
}

// forward 16-point DFT, natural-order input v[n]; OUTPUT X[k] is left at v[4*(k&3) + (k>>2)]
#define FFT16_AT(k) (4 * ((k) & 3) + ((k) >> 2))
__device__ __forceinline__ void fft16(cf (&v)[16])
{
#pragma unroll
    for (int n0 = 0; n0 < 4; ++n0) dft4(v[n0], v[n0 + 4], v[n0 + 8], v[n0 + 12]);
    // y[n0][k0] sits at v[n0 + 4*k0]; twiddle by W16^(n0*k0)
    const float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, r2 = 0.70710678118654752440f;
    v[1 + 4 * 1] = cmul(v[1 + 4 * 1], f2(c1, -s1));      // W^1
    v[2 + 4 * 1] = cmul(v[2 + 4 * 1], f2(r2, -r2));      // W^2
    v[3 + 4 * 1] = cmul(v[3 + 4 * 1], f2(s1, -c1));      // W^3
    v[1 + 4 * 2] = cmul(v[1 + 4 * 2], f2(r2, -r2));      // W^2
    v[2 + 4 * 2] = add_mi(f2(0.f, 0.f), v[2 + 4 * 2]);   // W^4 = -i
    v[3 + 4 * 2] = cmul(v[3 + 4 * 2], f2(-r2, -r2));    // W^6
    v[1 + 4 * 3] = cmul(v[1 + 4 * 3], f2(s1, -c1));      // W^3
    v[2 + 4 * 3] = cmul(v[2 + 4 * 3], f2(-r2, -r2));     // W^6
    v[3 + 4 * 3] = cmul(v[3 + 4 * 3], f2(-c1, s1));      // W^9
#pragma unroll
    for (int k0 = 0; k0 < 4; ++k0) dft4(v[4 * k0], v[4 * k0 + 1], v[4 * k0 + 2], v[4 * k0 + 3]);
}

// Per-thread twiddles are frame independent, so each workgroup re-lays the (double-precision generated) table once
// into the order its threads read it: twA[k0-1][tid] = W^(tid*k0), twB[k1-1][lo] = W^(16*lo*k1).  All twiddle reads are
// then consecutive or broadcast (conflict-free), instead of stride-k gathers into a 4096-entry table.
#define FFT_TW_F2 (15 * 256 + 15 * 16)
__device__ __forceinline__ void fft_load_twiddles(cf* tw, const float2* __restrict__ table_f2, int tid)
{
    const cf* __restrict__ table = reinterpret_cast<const cf*>(table_f2);
#pragma unroll
    for (int k0 = 1; k0 < 16; ++k0) tw[(k0 - 1) * 256 + tid] = table[(tid * k0) & 4095];
    if (tid < 240) tw[15 * 256 + tid] = table[(16 * (tid & 15) * (tid / 16 + 1)) & 4095];
}

// 4096-point forward FFT.  In: v[n2] = x[tid + 256*n2].  Out: v[FFT16_AT(k2)] = X[tid + 256*k2].
// s: FFT_SMEM_F2 cf of LDS scratch, tw: the re-laid twiddles (fft_load_twiddles).
// The caller must __syncthreads() before reusing s after return.
__device__ __forceinline__ void fft4096(cf (&v)[16], cf* s, const cf* tw, int tid)
{
    fft16(v);                                            // over n2 -> k0
#pragma unroll
    for (int k0 = 1; k0 < 16; ++k0) v[FFT16_AT(k0)] = cmul(v[FFT16_AT(k0)], tw[(k0 - 1) * 256 + tid]);
#pragma unroll
    for (int k0 = 0; k0 < 16; ++k0) s[k0 * FFT_EX1_LD + tid] = v[FFT16_AT(k0)];
    __syncthreads();
    const int lo = tid & 15, hi = tid >> 4;              // (n0, k0)
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) v[n1] = s[hi * FFT_EX1_LD + n1 * 16 + lo];
    fft16(v);                                            // over n1 -> k1
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) v[FFT16_AT(k1)] = cmul(v[FFT16_AT(k1)], tw[15 * 256 + (k1 - 1) * 16 + lo]);
    __syncthreads();
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) s[lo * FFT_EX2_LD + k1 * 16 + hi] = v[FFT16_AT(k1)];
    __syncthreads();
#pragma unroll
    for (int n0 = 0; n0 < 16; ++n0) v[n0] = s[n0 * FFT_EX2_LD + tid];   // tid = k0 + 16*k1
    fft16(v);                                            // over n0 -> k2
}

// The same transform for kernels that walk MANY frames per workgroup, with half the barriers: the 15 pass-1 twiddles of a thread
// are frame independent and live in registers (twa), which shrinks the LDS twiddle table to the 240 pass-2 entries and makes
// room for TWO exchange buffers.  With exchange 1 in one buffer and exchange 2 in the other no barrier is needed between
// reading an exchange and writing the next one:
//   in : v[n2] = x[tid + 256*n2], read by every thread from buffer `e2` (or from registers) AFTER a barrier that follows the
//        last use of buffer `e1` by the previous frame
//   out: v[FFT16_AT(k2)] = X[tid + 256*k2]; `e1` is free again, `e2` still holds exchange 2 until the caller's next barrier
// A frame then costs 3 barriers (staging, exchange 1, exchange 2) instead of 6.
#define FFT_TWB_F2 240
__device__ __forceinline__ void fft_load_twiddles_pp(cf (&twa)[15], cf* twb, const float2* __restrict__ table_f2, int tid)
{
    const cf* __restrict__ table = reinterpret_cast<const cf*>(table_f2);
#pragma unroll
    for (int k0 = 1; k0 < 16; ++k0) twa[k0 - 1] = table[(tid * k0) & 4095];
    if (tid < FFT_TWB_F2) twb[tid] = table[(16 * (tid & 15) * (tid / 16 + 1)) & 4095];
}
__device__ __forceinline__ void fft4096_pp(cf (&v)[16], cf* e1, cf* e2, const cf (&twa)[15], const cf* twb, int tid)
{
    fft16(v);                                            // over n2 -> k0
#pragma unroll
    for (int k0 = 1; k0 < 16; ++k0) v[FFT16_AT(k0)] = cmul(v[FFT16_AT(k0)], twa[k0 - 1]);
#pragma unroll
    for (int k0 = 0; k0 < 16; ++k0) e1[k0 * FFT_EX1_LD + tid] = v[FFT16_AT(k0)];
    __syncthreads();
    const int lo = tid & 15, hi = tid >> 4;              // (n0, k0)
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) v[n1] = e1[hi * FFT_EX1_LD + n1 * 16 + lo];
    fft16(v);                                            // over n1 -> k1
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) v[FFT16_AT(k1)] = cmul(v[FFT16_AT(k1)], twb[(k1 - 1) * 16 + lo]);
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) e2[lo * FFT_EX2_LD + k1 * 16 + hi] = v[FFT16_AT(k1)];
    __syncthreads();
#pragma unroll
    for (int n0 = 0; n0 < 16; ++n0) v[n0] = e2[n0 * FFT_EX2_LD + tid];   // tid = k0 + 16*k1
    fft16(v);                                            // over n0 -> k2
}

#define STFT_FPB 8      // frames per workgroup on long signals (amortises the twiddle-table load; consecutive frames share 75% of input)

// Inverse STFT with the overlap-add fused in (no frame scratch, no second pass, no atomics).
// With the radix-16 FFT's output distribution thread w holds samples w + 256*k2 of a frame, i.e. for each of the four
// 1024-sample quarters the SAME four in-hop offsets q_j = w + 256 j.  Overlap-add across frames is therefore
// thread-local: a workgroup (blockIdx.y = stem) walks a run of consecutive frames and keeps a rolling window of four
// partial output segments in registers; segment s is complete once frame s has been added (frames s-3..s, added in that
// order = the reference's accumulation order, stftFix.c:570-575) and is written out exactly once.  A workgroup that
// owns segments [s0, s1) recomputes the three frames before s0 as warm-up ((G+3)/G extra work).
// The loop body is straight-line: the next frame's rows are prefetched from a CLAMPED frame index (a redundant reload
// at the very end instead of a conditional assignment, which costs a register copy per staged value at every merge).
// Cross-stem ratio mask folded into the inverse transform's prologue (srt_config.ratio_mask): instead of a separate read-modify-write pass over every
// stem's masks (srt_ratio_mask_kernel: 2 x 0.5 GB at the bench shape), the workgroup that applies stem s's mask to a bin reads the OTHER stems' mask values of that bin
// too (its S-1 neighbours on the XCD read the same rows at the same time: L2 hits) and normalises in registers.  Same arithmetic in the same order as
// srt_ratio_mask_kernel (squares summed over stems ascending, (m_s^2 + eps/S) / (sum + eps)), so srtSeparate with ratio_mask equals srtRatioMask + srtIstft bit for bit.
// own: the stem's raw mask value (already loaded); row0: mask row of stem 0 for this (tile, channel, frame); sstride: floats between stems.
#pragma clang fp contract(off)     // (HIP's __fmul_rn / __fadd_rn are plain operators: only this keeps the compiler from fusing square and sum)
__device__ __forceinline__ float srt_ratio_of(float own, const float* __restrict__ row0, size_t sstride, int nstems, int stem, int k)
{
    // (plain operators under contract(off): the square is rounded before it is added, exactly as in srt_ratio_mask_kernel.  HIP's __fmul_rn / __fadd_rn would
    // not do: they are inline `x * y` / `x + y` from a header compiled with contraction on, and fuse after inlining.)
    float sum = 0.0f;
    const float mine = own * own;
    for (int s = 0; s < nstems; ++s) {
        const float v = row0[(size_t)s * sstride + k];
        const float sq = v * v;
        sum = sum + (s == stem ? mine : sq);
    }
    const float eps = 1e-10f, e1 = eps / (float)nstems;
    return (mine + e1) / (sum + eps);
}

// Overlapped network tiles (srtSetOverlap): OvRow / srt_ov_row (a row's primary tile, offset and blend weight) and srt_blend (the cross-fade,
// rounded step by step) live in srt_overlap.h, shared with the Wiener filter's option kernels.
// srt_ratio_of on BLENDED masks: every stem's value - the workgroup's own included - is blended from the two tiles' rows first (rowb0 / rowa0: mask row of stem 0
// in the primary / the previous tile; rowa0 is read only when two), then squared and summed as in srt_ratio_of.  The RATIO overlap instantiations do not prefetch
// their own mask row (it is one of the rows read here; the registers it would be staged in are what the F > 1024 form spills): ratio = false returns the stem's own
// blended value.
// SEAM: rowa0 may be a row of the mask seam carry (srt_ov_seam), whose stems lie astride floats apart; otherwise astride is unused (a's stems are sstride apart as b's).
template <bool SEAM = false>
__device__ __forceinline__ float srt_ratio_of_ov(const float* __restrict__ rowb0, const float* __restrict__ rowa0, bool two, float w,
                                                 size_t sstride, int nstems, int stem, int k, bool ratio, size_t astride = 0)
{
    float sum = 0.0f, own = 0.0f;
    for (int s = 0; s < nstems; ++s) {
        float v = rowb0[(size_t)s * sstride + k];
        if constexpr (SEAM) { if (two) v = srt_blend(rowa0[(size_t)s * astride + k], v, w); }
        else
        if (two) v = srt_blend(rowa0[(size_t)s * sstride + k], v, w);
        const float sq = v * v;
        sum = sum + sq;
        if (s == stem) own = v;
    }
    const float mine = own * own;
    const float eps = 1e-10f, e1 = eps / (float)nstems;
    return ratio ? (mine + e1) / (sum + eps) : own;
}

// Stem remix (srtSetMix): output m of a MIX launch multiplies a bin by h = G[m][S], then h = fmaf(G[m][s], g_s, h) for s = 0 .. S-1 ascending, where
// g_s is the gain the forms above apply for stem s - the mask value, blended (srt_blend), then normalised across the stems; the arithmetic of srt_ratio_of /
// srt_ratio_of_ov step for step (blend first, squares summed over the stems ascending, (m_s^2 + eps/S) / (sum + eps)), so a one-hot row gives stem m's bits.
// The stem loop is the OUTER one: a pass over the stems for the square sums (ratio only), a second one for the chain (its re-reads are cache hits) - one matrix
// entry per stem (a uniform load) and no per-stem array.  hl / hr: the NB bins tid + 256 j of the two channels.
// r0 / a0: stem 0's L row of the frame in its primary / previous tile (r0 null: no masks, g_s = 1; a0 read only when two); ratio: a run-time flag here.
// Where row m of the matrix comes from is the gain source `g`, g(s) = G[m][s]: the launch's own arguments (srtSetMix: one matrix per call), or a row of the
// device table of a packed batch (srtSeparateBatchMix: one matrix per track).  Either way the address is workgroup-uniform and an entry is loaded where it is used.
struct SrtMixArg { const SrtIstftParams& p; int m; __device__ __forceinline__ float operator()(int s) const { return p.mix[m][s]; } };
struct SrtMixTab { const float* __restrict__ row; __device__ __forceinline__ float operator()(int s) const { return row[s]; } };
// SEAM: a0 may be a row of the mask seam carry (srt_ov_seam): its stems lie astem floats apart and its channels ach; unused otherwise (a0 is a mask row like r0).
template <int NB, int JC, class GS, bool SEAM = false>
__device__ __forceinline__ void srt_mix_gains(const SrtIstftParams& p, const GS& g, const float* __restrict__ r0, const float* __restrict__ a0, bool two, float w, bool ratio, int tid,
                                              float (&hl)[NB], float (&hr)[NB], size_t astem = 0, size_t ach = 0)
{
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf;
    const size_t as = SEAM ? astem : sstride, ac = SEAM ? ach : tf;
    const float eps = 1e-10f, e1 = eps / (float)p.nstems;
    auto value = [&](const float* __restrict__ b, const float* __restrict__ a, int km) {
        float v = b[km];
        if (two) v = srt_blend(a[km], v, w);
        return v;
    };
    // JC bins at a time: the square sums of a chunk are dead before the next one starts (all nine bins of the F > 1024 form at once spill)
#pragma unroll
    for (int j0 = 0; j0 < NB; j0 += JC) {
        float suml[JC], sumr[JC];
#pragma unroll
        for (int i = 0; i < JC; ++i) { suml[i] = 0.0f; sumr[i] = 0.0f; }
#pragma unroll
        for (int i = 0; i < JC; ++i) if (j0 + i < NB) { hl[j0 + i] = g(p.nstems); hr[j0 + i] = hl[j0 + i]; }
        if (r0 && ratio) {
            for (int s = 0; s < p.nstems; ++s) {
                const float* b = r0 + (size_t)s * sstride; const float* a = a0 + (size_t)s * as;
#pragma unroll
                for (int i = 0; i < JC; ++i) {
                    if (j0 + i >= NB) continue;
                    const int km = min(min(tid + 256 * (j0 + i), 2048), p.F - 1);
                    const float vl = value(b, a, km), vr = value(b + tf, a + ac, km);
                    const float ql = vl * vl, qr = vr * vr;
                    suml[i] = suml[i] + ql; sumr[i] = sumr[i] + qr;
                }
            }
        }
        for (int s = 0; s < p.nstems; ++s) {
            const float gm = g(s);
            const float* b = r0 + (size_t)s * sstride; const float* a = a0 + (size_t)s * as;
#pragma unroll
            for (int i = 0; i < JC; ++i) {
                if (j0 + i >= NB) continue;
                const int km = min(min(tid + 256 * (j0 + i), 2048), p.F - 1);
                float vl = 1.0f, vr = 1.0f;
                if (r0) {
                    vl = value(b, a, km); vr = value(b + tf, a + ac, km);
                    if (ratio) {
                        const float ml = vl * vl, mr = vr * vr;
                        vl = (ml + e1) / (suml[i] + eps); vr = (mr + e1) / (sumr[i] + eps);
                    }
                }
                hl[j0 + i] = fmaf(gm, vl, hl[j0 + i]); hr[j0 + i] = fmaf(gm, vr, hr[j0 + i]);
            }
        }
    }
}
// the same chain over one value per stem (workgroup-uniform): x[s * stride], s ascending - the constant weights of bins >= F, or a row of the extension's table
template <class GS>
__device__ __forceinline__ float srt_mix_chain(const SrtIstftParams& p, const GS& g, const float* __restrict__ x, size_t stride)
{
    float h = g(p.nstems);
    for (int s = 0; s < p.nstems; ++s) h = fmaf(g(s), x[(size_t)s * stride], h);
    return h;
}

#pragma clang fp contract(fast)

// What a workgroup of the inverse kernels reads and writes of ONE signal: the whole call's signal (srt_istft_ola_kernel / srt_istft_ola3_kernel),
// or one track of a packed batch (srt_istft_batch_kernel: spectrum and masks offset to the track's first packed row / tile, its own frames and output).
// Everything else (stem count and stride, T, F, oob weights, tables) comes from the launch's SrtIstftParams.
// ext: the signal's rows of the average mask extension's gain table (stem 0's; EXT instantiations only, see srt_mask_ext_kernel)
// gain: row 0 of the signal's remix matrix [n_out][nstems + 1] in device memory (the GTAB instantiations only: a track of srtSeparateBatchMix)
struct IstftView { const float2* spec; const float* masks; float* out; size_t out_len; int frames; const float* ext; const float* gain; };
__device__ __forceinline__ IstftView istft_view(const SrtIstftParams& p) { IstftView v = { p.spec, p.masks, p.out, p.out_len, p.frames, p.ext, nullptr }; return v; }

// the gain source of output m of a MIX body (see srt_mix_gains)
template <bool GTAB>
__device__ __forceinline__ auto srt_mix_source(const SrtIstftParams& p, const IstftView& w, int m)
{
    if constexpr (GTAB) return SrtMixTab{ w.gain + (size_t)m * (p.nstems + 1) };
    else return SrtMixArg{ p, m };
}

#define ISTFT_OLA_LDS_F2 (2 * FFT_SMEM_F2 + FFT_TWB_F2)   // two staging / exchange buffers + the pass-2 twiddles (one LDS object)
// OV: overlapped network tiles (srt_ov_row): the mask row of a frame's primary tile is prefetched as always; inside an overlap the previous tile's row is
// read when the frame is staged and the two are blended before the ratio / multiply
// EXT: average mask extension (srtSetMaskExtension): bins >= F of frame f take the two gains ext[stem][f][L, R] instead of oob (fetched with the frame's rows
// from workgroup-uniform addresses: scalar loads into SGPRs, consumed before the next fetch overwrites them)
// MIX: stem remix (srt_mix_gains): `stem` is the OUTPUT index m; no mask row is prefetched (every stem's row is read in the prologue), RATIO = false (a run-time flag)
// TRK (with OV): the view is a track of a packed batch - p.ntiles is the packed total there (the masks' stem stride), and srt_ov_row clamps the primary tile with the
// track's own overlapped count, the argument ov_tiles (unused otherwise: a whole call's count is p.ntiles)
// GTAB (with MIX): the matrix row is read from the view's device table (w.gain, SrtMixTab) instead of the launch arguments (p.mix, SrtMixArg)
// SEAM (with OV): the signal is a piece of a longer stream (srtSeparateHostStreamOverlap) - rows [0, O) of its first tile (srt_ov_seam) take their
// blend partner `a` from the mask seam carry `seam` [nstems][2][O][F], what the previous piece's last tile held in rows [S, T); every other row as OV.  The choice
// of base and strides is workgroup-uniform (scalar); a null seam (the stream's first piece) leaves the OV behaviour
template <bool RATIO, bool OV = false, bool EXT = false, bool MIX = false, bool TRK = false, bool GTAB = false, bool SEAM = false>
__device__ __forceinline__ void istft_ola_run(const SrtIstftParams& p, const IstftView& w, int stem, int run, int G, cf* s_mem, int O = 0, int ov_tiles = 0, const float* seam = nullptr)
{
    static_assert(!SEAM || (OV && !TRK), "the seam carry belongs to one signal's overlapped tiles");
    cf* sx = s_mem;                                      // this frame's staging buffer (and its exchange 2)
    cf* sy = s_mem + FFT_SMEM_F2;                        // this frame's exchange 1; the roles swap every frame
    cf* s_twb = s_mem + 2 * FFT_SMEM_F2;
    const int tid = threadIdx.x;
    cf twa[15];
    fft_load_twiddles_pp(twa, s_twb, p.tab.twiddle, tid);
    const size_t tf = (size_t)p.T * p.F;
    const int nseg = w.frames + 3;
    const int s0 = run * G, s1 = min(s0 + G, nseg);
    const auto gsrc = srt_mix_source<GTAB>(p, w, stem);
    const float oob = MIX ? srt_mix_chain(p, gsrc, p.oob, 1) : p.oob[stem];   // bins >= F: "unaffectedWeight" (main.c:486-493)
    const cf* spec = reinterpret_cast<const cf*>(w.spec);
    float* oL = w.out + (size_t)(stem * 2 + 0) * w.out_len;
    float* oR = w.out + (size_t)(stem * 2 + 1) * w.out_len;

    cf acc[4][4];                                       // [segment slot][j] = (R, L) pairs: one packed fma per output sample pair
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[h][j] = f2(0.0f, 0.0f);

    // Software pipeline: the spectrum row and the mask rows of the NEXT frame are in flight while the current frame is
    // transformed, so the global-load latency is not exposed once per FFT.
    cf sl[9], sr[9];
    float gl[9], gr[9];
    float eL = oob, eR = oob;
    const float* __restrict__ const ext = EXT ? w.ext + (MIX ? 0 : (size_t)stem * p.ext_stem) : nullptr;
    // fetch only ISSUES loads (no value depends on them until the next iteration): without masks the two mask rows
    // are read from a harmless table instead of branching on the pointer
    const bool has_mask = w.masks != nullptr;
    auto fetch = [&](int f) {                                               // 0 <= f < w.frames
        int tile = f / p.T, t = f % p.T;
        OvRow ov = { 0, 0, false, 0.0f };
        if constexpr (OV) { ov = srt_ov_row(f, p.T, O, TRK ? ov_tiles : p.ntiles); tile = ov.j1; t = ov.k; }
        const cf* specL = spec + (size_t)f * SRT_SPEC_LD;
        const cf* specR = specL + p.spec_ch_stride;
        const float* mL = has_mask ? w.masks + ((size_t)(stem * p.ntiles + tile) * 2) * tf + (size_t)t * p.F : p.tab.postWin;
        const float* mR = has_mask ? mL + tf : p.tab.postWin;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int k = min(tid + 256 * j, 2048), km = min(k, p.F - 1);
            sl[j] = specL[k]; sr[j] = specR[k];
            if constexpr (!(RATIO && OV) && !MIX) { gl[j] = mL[km]; gr[j] = mR[km]; }      // (RATIO && OV: see srt_ratio_of_ov)
        }
        if constexpr (EXT && !MIX) { const size_t fu = (size_t)__builtin_amdgcn_readfirstlane(f) * 2; eL = ext[fu]; eR = ext[fu + 1]; }
    };
    float pw[16];                                       // this thread's 16 synthesis-window taps are the same for every frame
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) pw[k2] = p.tab.postWin[tid + 256 * k2];
    const int f0 = max(s0 - 3, 0);                      // frames before 0 do not exist: the window simply starts empty
    if (f0 < w.frames) fetch(f0);
    // Segment f is complete once frame f has been added, but it is WRITTEN in iteration f + 1, right before that iteration requests the rows of
    // frame f + 2: vmcnt counts loads and stores in one queue, so the wait for a frame's rows also waits for every store issued before them -
    // stores issued just ahead of the wait (the end of the previous iteration, where this code stood in rounds 1-2) cost their full
    // acknowledgement time (~1-2 us) once per frame; issued ahead of the NEXT prefetch they have a whole FFT to complete.
    auto emit_and_slide = [&](int seg) {
        if (seg >= s0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { oL[(size_t)seg * SRT_HOP + tid + 256 * j] = acc[0][j].y; oR[(size_t)seg * SRT_HOP + tid + 256 * j] = acc[0][j].x; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {                   // slide the window
            acc[0][j] = acc[1][j]; acc[1][j] = acc[2][j]; acc[2][j] = acc[3][j]; acc[3][j] = f2(0.0f, 0.0f);
        }
    };
    for (int f = f0; f < s1; ++f) {
        if (f < w.frames) {                             // workgroup-uniform; false only for the last three segments of the stream
            // staging into sx: its last readers (exchange 1 of the previous frame, when it was `sy`) all passed that frame's
            // second barrier; the first barrier below also orders the twiddle table written before the loop
            OvRow ov = { 0, 0, false, 0.0f };
            // SEAM: whether the row's partner is a row of the carry, and then the carry's strides in place of the masks' (stem 0, L of row ov.k at seam + ov.k * F)
            bool sm = false;
            size_t a_stem = 0, a_ch = 0;
            if constexpr (OV) {
                ov = srt_ov_row(f, p.T, O, TRK ? ov_tiles : p.ntiles);
                if constexpr (SEAM) {
                    asm volatile("" : "+s"(seam));       // the carry's lane addresses are formed per frame: hoisted out of the frame loop they would be 2 x NB more resident VGPRs
                    sm = srt_ov_seam(ov, O, seam);
                    a_ch = sm ? (size_t)O * p.F : tf; a_stem = sm ? 2 * (size_t)O * p.F : (size_t)p.ntiles * 2 * tf;
                    if (!RATIO && !MIX && has_mask && (ov.two || sm)) {      // as below, a from the carry on the piece's first O rows
                        const float* aL = sm ? seam + (size_t)stem * a_stem + (size_t)ov.k * p.F : w.masks + ((size_t)(stem * p.ntiles + ov.j1 - 1) * 2) * tf + (size_t)(ov.k + p.T - O) * p.F;
#pragma unroll
                        for (int j = 0; j < 9; ++j) {
                            const int km = min(min(tid + 256 * j, 2048), p.F - 1);
                            gl[j] = srt_blend(aL[km], gl[j], ov.w); gr[j] = srt_blend(aL[a_ch + km], gr[j], ov.w);
                        }
                    }
                } else
                if (!RATIO && !MIX && has_mask && ov.two) {      // cross-fade of the two tiles' masks: a (row k + S of the previous tile) + w (b - a).  The a rows are read HERE,
                    // not with the prefetch (18 more staged registers spill at two workgroups per CU); the other workgroup of the CU covers the wait
                    const float* aL = w.masks + ((size_t)(stem * p.ntiles + ov.j1 - 1) * 2) * tf + (size_t)(ov.k + p.T - O) * p.F;
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        const int km = min(min(tid + 256 * j, 2048), p.F - 1);
                        gl[j] = srt_blend(aL[km], gl[j], ov.w); gr[j] = srt_blend(aL[tf + km], gr[j], ov.w);
                    }
                }
            }
            if constexpr (RATIO) {
                if (has_mask && (p.ratio || OV)) {       // normalise this frame's mask values across the stems (they arrived with the spectrum rows)
                    const int tile = OV ? ov.j1 : f / p.T, t = OV ? ov.k : f % p.T;
                    const float* r0 = w.masks + ((size_t)tile * 2) * tf + (size_t)t * p.F;
                    if constexpr (SEAM) asm volatile("" : "+s"(r0));      // (the same for the mask rows: with two sets of lane addresses resident across the frame loop this form spills 16 dwords)
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        const int km = min(min(tid + 256 * j, 2048), p.F - 1);
                        if constexpr (SEAM) {            // as OV, a from the carry on the piece's first O rows
                            const float* a0 = sm ? seam + (size_t)ov.k * p.F : r0 - 2 * tf + (size_t)(p.T - O) * p.F;
                            gl[j] = srt_ratio_of_ov<true>(r0, a0, ov.two || sm, ov.w, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km, p.ratio != 0, a_stem);
                            gr[j] = srt_ratio_of_ov<true>(r0 + tf, a0 + a_ch, ov.two || sm, ov.w, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km, p.ratio != 0, a_stem);
                        } else if constexpr (OV) {       // every stem's masks, this one's included, are blended the same way before the squares are summed
                            const float* a0 = r0 - 2 * tf + (size_t)(p.T - O) * p.F;
                            gl[j] = srt_ratio_of_ov(r0, a0, ov.two, ov.w, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km, p.ratio != 0);
                            gr[j] = srt_ratio_of_ov(r0 + tf, a0 + tf, ov.two, ov.w, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km, p.ratio != 0);
                        } else {
                            gl[j] = srt_ratio_of(gl[j], r0, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km);
                            gr[j] = srt_ratio_of(gr[j], r0 + tf, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km);
                        }
                    }
                }
            }
            if constexpr (MIX) {                         // every stem's gains of this frame, chained with output `stem`'s matrix row
                const int tile = OV ? ov.j1 : f / p.T, t = OV ? ov.k : f % p.T;
                const float* r0 = has_mask ? w.masks + ((size_t)tile * 2) * tf + (size_t)t * p.F : nullptr;
                const float* a0 = OV && has_mask ? r0 - 2 * tf + (size_t)(p.T - O) * p.F : r0;
                if constexpr (SEAM) srt_mix_gains<9, 3, decltype(gsrc), true>(p, gsrc, r0, sm && has_mask ? seam + (size_t)ov.k * p.F : a0, ov.two || sm, ov.w, p.ratio && p.nstems > 1, tid, gl, gr, a_stem, a_ch);
                else
                srt_mix_gains<9, 3>(p, gsrc, r0, a0, OV && ov.two, ov.w, p.ratio && p.nstems > 1, tid, gl, gr);
                if constexpr (EXT) { const size_t fu = (size_t)__builtin_amdgcn_readfirstlane(f) * 2; eL = srt_mix_chain(p, gsrc, ext + fu, p.ext_stem); eR = srt_mix_chain(p, gsrc, ext + fu + 1, p.ext_stem); }
            }
            const float xl = EXT ? eL : oob, xr = EXT ? eR : oob;              // bins >= F
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const int k = tid + 256 * j;
                if (k <= 2048) {
                    const float wl = k < p.F ? (has_mask || MIX ? gl[j] : 1.0f) : xl, wr = k < p.F ? (has_mask || MIX ? gr[j] : 1.0f) : xr;
                    const cf A = sl[j] * wl, B = sr[j] * wr;                      // masked (re, im) of L and R
                    // G = F'_L + i F'_R, F' = re - i im, Hermitian-extended; stored swapped (im,re): inverse-by-forward trick
                    if (k == 0) sx[0] = f2(B.x, A.x);                             // a[0] = re[0]           (stftFix.c:556-557)
                    else if (k == 2048) sx[2048] = f2(B.x - B.y, A.x - A.y);     // rev[2048]: re - im wins (stftFix.c:563-566)
                    else {
                        sx[k] = sub_mi(B, A);                                     // (reR - imL, imR + reL)
                        sx[4096 - k] = herm_hi(B, A);                             // (reR + imL, reL - imR)
                    }
                }
            }
            __syncthreads();
            cf v[16];
#pragma unroll
            for (int n2 = 0; n2 < 16; ++n2) v[n2] = sx[tid + 256 * n2];
            __builtin_amdgcn_s_waitcnt(0x0F70);          // all of this frame's rows have arrived (also the ones only lane 0 uses): nothing below waits on the stores
            if (f > f0) emit_and_slide(f - 1);
            fetch(min(f + 1, w.frames - 1));            // the staging registers are free again: next frame's rows fly under this FFT
            // exchange 1 in sy (free: its previous contents, the previous frame's exchange 2, were read before the barrier above),
            // exchange 2 back in sx (every thread has read its staged values before the transform's first barrier)
            fft4096_pp(v, sy, sx, twa, s_twb, tid);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                acc[k2 >> 2][k2 & 3] = __builtin_elementwise_fma(v[FFT16_AT(k2)], f2(pw[k2], pw[k2]), acc[k2 >> 2][k2 & 3]);   // swapped back: L = .y, R = .x
            }
            { cf* t = sx; sx = sy; sy = t; }            // next frame stages where this frame's exchange 1 was (read before the second barrier)
        } else if (f > f0) emit_and_slide(f - 1);
    }
    if (s1 > f0) emit_and_slide(s1 - 1);                // the last segment of the run
}

template <bool RATIO = false>
__global__ void __launch_bounds__(256, 2) srt_istft_ola_kernel(const SrtIstftParams p, int G)
{
    // 1-D launch in XCD order, stem fastest: the nstems workgroups that walk the SAME run of frames sit next to each other on
    // one XCD, so the spectrum rows the first of them pulls from HBM are L2 hits for the others (each stem re-read them before).
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[ISTFT_OLA_LDS_F2];
    istft_ola_run<RATIO>(p, istft_view(p), stem, run, G, s_mem);
}
// the same with overlapped network tiles: p.masks in the overlapped layout, p.ntiles = srtOverlapTiles(frames), O = rows two consecutive tiles share (1..T/2)
template <bool RATIO = false>
__global__ void __launch_bounds__(256, 2) srt_istft_ola_ov_kernel(const SrtIstftParams p, int G, int O)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[ISTFT_OLA_LDS_F2];
    istft_ola_run<RATIO, true>(p, istft_view(p), stem, run, G, s_mem, O);
}
// the two with the average mask extension (p.ext; the names stay apart so that the forms above keep theirs)
template <bool RATIO = false>
__global__ void __launch_bounds__(256, 2) srt_istft_ola_ext_kernel(const SrtIstftParams p, int G)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[ISTFT_OLA_LDS_F2];
    istft_ola_run<RATIO, false, true>(p, istft_view(p), stem, run, G, s_mem);
}
template <bool RATIO = false>
__global__ void __launch_bounds__(256, 2) srt_istft_ola_ov_ext_kernel(const SrtIstftParams p, int G, int O)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[ISTFT_OLA_LDS_F2];
    istft_ola_run<RATIO, true, true>(p, istft_view(p), stem, run, G, s_mem, O);
}


// ------------------------------------------------------------------------------------------- three workgroups per CU
// Through round 4 both transforms held 2 workgroups per CU (250 / 190 VGPRs, 71.5 KB of LDS each - srt_istft_ola_kernel above is that form, kept for
// F > 1024): with one transform per workgroup in flight the VALU, the LDS pipe and HBM take turns instead of overlapping (r04 counters: active 0.36,
// wait 0.21 of the wave cycles, 0.33 / 0.53 of the HBM roofline).  The forms below fit THREE workgroups per CU (<= 168 VGPRs, <= 53 KB LDS; measured on
// the 64-tile batch: iSTFT 0.587 -> 0.480 ms, STFT 0.212 -> 0.204 ms):
//   * pass-1 twiddles from one register pair (fft_twiddle_powers) and, in the inverse, the synthesis window rebuilt from two registers per frame;
//   * ONE exchange buffer (4 barriers per frame instead of 3: exchange 2 waits until every thread has read exchange 1);
//   * no natural-order staging / result buffer.  What both kernels really need from LDS besides the two FFT exchanges is the HERMITIAN MIRROR:
//     thread t owns indices t + 256 j; for j < 8 these are bins k < 2048, and the partner index 4096 - k = (256 - t) + 256 (15 - j) belongs to thread
//     256 - t, slot 15 - j.  So only the upper half travels through LDS, 2049 values in `mir`: slot (j', t') at j' * 256 + t', read back at
//     (15 - n2) * 256 + 256 - t (thread 0 is its own partner; its "thread 256" column is the extra entry 2048, see each kernel) - 16 KB written and
//     read per frame instead of 32 + 32 KB, reversed-contiguous (conflict-free) on both sides.
// LDS: 4352 + 2049 + 240 complex = 53 128 bytes.
#define FFT_MIR_F2 2049
// pass-1 twiddles W^(tid*k0), k0 = 1..15, from ONE register pair w1 = W^tid: powers by binary splitting (every factor is at most three products
// deep, so the twiddles carry <= ~4 roundings = 2.4e-7 relative - inside the transform's own rounding) instead of 15 resident pairs (30 VGPRs).
__device__ __forceinline__ void fft_twiddle_powers(cf (&v)[16], cf w1)
{
    const cf w2 = cmul(w1, w1), w4 = cmul(w2, w2), w8 = cmul(w4, w4);
    const cf w3 = cmul(w1, w2), w5 = cmul(w1, w4), w6 = cmul(w2, w4), w7 = cmul(w3, w4);
    const cf lowp[8] = { f2(1.f, 0.f), w1, w2, w3, w4, w5, w6, w7 };
#pragma unroll
    for (int k0 = 1; k0 < 8; ++k0) v[FFT16_AT(k0)] = cmul(v[FFT16_AT(k0)], lowp[k0]);
    v[FFT16_AT(8)] = cmul(v[FFT16_AT(8)], w8);
#pragma unroll
    for (int k0 = 9; k0 < 16; ++k0) v[FFT16_AT(k0)] = cmul(cmul(v[FFT16_AT(k0)], w8), lowp[k0 - 8]);
}
__device__ __forceinline__ void fft4096_1b(cf (&v)[16], cf* x, const cf w1, const cf* twb, int tid)
{
    // in : v[n2] = x[tid + 256*n2]; `x` free (every thread is past its last read of the previous frame's exchange 2: the caller's barrier)
    // out: v[FFT16_AT(k2)] = X[tid + 256*k2]; `x` holds exchange 2 until the caller's next barrier
    fft16(v);
    fft_twiddle_powers(v, w1);
#pragma unroll
    for (int k0 = 0; k0 < 16; ++k0) x[k0 * FFT_EX1_LD + tid] = v[FFT16_AT(k0)];
    __syncthreads();
    const int lo = tid & 15, hi = tid >> 4;
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) v[n1] = x[hi * FFT_EX1_LD + n1 * 16 + lo];
    fft16(v);
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) v[FFT16_AT(k1)] = cmul(v[FFT16_AT(k1)], twb[(k1 - 1) * 16 + lo]);
    __syncthreads();                                     // every thread has read exchange 1
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) x[lo * FFT_EX2_LD + k1 * 16 + hi] = v[FFT16_AT(k1)];
    __syncthreads();
#pragma unroll
    for (int n0 = 0; n0 < 16; ++n0) v[n0] = x[n0 * FFT_EX2_LD + tid];
    fft16(v);
}

// The signal a workgroup of the forward kernels transforms: the whole call's (srt_stft_kernel), or one track of a packed batch (srt_stft_batch_kernel:
// its own PCM and frame counts, spectrum and magnitudes offset to its first packed row / tile).
struct StftView { const float* L; const float* R; size_t nsamples; int frames_computed, rows_total; float2* spec; float* mag; };
__device__ __forceinline__ StftView stft_view(const SrtStftParams& p) { StftView v = { p.L, p.R, p.nsamples, p.frames_computed, p.rows_total, p.spec, p.mag }; return v; }

// frames [blk * fpb, (blk + 1) * fpb) of the view (rows past rows_total are not this call's)
// OV: overlapped network tiles (srt_ov_row): a magnitude row goes to its primary tile and, inside an overlap, to row k + S of the previous tile too -
// both from the epilogue's registers (the spectrum is unchanged); nt = srtOverlapTiles(rows_total)
template <bool OV = false>
__device__ __forceinline__ void stft_run(const SrtStftParams& p, const StftView& w, int blk, int fpb, cf* s_mem, int O = 0, int nt = 0)
{
    cf* sx = s_mem;
    cf* mir = s_mem + FFT_SMEM_F2;
    cf* s_twb = mir + FFT_MIR_F2;
    const int tid = threadIdx.x;
    const cf w1 = reinterpret_cast<const cf*>(p.tab.twiddle)[tid];
    if (tid < FFT_TWB_F2) s_twb[tid] = reinterpret_cast<const cf*>(p.tab.twiddle)[(16 * (tid & 15) * (tid / 16 + 1)) & 4095];
    float nxtL[16], nxtR[16];
    float aw[16];
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) aw[n2] = p.tab.preWin[tid + 256 * n2];
    auto fetch = [&](int f) {
        const size_t pos = (size_t)f * SRT_HOP;
#pragma unroll
        for (int n2 = 0; n2 < 16; ++n2) {
            const int n = tid + 256 * n2;
            const size_t q = pos + n < w.nsamples ? pos + n : 0;
            nxtL[n2] = w.L[q]; nxtR[n2] = w.R[q];
        }
    };
    // Consecutive frames share three of their four hops, and thread tid's samples tid + 256 n2 of frame f + 1 are its samples n2 + 4 of frame f: the staging
    // registers slide by one hop and only the NEW hop is loaded (4 loads per channel and frame instead of 16).  Round 5's counters had this kernel fetching 0.45 GB
    // for 0.13 GB of PCM: most of the 4x frame overlap came from the fabric again.
    auto fetch_slide = [&](int f) {                      // the registers hold frame f - 1
        const size_t pos = (size_t)f * SRT_HOP;
#pragma unroll
        for (int n2 = 0; n2 < 12; ++n2) { nxtL[n2] = nxtL[n2 + 4]; nxtR[n2] = nxtR[n2 + 4]; }
#pragma unroll
        for (int n2 = 12; n2 < 16; ++n2) {
            const int n = tid + 256 * n2;
            const size_t q = pos + n < w.nsamples ? pos + n : 0;
            nxtL[n2] = w.L[q]; nxtR[n2] = w.R[q];
        }
    };
    const int flast = max(w.frames_computed, 1) - 1;
    fetch(min((int)(blk * fpb), flast));
    __syncthreads();                                     // the pass-2 twiddles are in LDS
    for (int fi = 0; fi < fpb; ++fi) {
        const int f = blk * fpb + fi;
        if (f >= w.rows_total) break;
        const OvRow ov = OV ? srt_ov_row(f, p.T, O, nt) : OvRow{ 0, 0, false, 0.0f };
        const int tile = OV ? ov.j1 : f / p.T, t = OV ? ov.k : f % p.T;
        const bool two = OV && w.mag && ov.two;          // the row is in an overlap (workgroup-uniform)
        float* magL = w.mag ? w.mag + ((size_t)(tile * 2 + 0) * p.T + t) * p.F : nullptr;
        float* magR = w.mag ? w.mag + ((size_t)(tile * 2 + 1) * p.T + t) * p.F : nullptr;
        const size_t prev = (size_t)(p.T + O) * p.F;     // floats from (tile, ch, t) back to (tile - 1, ch, t + S)
        cf* specL = reinterpret_cast<cf*>(w.spec) + (size_t)f * SRT_SPEC_LD;
        cf* specR = specL + p.spec_ch_stride;
        if (f >= w.frames_computed) {                    // rows the reference leaves calloc'ed (stftFix.c:368-371)
            for (int k = tid; k < SRT_SPEC_LD; k += 256) { specL[k] = f2(0.f, 0.f); specR[k] = f2(0.f, 0.f); }
            if (w.mag) for (int k = tid; k < p.F; k += 256) { magL[k] = 0.f; magR[k] = 0.f; }
            if constexpr (OV) { if (two) for (int k = tid; k < p.F; k += 256) { (magL - prev)[k] = 0.f; (magR - prev)[k] = 0.f; } }
            continue;
        }
        cf v[16];
#pragma unroll
        for (int n2 = 0; n2 < 16; ++n2) {
            const bool ok = (size_t)f * SRT_HOP + tid + 256 * n2 < w.nsamples;   // tail frame is zero padded (stftFix.c:460-472)
            v[n2] = f2(nxtL[n2], nxtR[n2]) * (ok ? aw[n2] : 0.f);
        }
        if (f + 1 <= flast) fetch_slide(f + 1);          // the next frame's new hop flies under this transform (past the last frame nothing is needed)
        fft4096_1b(v, sx, w1, s_twb, tid);               // v[FFT16_AT(k2)] = Z[tid + 256 k2]
        // upper half into the mirror buffer: slot (k2 - 8, tid); entry 2048 = Z[0] (partner of bin 0, read by thread 0 through its "column 256")
#pragma unroll
        for (int k2 = 8; k2 < 16; ++k2) mir[(k2 - 8) * 256 + tid] = v[FFT16_AT(k2)];
        if (tid == 0) mir[2048] = v[FFT16_AT(0)];
        const cf z2048 = v[FFT16_AT(8)];                 // thread 0: Z[2048], its own partner
        __syncthreads();                                 // also: every thread is done with exchange 2 (sx is free for the next frame)
        // separate the two real spectra; stored spectrum = conj(F) (the reference's re/im convention)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = tid + 256 * j;
            const cf zk = v[FFT16_AT(j)], zm = mir[(7 - j) * 256 + 256 - tid];
            const cf sl = split_l(zk, zm), sr = split_r(zk, zm);
            if (w.mag && k < p.F) {
                magL[k] = hypotf(sl.x, sl.y) * 4096.0f;              // main.c:468-469
                magR[k] = hypotf(sr.x, sr.y) * 4096.0f;
                if constexpr (OV) { if (two) { (magL - prev)[k] = hypotf(sl.x, sl.y) * 4096.0f; (magR - prev)[k] = hypotf(sr.x, sr.y) * 4096.0f; } }
            }
            specL[k] = sl;
            specR[k] = sr;
        }
        if (tid < SRT_SPEC_LD - 2048) {                  // bin 2048 and the zero padding of the row
            const cf sl = tid == 0 ? split_l(z2048, z2048) : f2(0.f, 0.f), sr = tid == 0 ? split_r(z2048, z2048) : f2(0.f, 0.f);
            specL[2048 + tid] = sl;
            specR[2048 + tid] = sr;
            if (w.mag && tid == 0 && 2048 < p.F) { magL[2048] = hypotf(sl.x, sl.y) * 4096.0f; magR[2048] = hypotf(sr.x, sr.y) * 4096.0f; }
            if constexpr (OV) { if (two && tid == 0 && 2048 < p.F) { (magL - prev)[2048] = hypotf(sl.x, sl.y) * 4096.0f; (magR - prev)[2048] = hypotf(sr.x, sr.y) * 4096.0f; } }
        }
    }
}

__global__ void __launch_bounds__(256, 3) srt_stft_kernel(const SrtStftParams p, int fpb)
{
    __shared__ cf s_mem[FFT_SMEM_F2 + FFT_MIR_F2 + FFT_TWB_F2];
    stft_run(p, stft_view(p), blockIdx.x, fpb, s_mem);
}
// the same with overlapped network tiles: p.mag is [nt][2][T][F] with nt = srtOverlapTiles(rows_total), O = rows two consecutive tiles share (1..T/2)
__global__ void __launch_bounds__(256, 3) srt_stft_ov_kernel(const SrtStftParams p, int fpb, int O, int nt)
{
    __shared__ cf s_mem[FFT_SMEM_F2 + FFT_MIR_F2 + FFT_TWB_F2];
    stft_run<true>(p, stft_view(p), blockIdx.x, fpb, s_mem, O, nt);
}

// NM: mask rows cover bins < F <= 256 NM, so only the first NM of a thread's eight bins can carry a mask value (F = 1024: 4 prefetch registers per channel instead of 8)
// M16: the masks are halves (the engine's own mask buffer in the fp16 mode, written by srt_head_rows_kernel<.., true>; never with RATIO)
#define ISTFT_OLA3_LDS_F2 (FFT_SMEM_F2 + FFT_MIR_F2 + FFT_TWB_F2)
// EXT: as istft_ola_run
// MIX: as istft_ola_run (RATIO = M16 = false)
// TRK, GTAB: as istft_ola_run
// SEAM: as istft_ola_run (float masks: M16 = false)
template <int NM, bool RATIO, bool M16, bool OV = false, bool EXT = false, bool MIX = false, bool TRK = false, bool GTAB = false, bool SEAM = false>
__device__ __forceinline__ void istft_ola3_run(const SrtIstftParams& p, const IstftView& w, int stem, int run, int G, cf* s_mem, int O = 0, int ov_tiles = 0, const float* seam = nullptr)
{
    static_assert(!SEAM || (OV && !TRK && !M16), "the seam carry belongs to one signal's overlapped tiles and holds floats");
    cf* sx = s_mem;
    cf* mir = s_mem + FFT_SMEM_F2;
    cf* s_twb = mir + FFT_MIR_F2;
    const int tid = threadIdx.x;
    const cf w1 = reinterpret_cast<const cf*>(p.tab.twiddle)[tid];
    if (tid < FFT_TWB_F2) s_twb[tid] = reinterpret_cast<const cf*>(p.tab.twiddle)[(16 * (tid & 15) * (tid / 16 + 1)) & 4095];
    const size_t tf = (size_t)p.T * p.F;
    const int nseg = w.frames + 3;
    const int s0 = run * G, s1 = min(s0 + G, nseg);
    const auto gsrc = srt_mix_source<GTAB>(p, w, stem);
    const float oob = MIX ? srt_mix_chain(p, gsrc, p.oob, 1) : p.oob[stem];   // bins >= F: "unaffectedWeight" (main.c:486-493)
    const cf* spec = reinterpret_cast<const cf*>(w.spec);
    float* oL = w.out + (size_t)(stem * 2 + 0) * w.out_len;
    float* oR = w.out + (size_t)(stem * 2 + 1) * w.out_len;
    cf acc[4][4];                                       // [segment slot][j] = (R, L) pairs
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[h][j] = f2(0.0f, 0.0f);
    cf sl[8], sr[8];
    float gl[NM], gr[NM];
    cf sl8, sr8;                                        // bin 2048 (only thread 0 uses it; the address is uniform)
    float eL = oob, eR = oob;
    const float* __restrict__ const ext = EXT ? w.ext + (MIX ? 0 : (size_t)stem * p.ext_stem) : nullptr;
    const bool has_mask = w.masks != nullptr;
    auto fetch = [&](int f) {                                               // 0 <= f < w.frames
        int tile = f / p.T, t = f % p.T;
        OvRow ov = { 0, 0, false, 0.0f };
        if constexpr (OV) { ov = srt_ov_row(f, p.T, O, TRK ? ov_tiles : p.ntiles); tile = ov.j1; t = ov.k; }
        const cf* specL = spec + (size_t)f * SRT_SPEC_LD;
        const cf* specR = specL + p.spec_ch_stride;
        const size_t mo = ((size_t)(stem * p.ntiles + tile) * 2) * tf + (size_t)t * p.F;
        const float* mL = has_mask ? w.masks + mo : p.tab.postWin;
        const float* mR = has_mask ? mL + tf : p.tab.postWin;
        const _Float16* hL = reinterpret_cast<const _Float16*>(w.masks) + mo;                   // (M16: the launcher checks that masks are given)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = tid + 256 * j;
            sl[j] = specL[k]; sr[j] = specR[k];
            if (j < NM) {
                const int km = min(k, p.F - 1);
                if constexpr (M16) { gl[j] = (float)hL[km]; gr[j] = (float)hL[tf + km]; }
                else if constexpr (!(RATIO && OV) && !MIX) { gl[j] = mL[km]; gr[j] = mR[km]; }      // (RATIO && OV: see srt_ratio_of_ov)
            }
        }
        sl8 = specL[2048]; sr8 = specR[2048];
        if constexpr (EXT && !MIX) { const size_t fu = (size_t)__builtin_amdgcn_readfirstlane(f) * 2; eL = ext[fu]; eR = ext[fu + 1]; }
    };
    // the 16 synthesis-window taps of this thread (samples tid + 256 k2) are rebuilt per frame from two registers: cos / sin of th = 2 pi (tid + 1/2) / 4096, over 3.
    // (A deviation from the table the F > 1024 kernel reads - postWin, which reproduces InitSTFT's rounding: 1/3 - cos/3 in fp32 is off by up to ~3e-8 absolute,
    // which is a large RELATIVE error only on the ~1e-7 taps at the window's edges.  tests/test_gpu_parity.py::test_istft_three_per_cu_kernel_against_the_table_kernel
    // bounds the two kernels against each other on identical input at 5e-7 of the output's peak (measured 3.1e-7).)
    float ws3, wc3;
    sincospif((tid + 0.5f) * (1.0f / 2048.0f), &ws3, &wc3);
    ws3 *= 1.0f / 3.0f; wc3 *= 1.0f / 3.0f;
    constexpr float COS_PI8[16] = { 1.0f, 0.92387953251128675613f, 0.70710678118654752440f, 0.38268343236508977173f, 0.0f, -0.38268343236508977173f, -0.70710678118654752440f, -0.92387953251128675613f,
                                    -1.0f, -0.92387953251128675613f, -0.70710678118654752440f, -0.38268343236508977173f, 0.0f, 0.38268343236508977173f, 0.70710678118654752440f, 0.92387953251128675613f };
    constexpr float SIN_PI8[16] = { 0.0f, 0.38268343236508977173f, 0.70710678118654752440f, 0.92387953251128675613f, 1.0f, 0.92387953251128675613f, 0.70710678118654752440f, 0.38268343236508977173f,
                                    0.0f, -0.38268343236508977173f, -0.70710678118654752440f, -0.92387953251128675613f, -1.0f, -0.92387953251128675613f, -0.70710678118654752440f, -0.38268343236508977173f };
    const int f0 = max(s0 - 3, 0);
    if (f0 < w.frames) fetch(f0);
    __syncthreads();                                     // the pass-2 twiddles are in LDS
    auto emit_and_slide = [&](int seg) {
        if (seg >= s0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { oL[(size_t)seg * SRT_HOP + tid + 256 * j] = acc[0][j].y; oR[(size_t)seg * SRT_HOP + tid + 256 * j] = acc[0][j].x; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[0][j] = acc[1][j]; acc[1][j] = acc[2][j]; acc[2][j] = acc[3][j]; acc[3][j] = f2(0.0f, 0.0f);
        }
    };
    for (int f = f0; f < s1; ++f) {
        if (f < w.frames) {
            // G = F'_L + i F'_R, F' = re - i im, Hermitian-extended; kept swapped (im, re): inverse-by-forward trick.  Bins k = tid + 256 j < 2048 are this
            // thread's own transform inputs n2 = j; their partners 4096 - k go through `mir` to thread 256 - tid (slot 15 - j).
            cf v[16];
            OvRow ov = { 0, 0, false, 0.0f };
            bool sm = false;                             // SEAM: as in istft_ola_run
            size_t a_stem = 0, a_ch = 0;
            if constexpr (OV) {
                ov = srt_ov_row(f, p.T, O, TRK ? ov_tiles : p.ntiles);
                if constexpr (SEAM) {
                    asm volatile("" : "+s"(seam));       // the carry's lane addresses are formed per frame: hoisted out of the frame loop they would be 2 x NB more resident VGPRs
                    sm = srt_ov_seam(ov, O, seam);
                    a_ch = sm ? (size_t)O * p.F : tf; a_stem = sm ? 2 * (size_t)O * p.F : (size_t)p.ntiles * 2 * tf;
                    if (!RATIO && !MIX && has_mask && (ov.two || sm)) {      // as below, a from the carry on the piece's first O rows
                        const float* aL = sm ? seam + (size_t)stem * a_stem + (size_t)ov.k * p.F : w.masks + ((size_t)(stem * p.ntiles + ov.j1 - 1) * 2) * tf + (size_t)(ov.k + p.T - O) * p.F;
#pragma unroll
                        for (int j = 0; j < NM; ++j) {
                            const int km = min(tid + 256 * j, p.F - 1);
                            gl[j] = srt_blend(aL[km], gl[j], ov.w); gr[j] = srt_blend(aL[a_ch + km], gr[j], ov.w);
                        }
                    }
                } else
                if (!RATIO && !MIX && has_mask && ov.two) {      // cross-fade of the two tiles' masks (halves are converted first): a (row k + S of the previous tile) + w (b - a).
                    // The a rows are read HERE, not with the prefetch: eight more staged registers do not fit the 168 of three workgroups per CU (9 dwords
                    // spilled when tried); the wait is covered by the CU's other workgroups and falls on O of every T - O frames only
                    const size_t ao = ((size_t)(stem * p.ntiles + ov.j1 - 1) * 2) * tf + (size_t)(ov.k + p.T - O) * p.F;
                    const _Float16* hA = reinterpret_cast<const _Float16*>(w.masks) + ao;
#pragma unroll
                    for (int j = 0; j < NM; ++j) {
                        const int km = min(tid + 256 * j, p.F - 1);
                        const float al = M16 ? (float)hA[km] : w.masks[ao + km], ar = M16 ? (float)hA[tf + km] : w.masks[ao + tf + km];
                        gl[j] = srt_blend(al, gl[j], ov.w); gr[j] = srt_blend(ar, gr[j], ov.w);
                    }
                }
            }
            if constexpr (RATIO) {
                if (has_mask && (p.ratio || OV)) {       // (see srt_ratio_of; the extra loads are why this instantiation is built for two workgroups per CU)
                    const int tile = OV ? ov.j1 : f / p.T, t = OV ? ov.k : f % p.T;
                    const float* r0 = w.masks + ((size_t)tile * 2) * tf + (size_t)t * p.F;
#pragma unroll
                    for (int j = 0; j < NM; ++j) {
                        const int km = min(tid + 256 * j, p.F - 1);
                        if constexpr (SEAM) {            // as OV, a from the carry on the piece's first O rows
                            const float* a0 = sm ? seam + (size_t)ov.k * p.F : r0 - 2 * tf + (size_t)(p.T - O) * p.F;
                            gl[j] = srt_ratio_of_ov<true>(r0, a0, ov.two || sm, ov.w, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km, p.ratio != 0, a_stem);
                            gr[j] = srt_ratio_of_ov<true>(r0 + tf, a0 + a_ch, ov.two || sm, ov.w, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km, p.ratio != 0, a_stem);
                        } else if constexpr (OV) {       // every stem's masks, this one's included, are blended the same way before the squares are summed
                            const float* a0 = r0 - 2 * tf + (size_t)(p.T - O) * p.F;
                            gl[j] = srt_ratio_of_ov(r0, a0, ov.two, ov.w, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km, p.ratio != 0);
                            gr[j] = srt_ratio_of_ov(r0 + tf, a0 + tf, ov.two, ov.w, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km, p.ratio != 0);
                        } else {
                            gl[j] = srt_ratio_of(gl[j], r0, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km);
                            gr[j] = srt_ratio_of(gr[j], r0 + tf, (size_t)p.ntiles * 2 * tf, p.nstems, stem, km);
                        }
                    }
                }
            }
            if constexpr (MIX) {                         // every stem's gains of this frame, chained with output `stem`'s matrix row
                const int tile = OV ? ov.j1 : f / p.T, t = OV ? ov.k : f % p.T;
                const float* r0 = has_mask ? w.masks + ((size_t)tile * 2) * tf + (size_t)t * p.F : nullptr;
                const float* a0 = OV && has_mask ? r0 - 2 * tf + (size_t)(p.T - O) * p.F : r0;
                if constexpr (SEAM) srt_mix_gains<NM, NM, decltype(gsrc), true>(p, gsrc, r0, sm && has_mask ? seam + (size_t)ov.k * p.F : a0, ov.two || sm, ov.w, p.ratio && p.nstems > 1, tid, gl, gr, a_stem, a_ch);
                else
                srt_mix_gains<NM, NM>(p, gsrc, r0, a0, OV && ov.two, ov.w, p.ratio && p.nstems > 1, tid, gl, gr);
                if constexpr (EXT) { const size_t fu = (size_t)__builtin_amdgcn_readfirstlane(f) * 2; eL = srt_mix_chain(p, gsrc, ext + fu, p.ext_stem); eR = srt_mix_chain(p, gsrc, ext + fu + 1, p.ext_stem); }
            }
            const float xl = EXT ? eL : oob, xr = EXT ? eR : oob;              // bins >= F
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = tid + 256 * j;
                float wl = xl, wr = xr;
                if (j < NM) { wl = k < p.F ? (has_mask || MIX ? gl[j] : 1.0f) : xl; wr = k < p.F ? (has_mask || MIX ? gr[j] : 1.0f) : xr; }
                const cf A = sl[j] * wl, B = sr[j] * wr;                          // masked (re, im) of L and R
                v[j] = sub_mi(B, A);                                              // (reR - imL, imR + reL)
                mir[j * 256 + tid] = herm_hi(B, A);                               // (reR + imL, reL - imR)   (slot (0, 0) is never read)
                if (j == 0 && tid == 0) v[0] = f2(B.x, A.x);                      // a[0] = re[0]           (stftFix.c:556-557)
            }
            if (tid == 0) {                                                       // rev[2048]: re - im wins (stftFix.c:563-566); F <= 2048, so bin 2048 is always out of band
                const cf A = sl8 * xl, B = sr8 * xr;
                mir[2048] = f2(B.x - B.y, A.x - A.y);
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);          // all of this frame's rows have arrived: nothing below waits on the stores
            if (f > f0) emit_and_slide(f - 1);
            fetch(min(f + 1, w.frames - 1));             // next frame's rows fly under this transform
            __syncthreads();                             // the mirror values are visible; every thread is past the previous frame's exchange 2
#pragma unroll
            for (int n2 = 8; n2 < 16; ++n2) v[n2] = mir[(15 - n2) * 256 + 256 - tid];
            fft4096_1b(v, sx, w1, s_twb, tid);
            asm volatile("" : "+v"(wc3), "+v"(ws3));     // keeps the 16 taps from being hoisted out of the frame loop (they would come back as 32 resident VGPRs)
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                // synthesis window tap of sample tid + 256 k2: (2/3) hann(i + 1/2) = 1/3 - (cos(th) cos(k2 pi/8) - sin(th) sin(k2 pi/8)) / 3 (stftFix.c:329-341)
                const float pwk = fmaf(-wc3, COS_PI8[k2], fmaf(ws3, SIN_PI8[k2], 1.0f / 3.0f));
                acc[k2 >> 2][k2 & 3] = __builtin_elementwise_fma(v[FFT16_AT(k2)], f2(pwk, pwk), acc[k2 >> 2][k2 & 3]);   // swapped back: L = .y, R = .x
            }
        } else if (f > f0) emit_and_slide(f - 1);
    }
    if (s1 > f0) emit_and_slide(s1 - 1);
}

template <int NM, bool RATIO = false, bool M16 = false>
__global__ void __launch_bounds__(256, RATIO ? 2 : 3) srt_istft_ola3_kernel(const SrtIstftParams p, int G)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;       // stem fastest: the stems of a run share the spectrum rows in L2
    __shared__ cf s_mem[ISTFT_OLA3_LDS_F2];
    istft_ola3_run<NM, RATIO, M16>(p, istft_view(p), stem, run, G, s_mem);
}
// the same with overlapped network tiles (see srt_istft_ola_ov_kernel)
template <int NM, bool RATIO = false, bool M16 = false>
__global__ void __launch_bounds__(256, RATIO ? 2 : 3) srt_istft_ola3_ov_kernel(const SrtIstftParams p, int G, int O)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[ISTFT_OLA3_LDS_F2];
    istft_ola3_run<NM, RATIO, M16, true>(p, istft_view(p), stem, run, G, s_mem, O);
}
// the two with the average mask extension (see srt_istft_ola_ext_kernel)
template <int NM, bool RATIO = false, bool M16 = false>
__global__ void __launch_bounds__(256, RATIO ? 2 : 3) srt_istft_ola3_ext_kernel(const SrtIstftParams p, int G)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[ISTFT_OLA3_LDS_F2];
    istft_ola3_run<NM, RATIO, M16, false, true>(p, istft_view(p), stem, run, G, s_mem);
}
template <int NM, bool RATIO = false, bool M16 = false>
__global__ void __launch_bounds__(256, RATIO ? 2 : 3) srt_istft_ola3_ov_ext_kernel(const SrtIstftParams p, int G, int O)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[ISTFT_OLA3_LDS_F2];
    istft_ola3_run<NM, RATIO, M16, true, true>(p, istft_view(p), stem, run, G, s_mem, O);
}

// Stem remix (srtSetMix): the workgroup index is the OUTPUT m, fastest in the XCD order - the outputs of a run share the spectrum rows (and every stem's mask
// rows) in L2.  Two workgroups per CU as the RATIO forms, which read every stem's row in the prologue too; O is unused without OV.
template <int NM, bool OV, bool EXT>
__global__ void __launch_bounds__(256, 2) srt_istft_ola3_mix_kernel(const SrtIstftParams p, int G, int O)
{
    const int pos = srt_xcd_order(gridDim.x), m = pos % p.n_out, run = pos / p.n_out;
    __shared__ cf s_mem[ISTFT_OLA3_LDS_F2];
    istft_ola3_run<NM, false, false, OV, EXT, true>(p, istft_view(p), m, run, G, s_mem, O);
}
template <bool OV, bool EXT>
__global__ void __launch_bounds__(256, 2) srt_istft_ola_mix_kernel(const SrtIstftParams p, int G, int O)
{
    const int pos = srt_xcd_order(gridDim.x), m = pos % p.n_out, run = pos / p.n_out;
    __shared__ cf s_mem[ISTFT_OLA_LDS_F2];
    istft_ola_run<false, OV, EXT, true>(p, istft_view(p), m, run, G, s_mem, O);
}

// A piece of a longer stream under overlapped tiles (srtSeparateHostStreamOverlap): the overlap forms above with the SEAM bodies - the piece's
// first O rows blend with the mask seam carry `seam` ([nstems][2][O][F] floats, srt_mask_seam_save_kernel).  Float masks only; the workgroups per CU of the OV siblings.
template <int NM, bool RATIO, bool EXT>
__global__ void __launch_bounds__(256, RATIO ? 2 : 3) srt_istft_ola3_seam_kernel(const SrtIstftParams p, int G, int O, const float* __restrict__ seam)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[ISTFT_OLA3_LDS_F2];
    istft_ola3_run<NM, RATIO, false, true, EXT, false, false, false, true>(p, istft_view(p), stem, run, G, s_mem, O, 0, seam);
}
template <bool RATIO, bool EXT>
__global__ void __launch_bounds__(256, 2) srt_istft_ola_seam_kernel(const SrtIstftParams p, int G, int O, const float* __restrict__ seam)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[ISTFT_OLA_LDS_F2];
    istft_ola_run<RATIO, true, EXT, false, false, false, true>(p, istft_view(p), stem, run, G, s_mem, O, 0, seam);
}
template <int NM, bool EXT>
__global__ void __launch_bounds__(256, 2) srt_istft_ola3_seam_bus_kernel(const SrtIstftParams p, int G, int O, const float* __restrict__ seam)
{
    const int pos = srt_xcd_order(gridDim.x), m = pos % p.n_out, run = pos / p.n_out;
    __shared__ cf s_mem[ISTFT_OLA3_LDS_F2];
    istft_ola3_run<NM, false, false, true, EXT, true, false, false, true>(p, istft_view(p), m, run, G, s_mem, O, 0, seam);
}
template <bool EXT>
__global__ void __launch_bounds__(256, 2) srt_istft_ola_seam_bus_kernel(const SrtIstftParams p, int G, int O, const float* __restrict__ seam)
{
    const int pos = srt_xcd_order(gridDim.x), m = pos % p.n_out, run = pos / p.n_out;
    __shared__ cf s_mem[ISTFT_OLA_LDS_F2];
    istft_ola_run<false, true, EXT, true, false, false, true>(p, istft_view(p), m, run, G, s_mem, O, 0, seam);
}

int srt_launch_stft(const SrtStftParams& p, hipStream_t s, int overlap, int ov_tiles)
{
    // short signals (one tile, the real-time regime): fewer frames per workgroup so that the frames spread over the CUs
    int fpb = p.rows_total >= 4096 ? STFT_FPB : (p.rows_total >= 1024 ? 2 : 1);
    if (p.rows_total >= 4096) {                          // whole rounds of the 768 resident workgroups (3 per CU), at most ~24 frames each
        // (round 6, with the sliding staging registers a longer run costs nothing and saves first-frame fetches: cap 6 / 8 / 12 / 24 / 48 -> 0.169 / 0.168 / 0.170 / 0.162 / 0.163 ms)
        constexpr int cap = 24;
        const int slots = 768, rounds = (p.rows_total + slots * cap - 1) / (slots * cap);
        fpb = (p.rows_total + slots * rounds - 1) / (slots * rounds);
    }
    // (tests/test_dsp_float64.py holds every row to float64 at one shape per regime of this rule: rows = 37 -> fpb 1, 1025 -> 2 and 4099 -> 6 (both with a last
    // workgroup of one frame), 9000 -> 12.  Nothing reads this rule from the tests: launcher_fpb / launcher_G in that file restate it and this function's sibling below
    // by hand, for the printed tags only.  Whoever changes a rule edits the restatement and moves the shapes, or the regimes lose their coverage with every test green.
    // tests/test_dsp_float64_forms.py runs srt_stft_ov_kernel at rows = 1025 and 4099 (fpb 2 and 6, O = 16) against this kernel's bits and the O = 0 magnitudes.)
    const int blocks = (p.rows_total + fpb - 1) / fpb;
    if (blocks <= 0) return 0;
    if (overlap > 0) {                                   // the rows of tile j are [j (T - O), j (T - O) + T): every row below rows_total must have a tile
        if (overlap > p.T / 2 || ov_tiles < 1 || (size_t)(ov_tiles - 1) * (p.T - overlap) + p.T < (size_t)p.rows_total) return -1;
        SRT_LAUNCH(srt_stft_ov_kernel, dim3(blocks), dim3(256), 0, s, p, fpb, overlap, ov_tiles);
    } else SRT_LAUNCH(srt_stft_kernel, dim3(blocks), dim3(256), 0, s, p, fpb);
    return srt_launch_status();
}

int srt_launch_istft(const SrtIstftParams& p, hipStream_t s, int overlap, const float* seam)
{
    if (p.frames <= 0) return 0;
    // overlapped tiles: p.ntiles tiles of stride T - O must cover every frame (the kernels index masks by srt_ov_row); without masks there is nothing to blend
    if (overlap < 0 || (overlap > 0 && (overlap > p.T / 2 || p.ntiles < 1 || (size_t)(p.ntiles - 1) * (p.T - overlap) + p.T < (size_t)p.frames))) return -1;
    const int O = p.masks ? overlap : 0;
    const int nseg = p.frames + 3;
    // One launch for all stems (blockIdx.y = stem): ~4 workgroups per CU over the whole grid when the stream is long enough,
    // runs of at least 13 segments so the 3-frame warm-up stays below ~25 % (64-tile batch, 4 stems: G = 65, 4.6 %).
    // three-per-CU form: ONE round of the 768 resident workgroups (64-tile batch, 4 stems: G = 86, warm-up 3.5 %; two rounds measured the same, 1024 / 2304
    // workgroups 6 % / 1 % slower); the two-per-CU form keeps its two rounds of 512
    if (p.masks16 && (!p.masks || p.F > 1024 || (p.ratio && p.nstems > 1))) return -1;      // halves are read by the three-per-CU kernel only
    const int target = p.F > 1024 ? 1024 : 768;
    // (runs x stems must not exceed the resident workgroups: five stems at 768 / 5 = 153.6 runs would leave two workgroups for a second round)
    if (p.n_out < 0 || p.n_out > SRT_MAX_STEMS || (p.n_out && (p.masks16 || p.nstems < 1 || p.nstems > SRT_MAX_STEMS))) return -1;      // remix: fp32 masks only
    const int ncol = p.n_out ? p.n_out : p.nstems;      // workgroup columns of the grid: the stems, or the outputs of a remix
    const int max_runs = target / ncol > 0 ? target / ncol : 1;
    int G = (nseg + max_runs - 1) / max_runs;
    const int gmin = (size_t)nseg * ncol >= 4096 ? 13 : 5;          // short signals: shorter runs (more warm-up, but all CUs busy)
    if (G < gmin) G = gmin;
    // (tests/test_dsp_float64.py, every output hop against float64: frames 1..4 and 13..17, one stem -> G = 5 with nseg mod G taking every value; 1400 frames x 3 stems
    // -> G = 13; 2100 x 5 -> G = 14, 755 workgroups; 4500 x 3 at F = 1088 -> G = 14 on the table kernel.  A change to this rule moves those shapes as well.
    // tests/test_dsp_float64_forms.py, the OV / EXT / MIX / RATIO / SEAM forms below against float64: 145 and 157 frames x 3 stems (2 outputs of a remix) and 277
    // frames in three pieces -> G = 5; one stem at O = 32, frames 4, 13..17 and 65..69 -> G = 5 with nseg mod G taking every value, with and without blended rows
    // inside the runs; 1400 frames x 3 stems at O = 16 -> G = 13 in both families (48 mod 13 = 9: every phase of a tile seam inside a run).)
    const int blocks = (nseg + G - 1) / G;
    // one stem per workgroup: 32 accumulator + 54 prefetch registers + the FFT fit in 256 VGPRs at 2 workgroups per CU
    // F > 1024: eight mask registers per channel do not fit the 168-VGPR budget of the three-per-CU form (22 dwords would spill): the two-per-CU kernel
    if (p.ext && (!p.masks || p.ext_stem < (size_t)p.frames * 2)) return -1;      // the table holds [frames][2] gains per stem, derived from masks
    if (seam) {                                          // a piece of a longer stream: the SEAM forms, chosen as the overlap forms below are (float masks only)
        if (O <= 0 || p.masks16) return -1;
        const bool ratio = p.ratio && p.nstems > 1, big = p.F > 1024;
        const dim3 grid(blocks * ncol), blk(256);
        if (p.n_out) {
            if (big) { if (p.ext) SRT_LAUNCH((srt_istft_ola_seam_bus_kernel<true>), grid, blk, 0, s, p, G, O, seam); else SRT_LAUNCH((srt_istft_ola_seam_bus_kernel<false>), grid, blk, 0, s, p, G, O, seam); }
            else if (p.ext) SRT_LAUNCH((srt_istft_ola3_seam_bus_kernel<4, true>), grid, blk, 0, s, p, G, O, seam);
            else SRT_LAUNCH((srt_istft_ola3_seam_bus_kernel<4, false>), grid, blk, 0, s, p, G, O, seam);
        } else if (big) {
            if (ratio) { if (p.ext) SRT_LAUNCH((srt_istft_ola_seam_kernel<true, true>), grid, blk, 0, s, p, G, O, seam); else SRT_LAUNCH((srt_istft_ola_seam_kernel<true, false>), grid, blk, 0, s, p, G, O, seam); }
            else if (p.ext) SRT_LAUNCH((srt_istft_ola_seam_kernel<false, true>), grid, blk, 0, s, p, G, O, seam);
            else SRT_LAUNCH((srt_istft_ola_seam_kernel<false, false>), grid, blk, 0, s, p, G, O, seam);
        } else if (ratio) { if (p.ext) SRT_LAUNCH((srt_istft_ola3_seam_kernel<4, true, true>), grid, blk, 0, s, p, G, O, seam); else SRT_LAUNCH((srt_istft_ola3_seam_kernel<4, true, false>), grid, blk, 0, s, p, G, O, seam); }
        else if (p.ext) SRT_LAUNCH((srt_istft_ola3_seam_kernel<4, false, true>), grid, blk, 0, s, p, G, O, seam);
        else SRT_LAUNCH((srt_istft_ola3_seam_kernel<4, false, false>), grid, blk, 0, s, p, G, O, seam);
        return srt_launch_status();
    }
    if (p.n_out) {                                      // stem remix: the MIX forms by the same F rule (ratio is their run-time flag)
        const dim3 grid(blocks * p.n_out);
        if (p.F > 1024) {
            if (O > 0 && p.ext) SRT_LAUNCH((srt_istft_ola_mix_kernel<true, true>), grid, dim3(256), 0, s, p, G, O);
            else if (O > 0) SRT_LAUNCH((srt_istft_ola_mix_kernel<true, false>), grid, dim3(256), 0, s, p, G, O);
            else if (p.ext) SRT_LAUNCH((srt_istft_ola_mix_kernel<false, true>), grid, dim3(256), 0, s, p, G, 0);
            else SRT_LAUNCH((srt_istft_ola_mix_kernel<false, false>), grid, dim3(256), 0, s, p, G, 0);
        } else if (O > 0 && p.ext) SRT_LAUNCH((srt_istft_ola3_mix_kernel<4, true, true>), grid, dim3(256), 0, s, p, G, O);
        else if (O > 0) SRT_LAUNCH((srt_istft_ola3_mix_kernel<4, true, false>), grid, dim3(256), 0, s, p, G, O);
        else if (p.ext) SRT_LAUNCH((srt_istft_ola3_mix_kernel<4, false, true>), grid, dim3(256), 0, s, p, G, 0);
        else SRT_LAUNCH((srt_istft_ola3_mix_kernel<4, false, false>), grid, dim3(256), 0, s, p, G, 0);
        return srt_launch_status();
    }
    if (p.ext) {                                         // average mask extension: the same choice among the EXT forms
        const dim3 grid(blocks * p.nstems);
        const bool ratio = p.ratio && p.nstems > 1;
        if (O > 0) {
            if (ratio) {
                if (p.F > 1024) SRT_LAUNCH((srt_istft_ola_ov_ext_kernel<true>), grid, dim3(256), 0, s, p, G, O);
                else SRT_LAUNCH((srt_istft_ola3_ov_ext_kernel<4, true>), grid, dim3(256), 0, s, p, G, O);
            } else if (p.F > 1024) SRT_LAUNCH((srt_istft_ola_ov_ext_kernel<false>), grid, dim3(256), 0, s, p, G, O);
            else if (p.masks16) SRT_LAUNCH((srt_istft_ola3_ov_ext_kernel<4, false, true>), grid, dim3(256), 0, s, p, G, O);
            else SRT_LAUNCH((srt_istft_ola3_ov_ext_kernel<4>), grid, dim3(256), 0, s, p, G, O);
        } else if (ratio) {
            if (p.F > 1024) SRT_LAUNCH((srt_istft_ola_ext_kernel<true>), grid, dim3(256), 0, s, p, G);
            else SRT_LAUNCH((srt_istft_ola3_ext_kernel<4, true>), grid, dim3(256), 0, s, p, G);
        } else if (p.F > 1024) SRT_LAUNCH((srt_istft_ola_ext_kernel<false>), grid, dim3(256), 0, s, p, G);
        else if (p.masks16) SRT_LAUNCH((srt_istft_ola3_ext_kernel<4, false, true>), grid, dim3(256), 0, s, p, G);
        else SRT_LAUNCH((srt_istft_ola3_ext_kernel<4>), grid, dim3(256), 0, s, p, G);
        return srt_launch_status();
    }
    if (O > 0) {                                         // the overlap instantiations (the forms below keep their code)
        const dim3 grid(blocks * p.nstems);
        if (p.ratio && p.nstems > 1) {
            if (p.F > 1024) SRT_LAUNCH((srt_istft_ola_ov_kernel<true>), grid, dim3(256), 0, s, p, G, O);
            else SRT_LAUNCH((srt_istft_ola3_ov_kernel<4, true>), grid, dim3(256), 0, s, p, G, O);
        } else if (p.F > 1024) SRT_LAUNCH((srt_istft_ola_ov_kernel<false>), grid, dim3(256), 0, s, p, G, O);
        else if (p.masks16) SRT_LAUNCH((srt_istft_ola3_ov_kernel<4, false, true>), grid, dim3(256), 0, s, p, G, O);
        else SRT_LAUNCH((srt_istft_ola3_ov_kernel<4>), grid, dim3(256), 0, s, p, G, O);
        return srt_launch_status();
    }
    if (p.ratio && p.masks && p.nstems > 1) {            // cross-stem ratio mask applied in the prologue (srt_ratio_of)
        if (p.F > 1024) SRT_LAUNCH((srt_istft_ola_kernel<true>), dim3(blocks * p.nstems), dim3(256), 0, s, p, G);
        else SRT_LAUNCH((srt_istft_ola3_kernel<4, true>), dim3(blocks * p.nstems), dim3(256), 0, s, p, G);
    } else if (p.F > 1024) SRT_LAUNCH((srt_istft_ola_kernel<false>), dim3(blocks * p.nstems), dim3(256), 0, s, p, G);
    else if (p.masks16) SRT_LAUNCH((srt_istft_ola3_kernel<4, false, true>), dim3(blocks * p.nstems), dim3(256), 0, s, p, G);
    else SRT_LAUNCH((srt_istft_ola3_kernel<4>), dim3(blocks * p.nstems), dim3(256), 0, s, p, G);
    return srt_launch_status();
}

// ------------------------------------------------------------------------------------------- average mask extension (srtSetMaskExtension)
// ext[s][r][c] = (sum over k < F of g_s(r, c, k)) / F, g = the in-band gain the inverse kernels above apply to stem s at row r, channel c: the mask value
// (halves converted), cross-faded between the two tiles of an overlapped row (srt_blend), normalised across the stems (srt_ratio_of / srt_ratio_of_ov) - formed
// by the very helpers the inverse kernels call, so the averaged values are bit for bit the applied ones.  The EXT inverse instantiations multiply bins >= F of
// that row and channel by it.  One wave per (row, channel), all stems at once (the ratio needs every stem's value of a bin): a lane loads 16 bytes per stem and
// step, the wave's lanes contiguous, and adds its values in ascending k into one running sum per stem; then a fixed xor butterfly over the 64 lanes and a true
// division by F.  The order depends on F alone - not on the grid, the batch packing or the chunking - and the longest chain is F / 64 + 6 additions.
// No atomics, no LDS.  NS (the stem count), the mask type, the ratio and the overlap are compile-time: the stem loops unroll over registers and no load
// sits behind a per-element select.
#pragma clang fp contract(off)
template <bool M16>
__device__ __forceinline__ void srt_mask_load16(const float* __restrict__ masks, size_t off, float (&v)[M16 ? 8 : 4])
{
    if constexpr (M16) {
        typedef _Float16 half8 __attribute__((ext_vector_type(8)));
        const half8 h = *reinterpret_cast<const half8*>(reinterpret_cast<const _Float16*>(masks) + off);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
    } else {
        const float4 x = *reinterpret_cast<const float4*>(masks + off);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    }
}

// nt: the tile count srt_ov_row clamps the primary tile with (OV only): p.ntiles for a whole call, the track's own in a packed batch (where p.ntiles is the packed
// total, the stem stride)
// TRK: the row belongs to a track of a packed batch - mo / eo: its first mask element (halves for M16) / its first float of a stem's table
// SEAM (with OV, float masks): the rows are a piece's of a longer stream - on its first O rows (srt_ov_seam) `a` comes from the mask seam carry, as in the inverse kernels
template <int NS, bool M16, bool RATIO, bool OV, bool TRK = false, bool SEAM = false>
__device__ __forceinline__ void srt_mask_ext_row(const SrtMaskExtParams& p, int O, int f, int c, int lane, int nt, size_t mo = 0, size_t eo = 0, const float* __restrict__ seam = nullptr)
{
    static_assert(!SEAM || (OV && !TRK && !M16), "the seam carry belongs to one signal's overlapped tiles and holds floats");
    constexpr int V = M16 ? 8 : 4;                      // mask values per 16-byte load
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf;
    int tile = f / p.T, t = f % p.T;
    OvRow ov = { 0, 0, false, 0.0f };
    if constexpr (OV) { ov = srt_ov_row(f, p.T, O, nt); tile = ov.j1; t = ov.k; }
    size_t bo = ((size_t)tile * 2 + c) * tf + (size_t)t * p.F;                           // stem 0's row in the primary tile
    if constexpr (TRK) bo += mo;
    const size_t ao = ov.two ? bo - 2 * tf + (size_t)(p.T - O) * p.F : bo;              // ... and row k + S of the previous tile
    const bool sm = SEAM && srt_ov_seam(ov, O, seam);                                   // ... or row k of the carry: its base, first element and stem stride
    const float* __restrict__ const am = sm ? seam : p.masks;
    const size_t so = sm ? ((size_t)c * O + ov.k) * p.F : ao, as = sm ? 2 * (size_t)O * p.F : sstride;
    float sum[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) sum[s] = 0.0f;
    auto walk = [&](auto two_c) {                        // (the row is inside an overlap or not: decided once per row, outside the load loop)
        constexpr bool TWO = decltype(two_c)::value;
        for (int k = lane * V; k < p.F; k += 64 * V) {
            float b[NS][V], a[NS][V];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                srt_mask_load16<M16>(p.masks, (size_t)s * sstride + bo + k, b[s]);
                if constexpr (TWO && SEAM) srt_mask_load16<M16>(am, (size_t)s * as + so + k, a[s]);
                else if constexpr (TWO) srt_mask_load16<M16>(p.masks, (size_t)s * sstride + ao + k, a[s]);
                else {
#pragma unroll
                    for (int j = 0; j < V; ++j) a[s][j] = b[s][j];
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    float g;
                    if constexpr (RATIO && OV) g = srt_ratio_of_ov(&b[0][j], &a[0][j], TWO, ov.w, V, NS, s, 0, true);
                    else if constexpr (RATIO) g = srt_ratio_of(b[s][j], &b[0][j], V, NS, s, 0);
                    else if constexpr (TWO) g = srt_blend(a[s][j], b[s][j], ov.w);
                    else g = b[s][j];
                    sum[s] = sum[s] + g;
                }
            }
        }
    };
    if (OV && (ov.two || sm)) walk(std::true_type{}); else walk(std::false_type{});
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float v = sum[s];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
        if (lane == 0) p.ext[(size_t)s * p.ext_stem + (TRK ? eo : 0) + (size_t)f * 2 + c] = v / (float)p.F;
    }
}

template <bool M16, bool RATIO, bool OV>
__global__ void __launch_bounds__(256) srt_mask_ext_kernel(const SrtMaskExtParams p, int O)
{
    const int wave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= p.rows * 2) return;                      // (wave-uniform; the kernel has no barrier)
    const int f = wave >> 1, c = wave & 1;
    switch (p.nstems) {
    case 1: srt_mask_ext_row<1, M16, RATIO, OV>(p, O, f, c, lane, p.ntiles); break;
    case 2: srt_mask_ext_row<2, M16, RATIO, OV>(p, O, f, c, lane, p.ntiles); break;
    case 3: srt_mask_ext_row<3, M16, RATIO, OV>(p, O, f, c, lane, p.ntiles); break;
    case 4: srt_mask_ext_row<4, M16, RATIO, OV>(p, O, f, c, lane, p.ntiles); break;
    case 5: srt_mask_ext_row<5, M16, RATIO, OV>(p, O, f, c, lane, p.ntiles); break;
    case 6: srt_mask_ext_row<6, M16, RATIO, OV>(p, O, f, c, lane, p.ntiles); break;
    case 7: srt_mask_ext_row<7, M16, RATIO, OV>(p, O, f, c, lane, p.ntiles); break;
    default: srt_mask_ext_row<8, M16, RATIO, OV>(p, O, f, c, lane, p.ntiles); break;
    }
}
// the table of a piece of a longer stream (srtSeparateHostStreamOverlap): the OV form with the SEAM rows
template <bool RATIO>
__global__ void __launch_bounds__(256) srt_mask_ext_seam_kernel(const SrtMaskExtParams p, int O, const float* __restrict__ seam)
{
    const int wave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= p.rows * 2) return;
    const int f = wave >> 1, c = wave & 1;
    switch (p.nstems) {
    case 1: srt_mask_ext_row<1, false, RATIO, true, false, true>(p, O, f, c, lane, p.ntiles, 0, 0, seam); break;
    case 2: srt_mask_ext_row<2, false, RATIO, true, false, true>(p, O, f, c, lane, p.ntiles, 0, 0, seam); break;
    case 3: srt_mask_ext_row<3, false, RATIO, true, false, true>(p, O, f, c, lane, p.ntiles, 0, 0, seam); break;
    case 4: srt_mask_ext_row<4, false, RATIO, true, false, true>(p, O, f, c, lane, p.ntiles, 0, 0, seam); break;
    case 5: srt_mask_ext_row<5, false, RATIO, true, false, true>(p, O, f, c, lane, p.ntiles, 0, 0, seam); break;
    case 6: srt_mask_ext_row<6, false, RATIO, true, false, true>(p, O, f, c, lane, p.ntiles, 0, 0, seam); break;
    case 7: srt_mask_ext_row<7, false, RATIO, true, false, true>(p, O, f, c, lane, p.ntiles, 0, 0, seam); break;
    default: srt_mask_ext_row<8, false, RATIO, true, false, true>(p, O, f, c, lane, p.ntiles, 0, 0, seam); break;
    }
}
#pragma clang fp contract(fast)

// the form follows the inverse launchers' gates: ratio when p.ratio && p.nstems > 1, halves never with the ratio, the overlap only with O > 0
int srt_launch_mask_ext(const SrtMaskExtParams& p, hipStream_t s, int overlap, const float* seam)
{
    if (p.rows <= 0) return 0;
    static_assert(SRT_MAX_STEMS == 8, "srt_mask_ext_kernel dispatches on 1..8 stems");
    if (!p.masks || !p.ext || p.nstems < 1 || p.nstems > SRT_MAX_STEMS || p.F < 64 || p.F % 64 || p.ext_stem < (size_t)p.rows * 2) return -1;
    if (((uintptr_t)p.masks & 15) != 0) return -1;      // 16-byte loads
    if (overlap < 0 || (overlap > 0 && (overlap > p.T / 2 || p.ntiles < 1 || (size_t)(p.ntiles - 1) * (p.T - overlap) + p.T < (size_t)p.rows))) return -1;
    if (overlap == 0 && (size_t)p.ntiles * p.T < (size_t)p.rows) return -1;
    const bool ratio = p.ratio && p.nstems > 1;
    if (p.masks16 && (ratio || p.F > 1024)) return -1;
    const dim3 grid((p.rows * 2 + 3) / 4), block(256);
    if (seam) {                                          // a piece of a longer stream: 16-byte loads from the carry too
        if (overlap <= 0 || p.masks16 || ((uintptr_t)seam & 15) != 0) return -1;
        if (ratio) SRT_LAUNCH((srt_mask_ext_seam_kernel<true>), grid, block, 0, s, p, overlap, seam);
        else SRT_LAUNCH((srt_mask_ext_seam_kernel<false>), grid, block, 0, s, p, overlap, seam);
        return srt_launch_status();
    }
    if (overlap > 0) {
        if (ratio) SRT_LAUNCH((srt_mask_ext_kernel<false, true, true>), grid, block, 0, s, p, overlap);
        else if (p.masks16) SRT_LAUNCH((srt_mask_ext_kernel<true, false, true>), grid, block, 0, s, p, overlap);
        else SRT_LAUNCH((srt_mask_ext_kernel<false, false, true>), grid, block, 0, s, p, overlap);
    } else if (ratio) SRT_LAUNCH((srt_mask_ext_kernel<false, true, false>), grid, block, 0, s, p, 0);
    else if (p.masks16) SRT_LAUNCH((srt_mask_ext_kernel<true, false, false>), grid, block, 0, s, p, 0);
    else SRT_LAUNCH((srt_mask_ext_kernel<false, false, false>), grid, block, 0, s, p, 0);
    return srt_launch_status();
}

// ------------------------------------------------------------------------------------------- packed batch of tracks (srtSeparateBatch)
// K independent tracks share one launch of each transform.  Track k owns the packed tiles [tile0, tile0 + ntiles) of the engine's buffers (spectrum rows from
// tile0 * T); a run of workgroups belongs to one track (the table's wg_stft / wg_istft: prefix sums of the per-track workgroup counts), and each workgroup runs
// the single-signal kernels' body on its track's view - the same frames, the same arithmetic, the same accumulation order per output sample (the inverse starts
// every run with the 3-frame warm-up from zero, so its bits do not depend on the run length G either).

// the track of workgroup (or run) `wg`: the last k with first(k) <= wg.  wg is workgroup-uniform, so every probe is a uniform (scalar) load.
template <bool ISTFT>
__device__ __forceinline__ int srt_batch_track(const SrtBatchTrack* __restrict__ t, int ntracks, int wg)
{
    int lo = 0, hi = ntracks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((ISTFT ? t[mid].wg_istft : t[mid].wg_stft) <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// p: the packed buffers (spec, spec_ch_stride, mag: never null here), T, F, tables; the PCM and frame counts come from the table
__global__ void __launch_bounds__(256, 3) srt_stft_batch_kernel(const SrtStftParams p, const SrtBatchTrack* __restrict__ tracks, int ntracks, int fpb)
{
    __shared__ cf s_mem[FFT_SMEM_F2 + FFT_MIR_F2 + FFT_TWB_F2];
    const SrtBatchTrack tk = tracks[srt_batch_track<false>(tracks, ntracks, blockIdx.x)];
    const int blk = blockIdx.x - tk.wg_stft;
    float* mag = p.mag + (size_t)tk.tile0 * 2 * p.T * p.F;
    const StftView w = { tk.L, tk.R, tk.n, tk.frames, tk.rows, p.spec + (size_t)tk.tile0 * p.T * SRT_SPEC_LD, mag };
    stft_run(p, w, blk, fpb, s_mem);
    // Magnitude rows from the track's last row to its tile boundary are zero (what srtStftEx's memset leaves there: the network reads whole tiles).  They are
    // shared out over the track's workgroups, after their transforms (a store queued ahead of the frame loop would hold up its first load wait).
    const int nwg = (tk.rows + fpb - 1) / fpb, pad = tk.ntiles * p.T - tk.rows;
    const int fb = tk.rows + (int)((long)(blk + 1) * pad / nwg);
    for (int f = tk.rows + (int)((long)blk * pad / nwg); f < fb; ++f) {
        const int tile = f / p.T, t = f % p.T;
        float* magL = mag + ((size_t)(tile * 2 + 0) * p.T + t) * p.F;
        float* magR = magL + (size_t)p.T * p.F;
        for (int k = threadIdx.x; k < p.F; k += 256) { magL[k] = 0.f; magR[k] = 0.f; }
    }
}

// OLA3: the three-per-CU form (F <= 1024), otherwise the two-per-CU table-window form; RATIO / M16 as srt_istft_ola3_kernel.  p.ntiles = the packed tile count
// (the stem stride of the masks), p.spec / p.masks: the packed buffers; frames, output and its length per track.
template <bool OLA3, bool RATIO, bool M16>
__global__ void __launch_bounds__(256, OLA3 && !RATIO ? 3 : 2) srt_istft_batch_kernel(const SrtIstftParams p, const SrtBatchTrack* __restrict__ tracks, int ntracks, int G)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;       // stem fastest, as in the single-signal kernels
    __shared__ cf s_mem[OLA3 ? ISTFT_OLA3_LDS_F2 : ISTFT_OLA_LDS_F2];
    const SrtBatchTrack tk = tracks[srt_batch_track<true>(tracks, ntracks, run)];
    const size_t mo = (size_t)tk.tile0 * 2 * p.T * p.F;                     // the track's first mask element (halves for M16)
    IstftView w;
    w.spec = p.spec + (size_t)tk.tile0 * p.T * SRT_SPEC_LD;
    w.masks = !p.masks ? nullptr : M16 ? reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(p.masks) + mo) : p.masks + mo;
    w.out = tk.out; w.out_len = tk.out_len; w.frames = tk.rows;
    w.ext = nullptr;
    if constexpr (OLA3) istft_ola3_run<4, RATIO, M16>(p, w, stem, run - tk.wg_istft, G, s_mem);
    else istft_ola_run<RATIO>(p, w, stem, run - tk.wg_istft, G, s_mem);
}
// the same with the average mask extension: the table is indexed by packed row, so the track's rows start at tile0 * T
template <bool OLA3, bool RATIO, bool M16>
__global__ void __launch_bounds__(256, OLA3 && !RATIO ? 3 : 2) srt_istft_batch_ext_kernel(const SrtIstftParams p, const SrtBatchTrack* __restrict__ tracks, int ntracks, int G)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[OLA3 ? ISTFT_OLA3_LDS_F2 : ISTFT_OLA_LDS_F2];
    const SrtBatchTrack tk = tracks[srt_batch_track<true>(tracks, ntracks, run)];
    const size_t mo = (size_t)tk.tile0 * 2 * p.T * p.F;
    IstftView w;
    w.spec = p.spec + (size_t)tk.tile0 * p.T * SRT_SPEC_LD;
    w.masks = M16 ? reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(p.masks) + mo) : p.masks + mo;      // (the launcher checks that masks are given)
    w.out = tk.out; w.out_len = tk.out_len; w.frames = tk.rows;
    w.ext = p.ext + (size_t)tk.tile0 * p.T * 2;
    if constexpr (OLA3) istft_ola3_run<4, RATIO, M16, false, true>(p, w, stem, run - tk.wg_istft, G, s_mem);
    else istft_ola_run<RATIO, false, true>(p, w, stem, run - tk.wg_istft, G, s_mem);
}

// per-stem spectra instead of masks (srtSeparateBatchWiener: the filter wrote one spectrum per stem over the packed rows): stem s of a track reads
// p.spec + s * stem_stride at the track's packed rows, all-ones in band and p.oob[s] above F - the single-signal filter path's mask-free, single-stem launches
// (srt_istft_ola3_kernel<4> / srt_istft_ola_kernel<false>) for every (track, stem) at once.  The stride is an argument of its own: SrtIstftParams stays as it is.
template <bool OLA3>
__global__ void __launch_bounds__(256, OLA3 ? 3 : 2) srt_istft_batch_spec_kernel(const SrtIstftParams p, const SrtBatchTrack* __restrict__ tracks, int ntracks, int G, size_t stem_stride)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[OLA3 ? ISTFT_OLA3_LDS_F2 : ISTFT_OLA_LDS_F2];
    const SrtBatchTrack tk = tracks[srt_batch_track<true>(tracks, ntracks, run)];
    IstftView w;
    w.spec = p.spec + (size_t)stem * stem_stride + (size_t)tk.tile0 * p.T * SRT_SPEC_LD;
    w.masks = nullptr;
    w.out = tk.out; w.out_len = tk.out_len; w.frames = tk.rows;
    w.ext = nullptr;
    if constexpr (OLA3) istft_ola3_run<4, false, false>(p, w, stem, run - tk.wg_istft, G, s_mem);
    else istft_ola_run<false>(p, w, stem, run - tk.wg_istft, G, s_mem);
}

// ---- overlapped tiles inside a packed batch (srtSeparateBatchOverlap): track k owns the packed tiles [tile0, tile0 + ntiles) with ntiles =
// srtOverlapTiles(rows, T, O), in the overlapped layout of section 13 INSIDE those tiles; its spectrum stays at packed rows from tile0 * T (rows <= ntiles * T).
// Each workgroup runs the single-signal overlap bodies on its track's view with the track's own tile count, so a row's second magnitude copy and a frame's
// blend partner are always a tile of the same track (srt_ov_row: only when j1 > 0 inside the track).

// stft_run<true> per track.  The pad: rows of a tile past the track's last row exist only in its last tile J = ntiles - 1 (tile J - 1 ends at row J S + O <= rows);
// its slots (J, t), t in [rows - J S, T), are zeroed and shared out over the track's workgroups after their transforms, as in srt_stft_batch_kernel.
__global__ void __launch_bounds__(256, 3) srt_stft_batch_ov_kernel(const SrtStftParams p, const SrtBatchTrack* __restrict__ tracks, int ntracks, int fpb, int O)
{
    __shared__ cf s_mem[FFT_SMEM_F2 + FFT_MIR_F2 + FFT_TWB_F2];
    const SrtBatchTrack tk = tracks[srt_batch_track<false>(tracks, ntracks, blockIdx.x)];
    const int blk = blockIdx.x - tk.wg_stft;
    float* mag = p.mag + (size_t)tk.tile0 * 2 * p.T * p.F;
    const StftView w = { tk.L, tk.R, tk.n, tk.frames, tk.rows, p.spec + (size_t)tk.tile0 * p.T * SRT_SPEC_LD, mag };
    stft_run<true>(p, w, blk, fpb, s_mem, O, tk.ntiles);
    const int J = tk.ntiles - 1, t0 = tk.rows - J * (p.T - O);              // 1 <= t0 <= T: the last tile's first pad slot
    const int nwg = (tk.rows + fpb - 1) / fpb, pad = p.T - t0;
    float* magL = mag + (size_t)J * 2 * p.T * p.F;
    float* magR = magL + (size_t)p.T * p.F;
    const int tb = t0 + (int)((long)(blk + 1) * pad / nwg);
    for (int t = t0 + (int)((long)blk * pad / nwg); t < tb; ++t)
        for (int k = threadIdx.x; k < p.F; k += 256) { magL[(size_t)t * p.F + k] = 0.f; magR[(size_t)t * p.F + k] = 0.f; }
}

// srt_istft_batch_kernel with the overlap bodies: srt_ov_row's tile count is the track's (the bodies' TRK form), p.ntiles stays the packed count (the stem stride).
// EXT: the average mask extension (the table is indexed by packed row: srt_mask_ext_batch_kernel) - a template argument here, not a second kernel name
template <bool OLA3, bool RATIO, bool M16, bool EXT>
__global__ void __launch_bounds__(256, OLA3 && !RATIO ? 3 : 2) srt_istft_batch_ov_kernel(const SrtIstftParams p, const SrtBatchTrack* __restrict__ tracks, int ntracks, int G, int O)
{
    const int pos = srt_xcd_order(gridDim.x), stem = pos % p.nstems, run = pos / p.nstems;
    __shared__ cf s_mem[OLA3 ? ISTFT_OLA3_LDS_F2 : ISTFT_OLA_LDS_F2];
    const SrtBatchTrack tk = tracks[srt_batch_track<true>(tracks, ntracks, run)];
    const size_t mo = (size_t)tk.tile0 * 2 * p.T * p.F;
    IstftView w;
    w.spec = p.spec + (size_t)tk.tile0 * p.T * SRT_SPEC_LD;
    w.masks = M16 ? reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(p.masks) + mo) : p.masks + mo;      // (the launcher checks that masks are given)
    w.out = tk.out; w.out_len = tk.out_len; w.frames = tk.rows;
    w.ext = EXT ? p.ext + (size_t)tk.tile0 * p.T * 2 : nullptr;
    if constexpr (OLA3) istft_ola3_run<4, RATIO, M16, true, EXT, false, true>(p, w, stem, run - tk.wg_istft, G, s_mem, O, tk.ntiles);
    else istft_ola_run<RATIO, true, EXT, false, true>(p, w, stem, run - tk.wg_istft, G, s_mem, O, tk.ntiles);
}

// Stem remix per track (srtSeparateBatchMix): the MIX bodies on a track's view.  The workgroup index is the OUTPUT m, fastest in the XCD order, so
// the outputs of a run share its spectrum rows and every stem's mask rows in L2 (srt_istft_ola3_mix_kernel).  Track k's matrix is row k of the device table
// `gains` [ntracks][n_out][nstems + 1], uploaded beside the track table: the bodies read row m of it entry by entry (SrtMixTab; k and m are workgroup-uniform, so
// these are scalar loads), nothing of p.mix.  OV = false: the back-to-back view of srt_istft_batch_kernel (O and the track's tile count are unused); EXT as above.
template <bool OLA3, bool OV, bool EXT>
__global__ void __launch_bounds__(256, 2) srt_istft_batch_bus_kernel(const SrtIstftParams p, const SrtBatchTrack* __restrict__ tracks, int ntracks, int G, int O, const float* __restrict__ gains)
{
    const int pos = srt_xcd_order(gridDim.x), m = pos % p.n_out, run = pos / p.n_out;
    __shared__ cf s_mem[OLA3 ? ISTFT_OLA3_LDS_F2 : ISTFT_OLA_LDS_F2];
    const int k = srt_batch_track<true>(tracks, ntracks, run);
    const SrtBatchTrack tk = tracks[k];
    IstftView w;
    w.spec = p.spec + (size_t)tk.tile0 * p.T * SRT_SPEC_LD;
    w.masks = p.masks + (size_t)tk.tile0 * 2 * p.T * p.F;                   // (the launcher checks that masks are given: floats)
    w.out = tk.out; w.out_len = tk.out_len; w.frames = tk.rows;
    w.ext = EXT ? p.ext + (size_t)tk.tile0 * p.T * 2 : nullptr;
    w.gain = gains + (size_t)k * p.n_out * (p.nstems + 1);
    if constexpr (OLA3) istft_ola3_run<4, false, false, OV, EXT, true, true, true>(p, w, m, run - tk.wg_istft, G, s_mem, O, tk.ntiles);
    else istft_ola_run<false, OV, EXT, true, true, true>(p, w, m, run - tk.wg_istft, G, s_mem, O, tk.ntiles);
}

// The gain table of the average mask extension for such a batch: one wave per (packed row, channel), as srt_mask_ext_kernel.  The row's track is the last one
// with tile0 * T <= row (the wave index is made uniform first, so every probe of the table is a scalar load); the row is mapped with the TRACK's tile count, its
// blend partner is read inside the track's tiles, and ext is written at the packed row.  Rows past the track's own (the rest of its last tile) are skipped.
// Per row the arithmetic and the order of the additions are srt_mask_ext_row's: a track's table is the single call's, bit for bit.
#pragma clang fp contract(off)
template <bool M16, bool RATIO>
__global__ void __launch_bounds__(256) srt_mask_ext_batch_kernel(const SrtMaskExtParams p, const SrtBatchTrack* __restrict__ tracks, int ntracks, int O)
{
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (wave >= p.rows * 2) return;                      // (wave-uniform; the kernel has no barrier)
    const int row = wave >> 1, c = wave & 1;
    int lo = 0, hi = ntracks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tracks[mid].tile0 * p.T <= row) lo = mid; else hi = mid - 1;
    }
    const int tile0 = tracks[lo].tile0, rows = tracks[lo].rows, nt = tracks[lo].ntiles;
    const int f = row - tile0 * p.T;
    if (f >= rows) return;
    const size_t mo = (size_t)tile0 * 2 * p.T * p.F, eo = (size_t)tile0 * p.T * 2;      // the track's first mask element (halves for M16) and table entry
    switch (p.nstems) {
    case 1: srt_mask_ext_row<1, M16, RATIO, true, true>(p, O, f, c, lane, nt, mo, eo); break;
    case 2: srt_mask_ext_row<2, M16, RATIO, true, true>(p, O, f, c, lane, nt, mo, eo); break;
    case 3: srt_mask_ext_row<3, M16, RATIO, true, true>(p, O, f, c, lane, nt, mo, eo); break;
    case 4: srt_mask_ext_row<4, M16, RATIO, true, true>(p, O, f, c, lane, nt, mo, eo); break;
    case 5: srt_mask_ext_row<5, M16, RATIO, true, true>(p, O, f, c, lane, nt, mo, eo); break;
    case 6: srt_mask_ext_row<6, M16, RATIO, true, true>(p, O, f, c, lane, nt, mo, eo); break;
    case 7: srt_mask_ext_row<7, M16, RATIO, true, true>(p, O, f, c, lane, nt, mo, eo); break;
    default: srt_mask_ext_row<8, M16, RATIO, true, true>(p, O, f, c, lane, nt, mo, eo); break;
    }
}
#pragma clang fp contract(fast)

// smallest q >= q0 with count(q) <= limit (count falls as q grows); q0 when even qmax does not get there
template <class C>
static int srt_batch_step(int q0, int qmax, long limit, C&& count)
{
    if (count(q0) <= limit || qmax <= q0 || count(qmax) > limit) return q0;
    int lo = q0, hi = qmax;                                                 // count(lo) > limit >= count(hi)
    while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; if (count(mid) <= limit) hi = mid; else lo = mid; }
    return hi;
}

// The two grids of a batch, with the single-signal launchers' rules applied to the totals: frames per STFT workgroup from the row total (srt_launch_stft; the
// magnitude rows that pad each track to whole tiles are zeroed by the track's workgroups on the side), the inverse's run length from the total segment count
// (srt_launch_istft).  Rounding per track can add up to one workgroup per track, so
// the step is raised until the grid again fits the rounds the totals call for.  Fills every track's wg_stft / wg_istft.
int srt_batch_geometry(SrtBatchTrack* t, int ntracks, int T, int F, int nstems, SrtBatchGrid* g)
{
    if (ntracks < 1 || nstems < 1) return -1;
    long rows = 0, nseg = 0;
    int max_rows = 1, max_seg = 1;
    for (int k = 0; k < ntracks; ++k) {
        rows += t[k].rows; nseg += t[k].rows + 3;
        max_rows = max(max_rows, t[k].rows); max_seg = max(max_seg, t[k].rows + 3);
    }
    auto stft_blocks = [&](int q) { long b = 0; for (int k = 0; k < ntracks; ++k) b += (t[k].rows + q - 1) / q; return b; };
    int fpb = rows >= 4096 ? STFT_FPB : (rows >= 1024 ? 2 : 1);
    if (rows >= 4096) {
        constexpr int cap = 24;
        const long slots = 768, rounds = (rows + slots * cap - 1) / (slots * cap);
        fpb = (int)((rows + slots * rounds - 1) / (slots * rounds));
        fpb = srt_batch_step(fpb, max_rows, slots * rounds, stft_blocks);
    }
    const int target = F > 1024 ? 1024 : 768;
    const int max_runs = target / nstems > 0 ? target / nstems : 1;
    auto runs = [&](int q) { long r = 0; for (int k = 0; k < ntracks; ++k) r += (t[k].rows + 3 + q - 1) / q; return r; };
    int G = (int)((nseg + max_runs - 1) / max_runs);
    const int gmin = nseg * nstems >= 4096 ? 13 : 5;
    if (G < gmin) G = gmin;
    G = srt_batch_step(G, max_seg, max_runs, runs);
    long wb = 0, wr = 0;
    for (int k = 0; k < ntracks; ++k) {
        t[k].wg_stft = (int)wb; t[k].wg_istft = (int)wr;
        wb += (t[k].rows + fpb - 1) / fpb;
        wr += (t[k].rows + 3 + G - 1) / G;
    }
    if (wb > (1l << 30) || wr * nstems > (1l << 30)) return -1;
    g->fpb = fpb; g->stft_blocks = (int)wb; g->G = G; g->istft_runs = (int)wr;
    return 0;
}

// overlap > 0: every track's magnitudes in the overlapped layout inside its own tiles (the table's ntiles = srtOverlapTiles(rows, T, overlap), checked by the caller, which
// filled the table); 0: the back-to-back kernels as they always were
int srt_launch_stft_batch(const SrtStftParams& p, const SrtBatchTrack* d_tracks, int ntracks, const SrtBatchGrid& g, hipStream_t s, int overlap)
{
    if (!p.mag || g.stft_blocks <= 0 || overlap < 0 || overlap > p.T / 2) return -1;
    if (overlap > 0) SRT_LAUNCH(srt_stft_batch_ov_kernel, dim3(g.stft_blocks), dim3(256), 0, s, p, d_tracks, ntracks, g.fpb, overlap);
    else SRT_LAUNCH(srt_stft_batch_kernel, dim3(g.stft_blocks), dim3(256), 0, s, p, d_tracks, ntracks, g.fpb);
    return srt_launch_status();
}

// the same form per geometry as srt_launch_istft; overlap as srt_launch_stft_batch (the masks are required then: there is nothing to blend without them)
int srt_launch_istft_batch(const SrtIstftParams& p, const SrtBatchTrack* d_tracks, int ntracks, const SrtBatchGrid& g, hipStream_t s, int overlap)
{
    if (g.istft_runs <= 0 || overlap < 0 || overlap > p.T / 2 || (overlap > 0 && !p.masks)) return -1;
    if (p.masks16 && (!p.masks || p.F > 1024 || (p.ratio && p.nstems > 1))) return -1;
    const dim3 grid(g.istft_runs * p.nstems);
    if (overlap > 0) {                                   // the overlap instantiations (the forms below keep their code)
        const int O = overlap;
        const bool ratio = p.ratio && p.nstems > 1;
        if (p.ext) {
            if (p.ext_stem < (size_t)p.frames * 2) return -1;
            if (ratio) {
                if (p.F > 1024) SRT_LAUNCH((srt_istft_batch_ov_kernel<false, true, false, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
                else SRT_LAUNCH((srt_istft_batch_ov_kernel<true, true, false, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
            } else if (p.F > 1024) SRT_LAUNCH((srt_istft_batch_ov_kernel<false, false, false, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
            else if (p.masks16) SRT_LAUNCH((srt_istft_batch_ov_kernel<true, false, true, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
            else SRT_LAUNCH((srt_istft_batch_ov_kernel<true, false, false, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
        } else if (ratio) {
            if (p.F > 1024) SRT_LAUNCH((srt_istft_batch_ov_kernel<false, true, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
            else SRT_LAUNCH((srt_istft_batch_ov_kernel<true, true, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
        } else if (p.F > 1024) SRT_LAUNCH((srt_istft_batch_ov_kernel<false, false, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
        else if (p.masks16) SRT_LAUNCH((srt_istft_batch_ov_kernel<true, false, true, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
        else SRT_LAUNCH((srt_istft_batch_ov_kernel<true, false, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O);
        return srt_launch_status();
    }
    if (p.ext) {
        if (!p.masks || p.ext_stem < (size_t)p.frames * 2) return -1;
        if (p.ratio && p.nstems > 1) {
            if (p.F > 1024) SRT_LAUNCH((srt_istft_batch_ext_kernel<false, true, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
            else SRT_LAUNCH((srt_istft_batch_ext_kernel<true, true, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
        } else if (p.F > 1024) SRT_LAUNCH((srt_istft_batch_ext_kernel<false, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
        else if (p.masks16) SRT_LAUNCH((srt_istft_batch_ext_kernel<true, false, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
        else SRT_LAUNCH((srt_istft_batch_ext_kernel<true, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
        return srt_launch_status();
    }
    if (p.ratio && p.masks && p.nstems > 1) {
        if (p.F > 1024) SRT_LAUNCH((srt_istft_batch_kernel<false, true, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
        else SRT_LAUNCH((srt_istft_batch_kernel<true, true, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
    } else if (p.F > 1024) SRT_LAUNCH((srt_istft_batch_kernel<false, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
    else if (p.masks16) SRT_LAUNCH((srt_istft_batch_kernel<true, false, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
    else SRT_LAUNCH((srt_istft_batch_kernel<true, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G);
    return srt_launch_status();
}

// the stem remix per track: p.n_out outputs per track (g from srt_batch_geometry with n_out workgroup columns), track k's matrix at d_gains + k * n_out * (nstems + 1);
// float masks are required, p.mix is not read.  The form follows F, the overlap and p.ext; ratio is a run-time flag of the MIX bodies
int srt_launch_istft_batch_mix(const SrtIstftParams& p, const SrtBatchTrack* d_tracks, const float* d_gains, int ntracks, const SrtBatchGrid& g, hipStream_t s, int overlap)
{
    if (g.istft_runs <= 0 || overlap < 0 || overlap > p.T / 2 || !p.masks || p.masks16 || !d_gains) return -1;
    if (p.n_out < 1 || p.n_out > SRT_MAX_STEMS || p.nstems < 1 || p.nstems > SRT_MAX_STEMS) return -1;
    if (p.ext && p.ext_stem < (size_t)p.frames * 2) return -1;
    const dim3 grid(g.istft_runs * p.n_out);
    const int O = overlap;
    if (p.F > 1024) {
        if (O > 0 && p.ext) SRT_LAUNCH((srt_istft_batch_bus_kernel<false, true, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O, d_gains);
        else if (O > 0) SRT_LAUNCH((srt_istft_batch_bus_kernel<false, true, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O, d_gains);
        else if (p.ext) SRT_LAUNCH((srt_istft_batch_bus_kernel<false, false, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, 0, d_gains);
        else SRT_LAUNCH((srt_istft_batch_bus_kernel<false, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, 0, d_gains);
    } else if (O > 0 && p.ext) SRT_LAUNCH((srt_istft_batch_bus_kernel<true, true, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O, d_gains);
    else if (O > 0) SRT_LAUNCH((srt_istft_batch_bus_kernel<true, true, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, O, d_gains);
    else if (p.ext) SRT_LAUNCH((srt_istft_batch_bus_kernel<true, false, true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, 0, d_gains);
    else SRT_LAUNCH((srt_istft_batch_bus_kernel<true, false, false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, 0, d_gains);
    return srt_launch_status();
}

// srt_launch_mask_ext for a packed batch with overlapped tiles: p on the packed buffers (ntiles = the packed tile count, rows = every packed row = ntiles * T),
// the per-track rows and tile counts from the table; the gates are srt_launch_mask_ext's.  (overlap = 0 needs no table: a packed row maps to its packed tile.)
int srt_launch_mask_ext_batch(const SrtMaskExtParams& p, const SrtBatchTrack* d_tracks, int ntracks, hipStream_t s, int overlap)
{
    if (overlap == 0) return srt_launch_mask_ext(p, s, 0);
    if (p.rows <= 0) return 0;
    if (!p.masks || !p.ext || !d_tracks || ntracks < 1 || p.nstems < 1 || p.nstems > SRT_MAX_STEMS || p.F < 64 || p.F % 64 || p.ext_stem < (size_t)p.rows * 2) return -1;
    if (((uintptr_t)p.masks & 15) != 0) return -1;      // 16-byte loads (a track's first tile keeps the alignment: F % 64 == 0)
    if (overlap < 0 || overlap > p.T / 2 || (size_t)p.ntiles * p.T < (size_t)p.rows) return -1;
    const bool ratio = p.ratio && p.nstems > 1;
    if (p.masks16 && (ratio || p.F > 1024)) return -1;
    const dim3 grid((p.rows * 2 + 3) / 4), block(256);
    if (ratio) SRT_LAUNCH((srt_mask_ext_batch_kernel<false, true>), grid, block, 0, s, p, d_tracks, ntracks, overlap);
    else if (p.masks16) SRT_LAUNCH((srt_mask_ext_batch_kernel<true, false>), grid, block, 0, s, p, d_tracks, ntracks, overlap);
    else SRT_LAUNCH((srt_mask_ext_batch_kernel<false, false>), grid, block, 0, s, p, d_tracks, ntracks, overlap);
    return srt_launch_status();
}

// the same two forms per geometry for per-stem spectra without masks (p.masks, p.ext and p.ratio are not used)
int srt_launch_istft_batch_spec(const SrtIstftParams& p, size_t stem_stride, const SrtBatchTrack* d_tracks, int ntracks, const SrtBatchGrid& g, hipStream_t s)
{
    if (g.istft_runs <= 0 || p.masks || p.masks16 || p.ext || stem_stride < 2 * p.spec_ch_stride) return -1;
    const dim3 grid(g.istft_runs * p.nstems);
    if (p.F > 1024) SRT_LAUNCH((srt_istft_batch_spec_kernel<false>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, stem_stride);
    else SRT_LAUNCH((srt_istft_batch_spec_kernel<true>), grid, dim3(256), 0, s, p, d_tracks, ntracks, g.G, stem_stride);
    return srt_launch_status();
}

// ------------------------------------------------------------------------------------------- residual chain / ratio mask
// Complex-domain residual of the three-output CLI flow (main.c:845-866): the first network's masked spectrum is subtracted
// from the original, and the second network sees the magnitude of what is left.  Same two roundings as the reference
// (product, then difference: no fused multiply-add).  One workgroup = one spectrogram row of one channel.  HBM bound:
// 16.4 KB read + 16.4 KB written + 2 x 4 F bytes per row.
__global__ void __launch_bounds__(256) srt_residual_kernel(const SrtResidualParams p)
{
    const int row = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
    const int tile = row / p.T, t = row % p.T;
    const cf* src = reinterpret_cast<const cf*>(p.spec) + (size_t)ch * p.spec_ch_stride + (size_t)row * SRT_SPEC_LD;
    cf* dst = reinterpret_cast<cf*>(p.res) + (size_t)ch * p.spec_ch_stride + (size_t)row * SRT_SPEC_LD;
    const size_t mo = ((size_t)(tile * 2 + ch) * p.T + t) * p.F;
    const float* m = p.mask + mo;
    float* mag = p.mag ? p.mag + mo : nullptr;
    for (int k = tid; k < SRT_SPEC_LD; k += 256) {
        cf r = f2(0.f, 0.f);
        if (k <= 2048) {
            const cf v = src[k];
            const float g = k < p.F ? m[k] : p.oob;
            r.x = __fsub_rn(v.x, __fmul_rn(v.x, g));
            r.y = __fsub_rn(v.y, __fmul_rn(v.y, g));
            if (mag && k < p.F) mag[k] = hypotf(r.x, r.y) * 4096.0f;
        }
        dst[k] = r;
    }
}

int srt_launch_residual(const SrtResidualParams& p, hipStream_t s)
{
    if (p.rows <= 0) return 0;
    SRT_LAUNCH(srt_residual_kernel, dim3(p.rows, 2), dim3(256), 0, s, p);
    return srt_launch_status();
}

// out = a - b on samples [lo, hi) of two planes of nb floats (a: two separate planes of na valid samples, zero beyond)
__global__ void __launch_bounds__(256) srt_time_residual_kernel(const float* aL, const float* aR, size_t na, const float* b, size_t nb, float* out, size_t lo, size_t hi)
{
    const size_t i = lo + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= hi) return;
    const float* a = blockIdx.y ? aR : aL;
    const size_t o = (size_t)blockIdx.y * nb + i;
    out[o] = (i < na ? a[i] : 0.0f) - b[o];
}

int srt_launch_time_residual(const float* aL, const float* aR, size_t na, const float* b, size_t nb, float* out, size_t lo, size_t hi, hipStream_t s)
{
    if (hi > nb) hi = nb;
    if (hi <= lo) return 0;
    SRT_LAUNCH(srt_time_residual_kernel, dim3((unsigned)((hi - lo + 255) / 256), 2), dim3(256), 0, s, aL, aR, na, b, nb, out, lo, hi);
    return srt_launch_status();
}

// Overlap-add across the chunks of a long stream: consecutive chunks share 3072 output samples (three hops of the last
// frames' tails, stftFix.c:570-575).  The previous chunk's tail is added to this chunk's head and this chunk's tail is kept.
__global__ void __launch_bounds__(256) srt_carry_kernel(float* out, size_t plane_len, size_t tail, float* carry, int first, int last)
{
    const int i = blockIdx.x * 256 + threadIdx.x, pl = blockIdx.y;         // i < 3072
    float* o = out + (size_t)pl * plane_len;
    float* c = carry + (size_t)pl * (SRT_FFT - SRT_HOP);
    if (!first) o[i] += c[i];
    if (!last) c[i] = o[tail + i];                                         // tail >= 3072 for every chunk but the last
}

int srt_launch_carry(float* out, size_t plane_len, int nplanes, size_t tail, float* carry, int first, int last, hipStream_t s)
{
    if (first && last) return 0;
    SRT_LAUNCH(srt_carry_kernel, dim3((SRT_FFT - SRT_HOP) / 256, nplanes), dim3(256), 0, s, out, plane_len, tail, carry, first, last);
    return srt_launch_status();
}

// The mask seam carry of overlapped tiles across the pieces of a long stream (srtSeparateHostStreamOverlap): the next piece's forward overwrites
// the mask buffer, and rows [0, O) of its first tile blend with rows [S, T) of this piece's last tile - those O * F floats per (stem, channel), contiguous in the
// tile, are copied out.  Bandwidth-bound: one 16-byte load and store per thread, blockIdx.y = stem * 2 + channel.
__global__ void __launch_bounds__(256) srt_mask_seam_save_kernel(const float4* __restrict__ masks4, float4* __restrict__ seam4, size_t stem4, size_t tf4, size_t row4, unsigned n4)
{
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    const int st = blockIdx.y >> 1, c = blockIdx.y & 1;
    if (i < n4) seam4[(size_t)blockIdx.y * n4 + i] = masks4[(size_t)st * stem4 + (size_t)c * tf4 + row4 + i];
}

int srt_launch_mask_seam_save(const float* masks, int nstems, int ntiles, int T, int F, int overlap, float* seam, hipStream_t s)
{
    if (!masks || !seam || nstems < 1 || ntiles < 1 || overlap < 1 || overlap > T / 2 || F < 4 || F % 4) return -1;
    if ((((uintptr_t)masks | (uintptr_t)seam) & 15) != 0) return -1;
    const size_t tf4 = (size_t)T * F / 4, n4 = (size_t)overlap * F / 4;
    const size_t row4 = (size_t)(ntiles - 1) * 2 * tf4 + (size_t)(T - overlap) * F / 4;                  // row S of the last tile, channel L
    SRT_LAUNCH(srt_mask_seam_save_kernel, dim3((unsigned)((n4 + 255) / 256), nstems * 2), dim3(256), 0, s, (const float4*)masks, (float4*)seam, (size_t)ntiles * 2 * tf4, tf4, row4, (unsigned)n4);
    return srt_launch_status();
}

// Cross-stem ratio mask (what official Spleeter applies and the reference deliberately leaves out, README.MD:82-85):
// every stem's mask is squared and normalised by the sum over stems at the same (tile, channel, frame, bin).
#pragma clang fp contract(off)
__global__ void __launch_bounds__(256) srt_ratio_mask_kernel(float* masks, int nstems, size_t count)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= count) return;                                        // count is a multiple of 4 (F % 64 == 0)
    // every operation individually rounded (plain operators under contract(off), no fused multiply-add): srt_ratio_of, the form folded into the inverse transform's prologue,
    // does the same operations in the same order, and the two must agree bit for bit (tests/test_gpu_parity.py::test_ratio_mask)
    float m[SRT_MAX_STEMS][4];
    float sum[4] = { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
    for (int s = 0; s < SRT_MAX_STEMS; ++s) {
        if (s < nstems) {
            const float4 v = *reinterpret_cast<const float4*>(masks + (size_t)s * count + i);
            const float x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int c = 0; c < 4; ++c) { m[s][c] = x[c] * x[c]; sum[c] = sum[c] + m[s][c]; }
        }
    }
    const float eps = 1e-10f, e1 = eps / (float)nstems;
#pragma unroll
    for (int s = 0; s < SRT_MAX_STEMS; ++s) {
        if (s < nstems) {
            float4 v;
            v.x = (m[s][0] + e1) / (sum[0] + eps); v.y = (m[s][1] + e1) / (sum[1] + eps);
            v.z = (m[s][2] + e1) / (sum[2] + eps); v.w = (m[s][3] + e1) / (sum[3] + eps);
            *reinterpret_cast<float4*>(masks + (size_t)s * count + i) = v;
        }
    }
}

#pragma clang fp contract(fast)
int srt_launch_ratio_mask(float* masks, int nstems, size_t count, hipStream_t s)
{
    if (!count || nstems < 1) return 0;
    SRT_LAUNCH(srt_ratio_mask_kernel, dim3((unsigned)((count / 4 + 255) / 256)), dim3(256), 0, s, masks, nstems, count);
    return srt_launch_status();
}

// ------------------------------------------------------------------------------------------- streaming hop
// Inverse of the DELAYED frame for stem st: masked spectrum -> time frame -> synthesis window on the last 2048 samples ->
// 50 % overlap-add with the kept half -> output segment interleaved by 2*nstems (Spleeter4Stems.c:64-101,272-320).
// srt_live_inverse_kernel runs it for every config but the plugin's.  The plugin's config (4 stems, oob 0.25 / 0 / 0.25 / 0.25) keeps
// srt_stream_inverse_kernel below unchanged: under fp contract(fast) the compiler fuses the mask products into FMAs differently once the
// body is shared or the weight is an argument (measured: 1-ulp differences on most output samples at 256 x 1536, with no source form
// found that reproduces the fixed kernel's choice), and the plugin's output must stay bit-identical.
__device__ __forceinline__ void srt_stream_inverse_body(const SrtStreamHop& p, int st, cf* s_tw, cf* s_x)
{
    const int tid = threadIdx.x;
    fft_load_twiddles(s_tw, p.twiddle, tid);
    const cf* specL = reinterpret_cast<const cf*>(p.specRow);
    const cf* specR = reinterpret_cast<const cf*>(p.specRow) + p.specChStride;
    const float* mL = p.maskRow + st * p.maskStemStride;
    const float* mR = mL + p.maskChStride;
    const float oob = p.oob[st];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int k = tid + 256 * j;
        if (k <= 2048) {
            const cf sl = specL[k], sr = specR[k];
            float gl = oob, gr = oob;
            if (k < p.F) { gl = mL[k]; gr = mR[k]; }
            const float reL = sl.x * gl, imL = sl.y * gl, reR = sr.x * gr, imR = sr.y * gr;
            if (k == 0) s_x[0] = f2(reR, reL);
            else if (k == 2048) s_x[2048] = f2(reR - imR, reL - imL);
            else {
                s_x[k] = f2(reR - imL, reL + imR);
                s_x[4096 - k] = f2(reR + imL, reL - imR);
            }
        }
    }
    __syncthreads();
    cf v[16];
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) v[n2] = s_x[tid + 256 * n2];
    __syncthreads();
    fft4096(v, s_x, s_tw, tid);
    float* ovL = p.overlap + (size_t)(2 * st) * 1024;
    float* ovR = ovL + 1024;
    const int os = 2 * p.nstems;
    // thread holds samples tid + 256*k2; only the last 2048 are synthesised.  k2 = 8..11 -> output, 12..15 -> kept half.
#pragma unroll
    for (int k2 = 8; k2 < 12; ++k2) {
        const int i = tid + 256 * (k2 - 8);                                   // 0..1023
        const float w0 = p.synthesisWnd[i], w1 = p.synthesisWnd[i + 1024];
        const cf y0 = v[FFT16_AT(k2)], y1 = v[FFT16_AT(k2 + 4)];
        p.out[(size_t)i * os + 2 * st + 0] = ovL[i] + y0.y * w0;             // mOverlapStage2dash + timeDomainOut (:313-315)
        p.out[(size_t)i * os + 2 * st + 1] = ovR[i] + y0.x * w0;
        ovL[i] = y1.y * w1;                                                   // :317-318
        ovR[i] = y1.x * w1;
    }
}

// one workgroup per stem (blockIdx.x = stem < p.nstems)
__global__ void __launch_bounds__(256) srt_live_inverse_kernel(const SrtStreamHop p)
{
    __shared__ cf s_tw[FFT_TW_F2];
    __shared__ cf s_x[FFT_SMEM_F2];
    srt_stream_inverse_body(p, blockIdx.x, s_tw, s_x);
}

// Inverse of the DELAYED frame for one stem (blockIdx.x = stem): masked spectrum -> time frame -> synthesis window on the
// last 2048 samples -> 50 % overlap-add with the kept half -> interleaved-by-8 output segment (Spleeter4Stems.c:64-101,272-320).
__global__ void __launch_bounds__(256) srt_stream_inverse_kernel(const SrtStreamHop p)
{
    __shared__ cf s_tw[FFT_TW_F2];
    __shared__ cf s_x[FFT_SMEM_F2];
    const int tid = threadIdx.x, st = blockIdx.x;
    fft_load_twiddles(s_tw, p.twiddle, tid);
    const cf* specL = reinterpret_cast<const cf*>(p.specRow);
    const cf* specR = reinterpret_cast<const cf*>(p.specRow) + p.specChStride;
    const float* mL = p.maskRow + st * p.maskStemStride;
    const float* mR = mL + p.maskChStride;
    const float oob = st == 1 ? 0.0f : 0.25f;                      // Spleeter4Stems.c:73,281
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int k = tid + 256 * j;
        if (k <= 2048) {
            const cf sl = specL[k], sr = specR[k];
            float gl = oob, gr = oob;
            if (k < p.F) { gl = mL[k]; gr = mR[k]; }
            const float reL = sl.x * gl, imL = sl.y * gl, reR = sr.x * gr, imR = sr.y * gr;
            if (k == 0) s_x[0] = f2(reR, reL);
            else if (k == 2048) s_x[2048] = f2(reR - imR, reL - imL);
            else {
                s_x[k] = f2(reR - imL, reL + imR);
                s_x[4096 - k] = f2(reR + imL, reL - imR);
            }
        }
    }
    __syncthreads();
    cf v[16];
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) v[n2] = s_x[tid + 256 * n2];
    __syncthreads();
    fft4096(v, s_x, s_tw, tid);
    float* ovL = p.overlap + (size_t)(2 * st) * 1024;
    float* ovR = ovL + 1024;
    // thread holds samples tid + 256*k2; only the last 2048 are synthesised.  k2 = 8..11 -> output, 12..15 -> kept half.
#pragma unroll
    for (int k2 = 8; k2 < 12; ++k2) {
        const int i = tid + 256 * (k2 - 8);                                   // 0..1023
        const float w0 = p.synthesisWnd[i], w1 = p.synthesisWnd[i + 1024];
        const cf y0 = v[FFT16_AT(k2)], y1 = v[FFT16_AT(k2 + 4)];
        p.out[(size_t)i * 8 + 2 * st + 0] = ovL[i] + y0.y * w0;              // mOverlapStage2dash + timeDomainOut (:313-315)
        p.out[(size_t)i * 8 + 2 * st + 1] = ovR[i] + y0.x * w0;
        ovL[i] = y1.y * w1;                                                   // :317-318
        ovR[i] = y1.x * w1;
    }
}

// Forward transform of the CURRENT 4096 ring samples with the asymmetric analysis window; spectrum + magnitude rows
// of the collecting batch (Spleeter4Stems.c:261-267,322-349).
__global__ void __launch_bounds__(256) srt_stream_forward_kernel(const SrtStreamHop p)
{
    __shared__ cf s_tw[FFT_TW_F2];
    __shared__ cf s_x[FFT_SMEM_F2];
    const int tid = threadIdx.x;
    fft_load_twiddles(s_tw, p.twiddle, tid);
    __syncthreads();
    cf v[16];
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) {
        const int n = tid + 256 * n2, k = (n + p.inPos) & 4095;
        const float w = p.analysisWnd[n];
        v[n2] = f2(p.ring[k] * w, p.ring[4096 + k] * w);
    }
    fft4096(v, s_x, s_tw, tid);
    __syncthreads();
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) s_x[tid + 256 * k2] = v[FFT16_AT(k2)];
    __syncthreads();
    cf* specL = reinterpret_cast<cf*>(p.specRow);
    cf* specR = reinterpret_cast<cf*>(p.specRow) + p.specChStride;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int k = tid + 256 * j;
        if (k <= 2048) {
            const cf zk = s_x[k], zm = s_x[(4096 - k) & 4095];
            const cf sl = f2(zk.x + zm.x, zm.y - zk.y);
            const cf sr = f2(zk.y + zm.y, zk.x - zm.x);
            specL[k] = sl; specR[k] = sr;
            if (k < p.F) {
                p.magRow[k] = hypotf(sl.x, sl.y) * 4096.0f;
                p.magRow[p.magChStride + k] = hypotf(sr.x, sr.y) * 4096.0f;
            }
        }
    }
}

int srt_launch_stream_hop(const SrtStreamHop& p, hipStream_t s)
{
    if (p.nstems < 1 || p.nstems > SRT_MAX_STEMS) return -1;
    const bool plugin = p.nstems == 4 && p.oob[0] == 0.25f && p.oob[1] == 0.0f && p.oob[2] == 0.25f && p.oob[3] == 0.25f;
    if (plugin) SRT_LAUNCH(srt_stream_inverse_kernel, dim3(4), dim3(256), 0, s, p);           // reads the delayed row ...
    else SRT_LAUNCH(srt_live_inverse_kernel, dim3(p.nstems), dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -1;
    SRT_LAUNCH(srt_stream_forward_kernel, dim3(1), dim3(256), 0, s, p);     // ... before the current frame overwrites it
    return srt_launch_status();
}

// The hop inverse of a live stream that combines its stems (srtLiveCreateEx): one workgroup per OUTPUT m.  The prologue forms the gain of
// the thread's nine bins for both channels from all S mask rows,
//   h = G[m][S];  for s = 0 .. S-1 ascending:  h = fmaf(G[m][s], g_s, h)
// (srt_mix_chain's arithmetic: fp32, one fused multiply-add per stem, nothing else contracted), g_s = the mask value below F and above it oob[s] or, EXT, the
// row's value of the average extension's table.  G travels by value in the launch; the stem loop is workgroup-uniform, so its entries, the weights and the
// table values are scalar loads.  Stems outermost: the 18 mask loads of a stem are in flight together.  Everything after the gains is srt_stream_inverse_body.
#pragma clang fp contract(off)
template <bool EXT>
__device__ __forceinline__ void srt_live_combine_gains(const SrtLiveCombineHop& p, int m, int tid, float (&hl)[9], float (&hr)[9])
{
    const float dry = p.gain[m][p.nstems];
#pragma unroll
    for (int j = 0; j < 9; ++j) hl[j] = hr[j] = dry;
    for (int s = 0; s < p.nstems; ++s) {
        const float gm = p.gain[m][s];
        const float* mL = p.maskRow + (size_t)s * p.maskStemStride;
        const float* mR = mL + p.maskChStride;
        float ol = p.oob[s], orr = ol;
        if constexpr (EXT) { ol = p.ext[(size_t)s * p.extStemStride]; orr = p.ext[(size_t)s * p.extStemStride + 1]; }
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int k = tid + 256 * j, km = min(k, p.F - 1);           // (bins >= F read the row's last value and drop it: no load past the row)
            float vl = mL[km], vr = mR[km];
            if (k >= p.F) { vl = ol; vr = orr; }
            hl[j] = fmaf(gm, vl, hl[j]); hr[j] = fmaf(gm, vr, hr[j]);
        }
    }
}
#pragma clang fp contract(fast)

template <bool EXT>
__global__ void __launch_bounds__(256) srt_live_combine_inverse_kernel(const SrtLiveCombineHop p)
{
    __shared__ cf s_tw[FFT_TW_F2];
    __shared__ cf s_x[FFT_SMEM_F2];
    const int tid = threadIdx.x, m = blockIdx.x;
    fft_load_twiddles(s_tw, p.twiddle, tid);
    const cf* specL = reinterpret_cast<const cf*>(p.specRow);
    const cf* specR = reinterpret_cast<const cf*>(p.specRow) + p.specChStride;
    float hl[9], hr[9];
    srt_live_combine_gains<EXT>(p, m, tid, hl, hr);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int k = tid + 256 * j;
        if (k <= 2048) {
            const cf sl = specL[k], sr = specR[k];
            const float gl = hl[j], gr = hr[j];
            const float reL = sl.x * gl, imL = sl.y * gl, reR = sr.x * gr, imR = sr.y * gr;
            if (k == 0) s_x[0] = f2(reR, reL);
            else if (k == 2048) s_x[2048] = f2(reR - imR, reL - imL);
            else {
                s_x[k] = f2(reR - imL, reL + imR);
                s_x[4096 - k] = f2(reR + imL, reL - imR);
            }
        }
    }
    __syncthreads();
    cf v[16];
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) v[n2] = s_x[tid + 256 * n2];
    __syncthreads();
    fft4096(v, s_x, s_tw, tid);
    float* ovL = p.overlap + (size_t)(2 * m) * 1024;
    float* ovR = ovL + 1024;
    const int os = 2 * p.n_out;
#pragma unroll
    for (int k2 = 8; k2 < 12; ++k2) {                                         // as srt_stream_inverse_body: k2 = 8..11 -> output, 12..15 -> kept half
        const int i = tid + 256 * (k2 - 8);
        const float w0 = p.synthesisWnd[i], w1 = p.synthesisWnd[i + 1024];
        const cf y0 = v[FFT16_AT(k2)], y1 = v[FFT16_AT(k2 + 4)];
        p.out[(size_t)i * os + 2 * m + 0] = ovL[i] + y0.y * w0;
        p.out[(size_t)i * os + 2 * m + 1] = ovR[i] + y0.x * w0;
        ovL[i] = y1.y * w1;
        ovR[i] = y1.x * w1;
    }
}

// q: the combining inverse (n_out workgroups); p: the hop's SrtStreamHop, of which only the forward transform's fields are used
int srt_launch_live_combine_hop(const SrtLiveCombineHop& q, const SrtStreamHop& p, hipStream_t s)
{
    if (q.nstems < 1 || q.nstems > SRT_MAX_STEMS || q.n_out < 1 || q.n_out > SRT_MAX_STEMS || q.F < 1) return -1;
    if (q.ext) SRT_LAUNCH((srt_live_combine_inverse_kernel<true>), dim3(q.n_out), dim3(256), 0, s, q);
    else SRT_LAUNCH((srt_live_combine_inverse_kernel<false>), dim3(q.n_out), dim3(256), 0, s, q);
    if (hipGetLastError() != hipSuccess) return -1;
    SRT_LAUNCH(srt_stream_forward_kernel, dim3(1), dim3(256), 0, s, p);     // after the inverse has read the delayed row, as srt_launch_stream_hop
    return srt_launch_status();
}

// The hop inverse of a live stream with the Wiener filter (srtLiveCreateWiener): one workgroup per OUTPUT m, as the combining inverse.  The filter
// is folded into the prologue: per bin k < F the thread loads s_L, s_R and the S mask values of both channels, runs the filter's chain for ALL stems - w_start,
// then p.iters times w_iter on the joined run's R tables with delta = sqrt(eps) (a / 4096)^2, the statements the offline kernels run (srt_wiener_chain.h) - and
// forms the output's spectrum per complex component,
//   h = G[m][S] s;  for j = 0 .. S-1 ascending:  h = fmaf(G[m][j], y_j, h)
// (srtIstftWienerEx's chain: one rounded product, one fused multiply-add per stem, nothing else contracted).  Above F the output is srt_live_combine_gains' gain
// chain on oob / the extension's row (workgroup-uniform: computed once) times s: the extension follows the mask, not the filter.  Every output recomputes the chain
// of every stem: one launch fewer on a hop that is bound by launch latency.  The nine bins are walked one after the other (no unrolling) so that yl / yr exist
// once.  An instance without a mix launches this kernel with the identity, so a one-hot row and the stem come out of one compiled copy of the chain and agree
// bit for bit.  Zero spectrum (the hops before the first join, silence): every y is exactly 0 and delta > 0 keeps the determinant positive - 0, never NaN.
// Everything from the s_x packing on is srt_stream_inverse_body.
#include "srt_wiener_chain.h"      // here, where the file's contraction state is the explicit `fast` the header leaves behind: the kernels above compile as they did
#pragma clang fp contract(off)
template <bool EXT>
__device__ __forceinline__ void srt_live_wiener_oob(const SrtLiveWienerHop& p, int m, float& hl, float& hr)
{
    hl = hr = p.gain[m][p.nstems];
    for (int s = 0; s < p.nstems; ++s) {
        float ol = p.oob[s], orr = ol;
        if constexpr (EXT) { ol = p.ext[(size_t)s * p.extStemStride]; orr = p.ext[(size_t)s * p.extStemStride + 1]; }
        hl = fmaf(p.gain[m][s], ol, hl); hr = fmaf(p.gain[m][s], orr, hr);
    }
}
__device__ __forceinline__ float2 srt_live_wiener_mix(const SrtLiveWienerHop& p, int m, int S, float2 s, const float2 (&y)[SRT_MAX_STEMS])
{
    const float g = p.gain[m][S];
    float hx = g * s.x, hy = g * s.y;
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j)
        if (j < S) { const float gj = p.gain[m][j]; hx = fmaf(gj, y[j].x, hx); hy = fmaf(gj, y[j].y, hy); }
    return make_float2(hx, hy);
}
#pragma clang fp contract(fast)

template <bool EXT>
__global__ void __launch_bounds__(256) srt_live_wiener_inverse_kernel(const SrtLiveWienerHop p)
{
    __shared__ cf s_tw[FFT_TW_F2];
    __shared__ cf s_x[FFT_SMEM_F2];
    const int tid = threadIdx.x, m = blockIdx.x, S = p.nstems;
    fft_load_twiddles(s_tw, p.twiddle, tid);
    const float2* specL = p.specRow;
    const float2* specR = p.specRow + p.specChStride;
    const float al = p.scal[0] * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    float ol, orr;
    srt_live_wiener_oob<EXT>(p, m, ol, orr);
#pragma unroll 1
    for (int j = 0; j < 9; ++j) {
        const int k = tid + 256 * j;
        if (k <= 2048) {
            const float2 sL = specL[k], sR = specR[k];
            float reL, imL, reR, imR;
            if (k < p.F) {
                float2 yl[SRT_MAX_STEMS], yr[SRT_MAX_STEMS];
                w_start(yl, yr, sL, sR, p.maskRow + k, p.maskStemStride, p.maskChStride, S);
                for (int i = 0; i < p.iters; ++i)
                    w_iter<true>(yl, yr, sL, sR, p.rtab + (size_t)i * S * p.F + k, p.F, delta, S);
                const float2 hL = srt_live_wiener_mix(p, m, S, sL, yl), hR = srt_live_wiener_mix(p, m, S, sR, yr);
                reL = hL.x; imL = hL.y; reR = hR.x; imR = hR.y;
            } else { reL = sL.x * ol; imL = sL.y * ol; reR = sR.x * orr; imR = sR.y * orr; }
            if (k == 0) s_x[0] = f2(reR, reL);
            else if (k == 2048) s_x[2048] = f2(reR - imR, reL - imL);
            else {
                s_x[k] = f2(reR - imL, reL + imR);
                s_x[4096 - k] = f2(reR + imL, reL - imR);
            }
        }
    }
    __syncthreads();
    cf v[16];
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) v[n2] = s_x[tid + 256 * n2];
    __syncthreads();
    fft4096(v, s_x, s_tw, tid);
    float* ovL = p.overlap + (size_t)(2 * m) * 1024;
    float* ovR = ovL + 1024;
    const int os = 2 * p.n_out;
#pragma unroll
    for (int k2 = 8; k2 < 12; ++k2) {                                         // as srt_stream_inverse_body: k2 = 8..11 -> output, 12..15 -> kept half
        const int i = tid + 256 * (k2 - 8);
        const float w0 = p.synthesisWnd[i], w1 = p.synthesisWnd[i + 1024];
        const cf y0 = v[FFT16_AT(k2)], y1 = v[FFT16_AT(k2 + 4)];
        p.out[(size_t)i * os + 2 * m + 0] = ovL[i] + y0.y * w0;
        p.out[(size_t)i * os + 2 * m + 1] = ovR[i] + y0.x * w0;
        ovL[i] = y1.y * w1;
        ovR[i] = y1.x * w1;
    }
}

// q: the filtering inverse (n_out workgroups); p: the hop's SrtStreamHop, of which only the forward transform's fields are used
int srt_launch_live_wiener_hop(const SrtLiveWienerHop& q, const SrtStreamHop& p, hipStream_t s)
{
    if (q.nstems < 1 || q.nstems > SRT_MAX_STEMS || q.n_out < 1 || q.n_out > SRT_MAX_STEMS || q.F < 1 || q.F > SRT_HALF - 1 ||
        q.iters < 1 || q.iters > SRT_WIENER_MAX_ITERS || !q.rtab || !q.scal) return -1;
    if (q.ext) SRT_LAUNCH((srt_live_wiener_inverse_kernel<true>), dim3(q.n_out), dim3(256), 0, s, q);
    else SRT_LAUNCH((srt_live_wiener_inverse_kernel<false>), dim3(q.n_out), dim3(256), 0, s, q);
    if (hipGetLastError() != hipSuccess) return -1;
    SRT_LAUNCH(srt_stream_forward_kernel, dim3(1), dim3(256), 0, s, p);     // after the inverse has read the delayed row, as srt_launch_stream_hop
    return srt_launch_status();
}

// Live spectrum-window gather (srtLiveCreateWiener): the spectrum ring holds frame g in row g mod R of each channel, R >= T; the statistics want the window's
// oldest frame in row 0.  dst[c][i][:] = ring[c][(i + rot) mod R][:] for i < T, one workgroup per (row, 512 floats), 16-byte loads and stores (a row is
// SRT_SPEC_LD complex values = 1026 float4).
__global__ void __launch_bounds__(128) srt_live_spec_gather_kernel(const float4* __restrict__ ring, float4* __restrict__ dst, int T, int R, int rot)
{
    constexpr int LD4 = SRT_SPEC_LD / 2;
    const int f = blockIdx.x * 128 + threadIdx.x;
    if (f >= LD4) return;
    const int row = blockIdx.y, c = row >= T ? 1 : 0, i = row - c * T;
    int src = i + rot;
    if (src >= R) src -= R;
    dst[(size_t)row * LD4 + f] = ring[((size_t)c * R + src) * LD4 + f];
}

int srt_launch_live_spec_gather(const float2* ring, float2* dst, int T, int R, int rot, hipStream_t s)
{
    static_assert(SRT_SPEC_LD % 2 == 0, "a spectrum row is a whole number of float4");
    if (T < 1 || R < T || rot < 0 || rot >= R) return -1;
    SRT_LAUNCH(srt_live_spec_gather_kernel, dim3((SRT_SPEC_LD / 2 + 127) / 128, 2 * T), dim3(128), 0, s,
               reinterpret_cast<const float4*>(ring), reinterpret_cast<float4*>(dst), T, R, rot);
    return srt_launch_status();
}

// Live window gather (srt_stream.hip): the magnitude ring holds frame g in row g mod T of each channel; the network wants the
// window's oldest frame in row 0.  dst[c][i][:] = ring[c][(i + rot) mod T][:], one workgroup per (row, 512 columns), 16-byte
// loads and stores.  rot = 0 is a plain copy (the plugin's geometry, where every window starts at a multiple of T).
__global__ void __launch_bounds__(128) srt_live_gather_kernel(const float4* __restrict__ ring, float4* __restrict__ dst, int T, int F4, int rot)
{
    const int f = blockIdx.x * 128 + threadIdx.x;
    if (f >= F4) return;
    const int row = blockIdx.y, c = row >= T ? 1 : 0, i = row - c * T;
    int src = i + rot;
    if (src >= T) src -= T;
    dst[(size_t)row * F4 + f] = ring[((size_t)c * T + src) * F4 + f];
}

int srt_launch_live_gather(const float* ring, float* dst, int T, int F, int rot, hipStream_t s)
{
    if (T < 1 || F < 4 || F % 4 || rot < 0 || rot >= T) return -1;
    const int F4 = F / 4;
    SRT_LAUNCH(srt_live_gather_kernel, dim3((F4 + 127) / 128, 2 * T), dim3(128), 0, s,
               reinterpret_cast<const float4*>(ring), reinterpret_cast<float4*>(dst), T, F4, rot);
    return srt_launch_status();
}
