// srt_resample.hip — band-limited sample-rate conversion of planar stereo fp32 PCM in HBM (srtResampler*, include/spleeterrt_amd.h).
//
// The arithmetic is libsamplerate's sinc converter as the reference program runs it (Executable/main.c:264-271 -> src_simple ->
// libsamplerate/src_sinc.c:366-512, sinc_stereo_vari_process / calc_output_stereo), restated with an exact rational phase:
//   output frame n sits at input position n * fs_in / fs_out = i + frac   (64-bit integers; frac = ((n fs_in) mod fs_out) / fs_out)
//   float_increment = index_inc * min(r, 1), increment = lrint(float_increment * 4096) (12 fraction bits), start = lrint(frac * float_increment * 4096)
//   left half:  taps x[i - k] at filter index start + k increment        (k >= 0, index <= (table_len - 2) << 12)
//   right half: taps x[i + 1 + j] at filter index increment - start + j increment   (index > 0, same bound)
//   weight = c[f >> 12] + (f & 4095) / 4096 * (c[(f >> 12) + 1] - c[f >> 12]),   y = min(r, 1) * sum(weight * x),  x = 0 outside [0, n_in)
// The weights of a frame depend only on its phase n mod Q (Q = fs_out / gcd), so srt_resample_bank_kernel evaluates them once per
// resampler into a bank [T/4][Q][4] (T taps per frame, window starting at i - LO); srt_resample_kernel then stages each block's input
// window in LDS and runs the T-tap dot products in fp32 (fixed order, explicit FMAs).  A frame's value depends on its absolute index only:
// any partition of the output range gives the same bits.  When the bank would exceed SRT_RS_BANK_BYTES the kernel evaluates the same
// weight function per tap instead (ONFLY = true): same floats, same FMA order, same bits.
#include "srt_internal.h"
#include "srt_rs.h"
#include "../../include/spleeterrt_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>

struct SrtRsArgs {
    SrtRsGeom g;
    const float* table; const float4* bank;
    const float* L; const float* R; long long nIn;
    float* Lo; float* Ro;
    long long out0, outEnd;  // frames [out0, outEnd); Lo[0] holds frame out0
    int B, opt;              // frames per workgroup, frames per thread (B = blockDim.x * opt)
    long long stepI, stepR, stepM;   // blockDim.x frames further: i += stepI (+1 on carry), (n P) mod Q += stepR, n mod Q += stepM
};

__global__ __launch_bounds__(256) void srt_resample_bank_kernel(SrtRsGeom g, const float* __restrict__ table, float* __restrict__ bank)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x, n = g.Q * g.T4;
    if (e >= n) return;
    const long long q4 = g.Q * 4, m = (e % q4) >> 2;
    const int t = (int)(e / q4) * 4 + (int)(e & 3);
    bank[e] = rs_weight(g, table, rs_start(g, m), t);
}

template <bool ONFLY>
__global__ __launch_bounds__(256) void srt_resample_kernel(SrtRsArgs a)
{
    extern __shared__ float2 win[];
    const SrtRsGeom& g = a.g;
    const long long n0 = a.out0 + (long long)blockIdx.x * a.B;
    const long long nEnd = min(n0 + (long long)a.B, a.outEnd);
    const long long i0 = n0 * g.P / g.Q, s0 = i0 - g.LO;
    const int W = (int)((nEnd - 1) * g.P / g.Q - i0) + g.T4;   // <= floor((B - 1) P / Q) + 1 + T4 frames: the host sized the LDS for that
    for (int j = threadIdx.x; j < W; j += blockDim.x) {
        const long long s = s0 + j;
        float2 v = make_float2(0.0f, 0.0f);
        if (s >= 0 && s < a.nIn) { v.x = a.L[s]; v.y = a.R[s]; }
        win[j] = v;
    }
    __syncthreads();
    long long n = n0 + threadIdx.x;
    if (n >= nEnd) return;
    long long pos = n * g.P, i = pos / g.Q, r = pos - i * g.Q, m = n % g.Q;
    for (int k = 0; k < a.opt && n < nEnd; ++k) {
        const float2* x = win + (i - i0);
        float l0 = 0.0f, r0 = 0.0f, l1 = 0.0f, r1 = 0.0f;
        if (ONFLY) {
            const long long start = rs_start(g, m);
            for (int t = 0; t < g.T4; t += 4) {
                const float w0 = rs_weight(g, a.table, start, t), w1 = rs_weight(g, a.table, start, t + 1);
                const float w2 = rs_weight(g, a.table, start, t + 2), w3 = rs_weight(g, a.table, start, t + 3);
                const float2 x0 = x[t], x1 = x[t + 1], x2 = x[t + 2], x3 = x[t + 3];
                l0 = fmaf(w0, x0.x, l0); r0 = fmaf(w0, x0.y, r0); l1 = fmaf(w1, x1.x, l1); r1 = fmaf(w1, x1.y, r1);
                l0 = fmaf(w2, x2.x, l0); r0 = fmaf(w2, x2.y, r0); l1 = fmaf(w3, x3.x, l1); r1 = fmaf(w3, x3.y, r1);
            }
        } else {
            const float4* wp = a.bank + m;
#pragma unroll 4
            for (int t = 0; t < g.T4; t += 4) {
                const float4 w = wp[(long long)(t >> 2) * g.Q];
                const float2 x0 = x[t], x1 = x[t + 1], x2 = x[t + 2], x3 = x[t + 3];
                l0 = fmaf(w.x, x0.x, l0); r0 = fmaf(w.x, x0.y, r0); l1 = fmaf(w.y, x1.x, l1); r1 = fmaf(w.y, x1.y, r1);
                l0 = fmaf(w.z, x2.x, l0); r0 = fmaf(w.z, x2.y, r0); l1 = fmaf(w.w, x3.x, l1); r1 = fmaf(w.w, x3.y, r1);
            }
        }
        const long long o = n - a.out0;
        a.Lo[o] = l0 + l1;
        if (a.Ro != a.Lo) a.Ro[o] = r0 + r1;
        n += blockDim.x; i += a.stepI; r += a.stepR; m += a.stepM;
        if (r >= g.Q) { r -= g.Q; ++i; }
        if (m >= g.Q) m -= g.Q;
    }
}

// The same frames from two consecutive spans of the stream instead of the whole resident input (srtResampleSpans): stream position s is a.A[s - a0] inside
// [a0, a0 + aLen), a.Bs[s - a0 - aLen] inside the aLen .. aLen + bLen behind it, and 0.0f anywhere else - outside [0, nIn) as above, and where no span holds the
// position, which the host allows for zero-weight taps only (never memory nobody wrote: 0 x NaN is NaN).  NP stereo pairs share every weight: the workgroup stages NP
// windows (pair p's at win + p * winLen) and each 16-byte weight load (or rs_weight evaluation) feeds NP dot products.  Per pair the weights, the order of the
// FMAs and the final l0 + l1 are srt_resample_kernel's, so a frame has srtResample's bits.  blockIdx.y selects the first pair of the workgroup (NP = 1 grids).
struct SrtRsSpanArgs {
    SrtRsGeom g;
    const float* table; const float4* bank;
    const float* A; long long aStride, a0, aLen;
    const float* Bs; long long bStride, bLen;
    long long nIn;
    float* out; long long outStride;
    long long out0, outEnd;
    int B, opt, winLen;
    long long stepI, stepR, stepM;
};

template <bool ONFLY, int NP>
__global__ __launch_bounds__(256) void srt_resample_spans_kernel(SrtRsSpanArgs a)
{
    extern __shared__ float2 win[];
    const SrtRsGeom& g = a.g;
    const int p0 = blockIdx.y * NP;
    const long long n0 = a.out0 + (long long)blockIdx.x * a.B;
    const long long nEnd = min(n0 + (long long)a.B, a.outEnd);
    const long long i0 = n0 * g.P / g.Q, s0 = i0 - g.LO;
    const int W = (int)((nEnd - 1) * g.P / g.Q - i0) + g.T4;   // <= winLen: the host sized the LDS for that
    for (int j = threadIdx.x; j < W; j += blockDim.x) {
        const long long s = s0 + j, ua = s - a.a0, ub = ua - a.aLen;
        const bool live = s >= 0 && s < a.nIn, inA = live && ua >= 0 && ua < a.aLen, inB = live && ub >= 0 && ub < a.bLen;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float2 v = make_float2(0.0f, 0.0f);
            if (inA) { const float* x = a.A + (long long)(2 * (p0 + p)) * a.aStride + ua; v.x = x[0]; v.y = x[a.aStride]; }
            else if (inB) { const float* x = a.Bs + (long long)(2 * (p0 + p)) * a.bStride + ub; v.x = x[0]; v.y = x[a.bStride]; }
            win[p * a.winLen + j] = v;
        }
    }
    __syncthreads();
    long long n = n0 + threadIdx.x;
    if (n >= nEnd) return;
    long long pos = n * g.P, i = pos / g.Q, r = pos - i * g.Q, m = n % g.Q;
    for (int k = 0; k < a.opt && n < nEnd; ++k) {
        const float2* x = win + (i - i0);
        float l0[NP], r0[NP], l1[NP], r1[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) l0[p] = r0[p] = l1[p] = r1[p] = 0.0f;
        if (ONFLY) {
            const long long start = rs_start(g, m);
            for (int t = 0; t < g.T4; t += 4) {
                const float w0 = rs_weight(g, a.table, start, t), w1 = rs_weight(g, a.table, start, t + 1);
                const float w2 = rs_weight(g, a.table, start, t + 2), w3 = rs_weight(g, a.table, start, t + 3);
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const float2* xp = x + p * a.winLen;
                    const float2 x0 = xp[t], x1 = xp[t + 1], x2 = xp[t + 2], x3 = xp[t + 3];
                    l0[p] = fmaf(w0, x0.x, l0[p]); r0[p] = fmaf(w0, x0.y, r0[p]); l1[p] = fmaf(w1, x1.x, l1[p]); r1[p] = fmaf(w1, x1.y, r1[p]);
                    l0[p] = fmaf(w2, x2.x, l0[p]); r0[p] = fmaf(w2, x2.y, r0[p]); l1[p] = fmaf(w3, x3.x, l1[p]); r1[p] = fmaf(w3, x3.y, r1[p]);
                }
            }
        } else {
            const float4* wp = a.bank + m;
            for (int t = 0; t < g.T4; t += 4) {
                const float4 w = wp[(long long)(t >> 2) * g.Q];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const float2* xp = x + p * a.winLen;
                    const float2 x0 = xp[t], x1 = xp[t + 1], x2 = xp[t + 2], x3 = xp[t + 3];
                    l0[p] = fmaf(w.x, x0.x, l0[p]); r0[p] = fmaf(w.x, x0.y, r0[p]); l1[p] = fmaf(w.y, x1.x, l1[p]); r1[p] = fmaf(w.y, x1.y, r1[p]);
                    l0[p] = fmaf(w.z, x2.x, l0[p]); r0[p] = fmaf(w.z, x2.y, r0[p]); l1[p] = fmaf(w.w, x3.x, l1[p]); r1[p] = fmaf(w.w, x3.y, r1[p]);
                }
            }
        }
        const long long o = n - a.out0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float* y = a.out + (long long)(2 * (p0 + p)) * a.outStride + o;
            y[0] = l0[p] + l1[p];
            y[a.outStride] = r0[p] + r1[p];
        }
        n += blockDim.x; i += a.stepI; r += a.stepR; m += a.stepM;
        if (r >= g.Q) { r -= g.Q; ++i; }
        if (m >= g.Q) m -= g.Q;
    }
}

struct srt_resampler {
    int fs_in, fs_out, device, onfly;
    SrtRsGeom g;
    int B, threads;
    size_t ldsBytes;
    hipStream_t stream;
    float* d_table; float* d_bank;
};

static int rs_fail(int code, const char* fmt, const char* detail = "") { return srt_set_error(code, fmt, detail); }
static int rs_fail_who(int code, const char* who, const char* what, const char* detail = "")
{
    char fmt[320];
    snprintf(fmt, sizeof fmt, "%s: %s", who, what);                     // `what` may hold one %s for `detail`; `who` is a plain identifier
    return srt_set_error(code, fmt, detail);
}
static long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

// built-in half filter in the reference's layout (index_inc = 491, 22 438 points): a Kaiser-windowed sinc (beta 12) with its cutoff at
// 0.918 of the lower rate's Nyquist frequency, the window reaching its edge at the table's last point.  Project's own design: passband
// flat to 2e-5 dB up to 17 kHz and stopband below -115 dB from 22.5 kHz at 48 k -> 44.1 k (tests/test_resample.py).
#define SRT_RS_BUILTIN_LEN 22438
#define SRT_RS_BUILTIN_INC 491
static void builtin_table(std::vector<float>& c)
{
    const int n = SRT_RS_BUILTIN_LEN, inc = SRT_RS_BUILTIN_INC;
    const double fc = 0.918, beta = 12.0, half = (n - 1) / (double)inc, PI = 3.141592653589793;
    auto i0 = [](double x) { double s = 1.0, term = 1.0; for (int k = 1; k < 200; ++k) { term *= (x / (2.0 * k)) * (x / (2.0 * k)); s += term; if (term < 1e-18 * s) break; } return s; };
    const double norm = 1.0 / i0(beta);
    c.resize(n);
    for (int k = 0; k < n; ++k) {
        const double t = k / (double)inc, q = t / half, a = fc * t;
        const double sinc = k == 0 ? 1.0 : sin(PI * a) / (PI * a);
        c[k] = (float)(fc * sinc * i0(beta * sqrt(q < 1.0 ? 1.0 - q * q : 0.0)) * norm);
    }
}

size_t srtResampleLength(size_t n_in, int fs_in, int fs_out)
{
    if (fs_in <= 0 || fs_out <= 0) return 0;
    return (size_t)ceil((double)n_in * (fs_out / (double)fs_in));      // main.c:266
}

int srt_rs_geometry(int fs_in, int fs_out, bool has_table, int table_len, int index_inc, const char* who, SrtRsGeom* out)
{
    if (fs_in < SRT_RS_MIN_RATE || fs_in > SRT_RS_MAX_RATE || fs_out < SRT_RS_MIN_RATE || fs_out > SRT_RS_MAX_RATE)
        return rs_fail_who(-1, who, "sample rates must lie in 8000..384000 Hz");
    if (has_table && table_len < 2) return rs_fail_who(-1, who, "table_len must be at least 2");
    if (has_table && index_inc < 1) return rs_fail_who(-1, who, "index_inc must be at least 1");
    if (has_table && table_len > (1 << 24)) return rs_fail_who(-1, who, "table_len above 2^24");
    if (!has_table) { table_len = SRT_RS_BUILTIN_LEN; index_inc = SRT_RS_BUILTIN_INC; }
    SrtRsGeom g;
    const long long gc = gcd_ll(fs_in, fs_out);
    g.P = fs_in / gc; g.Q = fs_out / gc;
    const double r = fs_out / (double)fs_in;
    g.fi = index_inc * (r < 1.0 ? r : 1.0);
    g.scale = g.fi / index_inc;
    g.inc = (long long)rint(g.fi * 4096.0);
    g.maxIdx = (long long)(table_len - 2) << 12;
    if (g.inc < 1) return rs_fail_who(-1, who, "index_inc * min(fs_out / fs_in, 1) rounds to a zero filter increment");
    const long long half = g.maxIdx / g.inc, taps = 2 * half + 2;
    g.LO = (int)half;
    g.T4 = (int)((taps + 3) / 4 * 4);
    *out = g;
    return 0;
}

int srt_rs_filter_create(const SrtRsGeom& g, const float* h_table, int table_len, hipStream_t stream, const char* who, SrtRsFilter* f)
{
    std::vector<float> tab;
    if (!h_table) { builtin_table(tab); table_len = (int)tab.size(); h_table = tab.data(); }
    const size_t bankBytes = (size_t)g.Q * g.T4 * sizeof(float);
    const char* of = getenv("SPLEETERRT_RESAMPLE_ONFLY");               // measurement / test aid: skip the bank (the results are the same bits)
    f->g = g; f->d_table = nullptr; f->d_bank = nullptr;
    f->onfly = bankBytes > SRT_RS_BANK_BYTES || (of && of[0] == '1');
    hipError_t e = hipMalloc((void**)&f->d_table, (size_t)table_len * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_table, h_table, (size_t)table_len * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && !f->onfly) e = hipMalloc((void**)&f->d_bank, bankBytes);
    if (e == hipSuccess && !f->onfly) {
        const long long n = g.Q * g.T4;
        SRT_LAUNCH(srt_resample_bank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g, f->d_table, f->d_bank);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);              // the host table may go away after the call
    if (e != hipSuccess) { srt_rs_filter_free(f); return rs_fail_who(-2, who, "HIP error: %s", hipGetErrorString(e)); }
    return 0;
}

void srt_rs_filter_free(SrtRsFilter* f)
{
    if (f->d_table) hipFree(f->d_table);
    if (f->d_bank) hipFree(f->d_bank);
    f->d_table = f->d_bank = nullptr;
}

int srtResamplerCreate(int fs_in, int fs_out, const float* h_table, int table_len, int index_inc, void* stream, srt_resampler** out)
{
    const char* who = "srtResamplerCreate";
    if (!out) return rs_fail(-1, "srtResamplerCreate: null output pointer");
    *out = nullptr;
    SrtRsGeom g;
    if (const int rc = srt_rs_geometry(fs_in, fs_out, h_table != nullptr, table_len, index_inc, who, &g)) return rc;
    // workgroup size: the most frames whose input window fits the LDS budget
    int B = 1024;
    auto window = [&](int b) { return (size_t)(((long long)(b - 1) * g.P) / g.Q + 1 + g.T4) * sizeof(float2); };
    while (B > 64 && window(B) > SRT_RS_LDS_BYTES) B >>= 1;
    if (window(B) > SRT_RS_LDS_BYTES) return rs_fail(-1, "srtResamplerCreate: filter too long for this rate pair (input window above 64 KiB)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return rs_fail(-3, "srtResamplerCreate: no HIP device (this library has no CPU path)");
    srt_resampler* s = new (std::nothrow) srt_resampler();
    if (!s) return rs_fail(-2, "srtResamplerCreate: out of host memory");
    s->fs_in = fs_in; s->fs_out = fs_out; s->g = g; s->B = B; s->threads = B < 256 ? B : 256; s->ldsBytes = window(B);
    s->stream = (hipStream_t)stream; s->d_table = nullptr; s->d_bank = nullptr;
    const hipError_t e = hipGetDevice(&s->device);
    if (e != hipSuccess) { delete s; return rs_fail(-2, "srtResamplerCreate: HIP error: %s", hipGetErrorString(e)); }
    SrtRsFilter f;
    if (const int rc = srt_rs_filter_create(g, h_table, table_len, s->stream, who, &f)) { delete s; return rc; }
    s->onfly = f.onfly; s->d_table = f.d_table; s->d_bank = f.d_bank;
    *out = s;
    return 0;
}

int srtResamplerDestroy(srt_resampler* s)
{
    if (!s) return 0;
    if (s->stream) hipStreamSynchronize(s->stream);
    else hipDeviceSynchronize();
    if (s->d_table) hipFree(s->d_table);
    if (s->d_bank) hipFree(s->d_bank);
    delete s;
    return 0;
}

int srtResample(srt_resampler* s, const float* d_L, const float* d_R, size_t n_in, size_t out0, size_t n_out, float* d_Lo, float* d_Ro)
{
    if (!s) return rs_fail(-1, "srtResample: null resampler");
    if (n_out == 0) return 0;
    if (!d_L || !d_R || !d_Lo || !d_Ro) return rs_fail(-1, "srtResample: null buffer");
    if (d_Lo == d_Ro && d_L != d_R) return rs_fail(-1, "srtResample: d_Lo == d_Ro needs mono input (d_L == d_R)");
    const unsigned long long nb = (n_out + s->B - 1) / s->B;
    if (nb > 0x7fffffffull || out0 + n_out > (size_t)1 << 44) return rs_fail(-1, "srtResample: output range too large");
    SrtRsArgs a;
    a.g = s->g; a.table = s->d_table; a.bank = (const float4*)s->d_bank;
    a.L = d_L; a.R = d_R; a.nIn = (long long)n_in; a.Lo = d_Lo; a.Ro = d_Ro;
    a.out0 = (long long)out0; a.outEnd = (long long)(out0 + n_out);
    a.B = s->B; a.opt = s->B / s->threads;
    const long long adv = (long long)s->threads * s->g.P;
    a.stepI = adv / s->g.Q; a.stepR = adv % s->g.Q; a.stepM = s->threads % s->g.Q;
    if (s->onfly) SRT_LAUNCH(srt_resample_kernel<true>, dim3((unsigned)nb), dim3(s->threads), s->ldsBytes, s->stream, a);
    else SRT_LAUNCH(srt_resample_kernel<false>, dim3((unsigned)nb), dim3(s->threads), s->ldsBytes, s->stream, a);
    if (srt_launch_status()) return rs_fail(-2, "srtResample: kernel launch failed%s", "");
    return 0;
}

// Launch shape of the spans kernel: every pair of a frame block in one workgroup where `pairs` windows of B >= 64 frames fit the LDS budget (B shrinks as in
// srtResamplerCreate), else one pair per workgroup and a second grid dimension over the pairs.  -1: not even one pair's window of 64 frames fits.
int srt_rs_spans_shape(const SrtRsGeom& g, int pairs, int* B_out, int* per_wg, int* win_len)
{
    auto window = [&](int b) { return (size_t)(((long long)(b - 1) * g.P) / g.Q + 1 + g.T4); };
    for (int np = pairs; ; np = 1) {
        int B = 1024;
        while (B > 64 && np * window(B) * sizeof(float2) > SRT_RS_LDS_BYTES) B >>= 1;
        if (np * window(B) * sizeof(float2) <= SRT_RS_LDS_BYTES) { *B_out = B; *per_wg = np; *win_len = (int)window(B); return 0; }
        if (np == 1) return -1;
    }
}

template <bool ONFLY>
static void spans_launch_np(int np, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const SrtRsSpanArgs& a)
{
    switch (np) {
    case 1: SRT_LAUNCH((srt_resample_spans_kernel<ONFLY, 1>), grid, block, lds, stream, a); break;
    case 2: SRT_LAUNCH((srt_resample_spans_kernel<ONFLY, 2>), grid, block, lds, stream, a); break;
    case 3: SRT_LAUNCH((srt_resample_spans_kernel<ONFLY, 3>), grid, block, lds, stream, a); break;
    case 4: SRT_LAUNCH((srt_resample_spans_kernel<ONFLY, 4>), grid, block, lds, stream, a); break;
    case 5: SRT_LAUNCH((srt_resample_spans_kernel<ONFLY, 5>), grid, block, lds, stream, a); break;
    case 6: SRT_LAUNCH((srt_resample_spans_kernel<ONFLY, 6>), grid, block, lds, stream, a); break;
    case 7: SRT_LAUNCH((srt_resample_spans_kernel<ONFLY, 7>), grid, block, lds, stream, a); break;
    default: SRT_LAUNCH((srt_resample_spans_kernel<ONFLY, 8>), grid, block, lds, stream, a); break;
    }
}

// Checks, then one launch on `stream`.  Taps 0 .. 2 LO + 1 of a frame's window count as weighted (srtResampleHorizon's view: the two outermost may have a zero
// weight at some phases); the taps that pad the window to T4 never do.
int srt_rs_spans_launch(const SrtRsFilter& f, const SrtRsSpans& s, hipStream_t stream, const char* who)
{
    const SrtRsGeom& g = f.g;
    if (s.pairs < 1 || s.pairs > SRT_MAX_STEMS) return rs_fail_who(-1, who, "pairs must be 1..SRT_MAX_STEMS");
    if (s.n_out == 0) return 0;
    if ((s.a_len && !s.a) || (s.b_len && !s.b) || !s.out) return rs_fail_who(-1, who, "null buffer");
    if (s.a_len > s.a_stride || s.b_len > s.b_stride || s.n_out > s.out_stride) return rs_fail_who(-1, who, "a plane stride is shorter than its span");
    const size_t big = (size_t)1 << 44;
    if (s.out0 > big || s.n_out > big || s.out0 + s.n_out > big || s.n_in > ((size_t)1 << 62) || s.a_len > big || s.b_len > big || s.a0 > (long long)1 << 62 || s.a0 < -((long long)1 << 62))
        return rs_fail_who(-1, who, "output range too large");
    int B, np, winLen;
    if (srt_rs_spans_shape(g, s.pairs, &B, &np, &winLen)) return rs_fail_who(-1, who, "filter too long for this rate pair (input window above 64 KiB)");
    const unsigned long long nb = (s.n_out + B - 1) / B;
    if (nb > 0x7fffffffull) return rs_fail_who(-1, who, "output range too large");
    // the frames of [0, n_in) a weighted tap of the range falls on
    const long long iFirst = (long long)s.out0 * g.P / g.Q, iLast = (long long)(s.out0 + s.n_out - 1) * g.P / g.Q;
    const long long lo = iFirst - g.LO > 0 ? iFirst - g.LO : 0, hi = iLast + g.LO + 2 < (long long)s.n_in ? iLast + g.LO + 2 : (long long)s.n_in;
    if (lo < hi && (lo < s.a0 || hi > s.a0 + (long long)s.a_len + (long long)s.b_len))
        return rs_fail_who(-1, who, "a requested frame has a weighted tap on an input frame that neither span holds");
    SrtRsSpanArgs a;
    a.g = g; a.table = f.d_table; a.bank = (const float4*)f.d_bank;
    a.A = s.a; a.aStride = (long long)s.a_stride; a.a0 = s.a0; a.aLen = (long long)s.a_len;
    a.Bs = s.b; a.bStride = (long long)s.b_stride; a.bLen = (long long)s.b_len;
    a.nIn = (long long)s.n_in; a.out = s.out; a.outStride = (long long)s.out_stride;
    a.out0 = (long long)s.out0; a.outEnd = (long long)(s.out0 + s.n_out);
    const int threads = B < 256 ? B : 256;
    a.B = B; a.opt = B / threads; a.winLen = winLen;
    const long long adv = (long long)threads * g.P;
    a.stepI = adv / g.Q; a.stepR = adv % g.Q; a.stepM = threads % g.Q;
    const dim3 grid((unsigned)nb, (unsigned)(s.pairs / np)), block(threads);
    const size_t lds = (size_t)np * winLen * sizeof(float2);
    if (f.onfly) spans_launch_np<true>(np, grid, block, lds, stream, a);
    else spans_launch_np<false>(np, grid, block, lds, stream, a);
    if (srt_launch_status()) return rs_fail_who(-2, who, "kernel launch failed");
    return 0;
}

int srtResampleSpans(srt_resampler* s, int pairs, const float* d_a, size_t a_stride, long long a0, size_t a_len, const float* d_b, size_t b_stride, size_t b_len,
                     size_t n_in, size_t out0, size_t n_out, float* d_out, size_t out_stride)
{
    if (!s) return rs_fail(-1, "srtResampleSpans: null resampler");
    SrtRsFilter f;
    f.g = s->g; f.onfly = s->onfly; f.d_table = s->d_table; f.d_bank = s->d_bank;
    const SrtRsSpans sp = { pairs, d_a, a_stride, a0, a_len, d_b, b_stride, b_len, n_in, out0, n_out, d_out, out_stride };
    return srt_rs_spans_launch(f, sp, s->stream, "srtResampleSpans");
}

int srtResampleHost(srt_resampler* s, const float* h_L, const float* h_R, size_t n_in, float* h_Lo, float* h_Ro)
{
    if (!s) return rs_fail(-1, "srtResampleHost: null resampler");
    if (!h_L || !h_R || !h_Lo || !h_Ro) return rs_fail(-1, "srtResampleHost: null buffer");
    const size_t n_out = srtResampleLength(n_in, s->fs_in, s->fs_out);
    if (n_out == 0) return 0;
    const bool mono = h_L == h_R;
    float *dIn = nullptr, *dOut = nullptr;
    const size_t inF = mono ? n_in : 2 * n_in;
    hipError_t e = hipMalloc((void**)&dIn, inF * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dOut, 2 * n_out * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(dIn, h_L, n_in * sizeof(float), hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess && !mono) e = hipMemcpyAsync(dIn + n_in, h_R, n_in * sizeof(float), hipMemcpyHostToDevice, s->stream);
    int rc = 0;
    if (e == hipSuccess) rc = srtResample(s, dIn, mono ? dIn : dIn + n_in, n_in, 0, n_out, dOut, dOut + n_out);
    if (e == hipSuccess && rc == 0) e = hipMemcpyAsync(h_Lo, dOut, n_out * sizeof(float), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && rc == 0) e = hipMemcpyAsync(h_Ro, dOut + n_out, n_out * sizeof(float), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && rc == 0) e = hipStreamSynchronize(s->stream);
    if (dIn) hipFree(dIn);
    if (dOut) hipFree(dOut);
    if (rc) return rc;
    if (e != hipSuccess) return rs_fail(-2, "srtResampleHost: HIP error: %s", hipGetErrorString(e));
    return 0;
}
