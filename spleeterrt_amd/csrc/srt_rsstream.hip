// srt_rsstream.hip — the sample-rate converter of srt_resample.hip as a stream (srtResamplerStream*, include/spleeterrt_amd.h): fed block by
// block, it emits every output frame that has become computable.  The converted stream is the one srtResample defines (output frame j at input
// position j * fs_in / fs_out, input zero before frame 0), with the same weights, tap order and two-accumulator sums, so the concatenation of what
// the calls emit equals srtResample on the whole input bit for bit, for any partition into blocks.
//
// State on the device: a ring [cap][C] of the newest input frames, zero-initialised (a window's zero-padded taps may read slots that hold older
// frames or nothing yet: their weight is 0, so they must only be finite).  Frame j needs input up to floor(j P / Q) + H, H = LO + 1; how many frames a
// call emits is therefore host integer arithmetic (srt_rs_computable): no device-to-host feedback, no host wait, capturable.
// One launch per call: workgroup (x, y) computes up to B <= 256 frames of channel pair y, one frame per thread, from a window staged in LDS out of the
// ring (older frames, wrap resolved at staging) and the call's block (newer frames); the same launch copies the block into the ring, into slots that
// no window of this call reads (cap >= max_block + 2 LO + 1).  The live stream (srt_stream.hip) drives the same kernel through srt_rsstream_launch.
#include "srt_internal.h"
#include "srt_rs.h"
#include "../../include/spleeterrt_amd.h"
#include <stdio.h>
#include <string.h>
#include <new>

__device__ inline long long rs_floordiv(long long a, long long b) { long long q = a / b; if (a - q * b < 0) --q; return q; }      // b > 0

template <bool ONFLY>
__global__ __launch_bounds__(256) void srt_rsstream_kernel(SrtRsStreamArgs a)
{
    extern __shared__ float2 win[];
    const SrtRsGeom& g = a.g;
    const int C = a.C, c0 = 2 * blockIdx.y, c1 = c0 + 1 < C ? c0 + 1 : c0;
    if (a.append) {
        const long long total = (long long)a.n * C, step = (long long)gridDim.x * gridDim.y * blockDim.x;
        for (long long e = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += step) {
            const long long f = e / C;
            const int c = (int)(e - f * C);
            a.ring[((a.have + f) % a.cap) * C + c] = a.inStride ? a.in[c * a.inStride + f] : a.in[e];
        }
    }
    const long long n0 = a.out0 + (long long)blockIdx.x * a.B;
    const long long nEnd = min(n0 + (long long)a.B, a.out0 + (long long)a.nOut);
    if (n0 >= nEnd) return;
    const long long i0 = rs_floordiv(n0 * g.P, g.Q), s0 = i0 - g.LO + a.shift;
    const int W = (int)(rs_floordiv((nEnd - 1) * g.P, g.Q) - i0) + g.T4;      // <= floor((B - 1) P / Q) + 1 + T4 frames: srt_rsstream_block sized the LDS for that
    for (int j = threadIdx.x; j < W; j += blockDim.x) {
        const long long s = s0 + j;
        float2 v = make_float2(0.0f, 0.0f);
        if (s >= 0 && s < a.end) {
            if (s >= a.have) {
                const long long f = s - a.have;                                  // < n: the host keeps end <= have + n
                v.x = a.inStride ? a.in[c0 * a.inStride + f] : a.in[f * C + c0];
                v.y = a.inStride ? a.in[c1 * a.inStride + f] : a.in[f * C + c1];
            } else {
                const float* p = a.ring + (s % a.cap) * C;
                v.x = p[c0]; v.y = p[c1];
            }
        }
        win[j] = v;
    }
    __syncthreads();
    const long long n = n0 + threadIdx.x;
    if (n >= nEnd) return;
    const long long i = rs_floordiv(n * g.P, g.Q);
    long long m = n % g.Q;
    if (m < 0) m += g.Q;
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
    const long long o = (long long)((a.outPos + (int)(n - a.out0)) & a.outMask);
    a.out[c0 * a.outStride + o] = l0 + l1;
    if (c1 != c0) a.out[c1 * a.outStride + o] = r0 + r1;
}

int srt_rsstream_block(const SrtRsGeom& g, size_t* ldsBytes)
{
    int B = 256;
    auto window = [&](int b) { return (size_t)(((long long)(b - 1) * g.P) / g.Q + 1 + g.T4) * sizeof(float2); };
    while (B > 1 && window(B) > SRT_RS_LDS_BYTES) B >>= 1;
    if (window(B) > SRT_RS_LDS_BYTES) return 0;
    *ldsBytes = window(B);
    return B;
}

int srt_rsstream_launch(const SrtRsFilter& f, SrtRsStreamArgs a, size_t ldsBytes, hipStream_t stream)
{
    a.g = f.g; a.table = f.d_table; a.bank = (const float4*)f.d_bank;
    if (a.nOut <= 0 && !(a.append && a.n > 0)) return 0;
    const unsigned nb = a.nOut > 0 ? (unsigned)((a.nOut + a.B - 1) / a.B) : 1u;
    const dim3 grid(nb, (unsigned)((a.C + 1) / 2));
    if (f.onfly) SRT_LAUNCH(srt_rsstream_kernel<true>, grid, dim3(a.B < 64 ? 64 : a.B), ldsBytes, stream, a);
    else SRT_LAUNCH(srt_rsstream_kernel<false>, grid, dim3(a.B < 64 ? 64 : a.B), ldsBytes, stream, a);
    return srt_launch_status();
}

struct srt_resampler_stream {
    int fs_in, fs_out, C, maxBlock, B, cap;
    size_t ldsBytes;
    SrtRsFilter f;
    hipStream_t stream;
    float* d_ring;
    long long have, emitted;             // input frames received, output frames emitted
    bool ended;                          // flushed: no more input until reset
};

static int rss_fail(int code, const char* fmt, const char* detail = "") { return srt_set_error(code, fmt, detail); }
#define SRT_RSS_MAX_BLOCK (1 << 20)

int srtResampleHorizon(int fs_in, int fs_out, int table_len, int index_inc)
{
    SrtRsGeom g;
    if (const int rc = srt_rs_geometry(fs_in, fs_out, table_len != 0, table_len, index_inc, "srtResampleHorizon", &g)) return rc;
    return srt_rs_horizon(g);
}

long long srtResampleComputable(int fs_in, int fs_out, int horizon, long long n_in)
{
    if (fs_in <= 0 || fs_out <= 0 || horizon < 0 || n_in <= horizon) return 0;
    long long a = fs_in, b = fs_out;
    while (b) { const long long t = a % b; a = b; b = t; }
    const long long P = fs_in / a, Q = fs_out / a;
    return (long long)(((__int128)(n_in - horizon) * Q + P - 1) / P);
}

int srtResamplerStreamCreate(int fs_in, int fs_out, int channels, int max_block, const float* h_table, int table_len, int index_inc, void* stream,
                             srt_resampler_stream** out)
{
    const char* who = "srtResamplerStreamCreate";
    if (!out) return rss_fail(-1, "srtResamplerStreamCreate: null output pointer");
    *out = nullptr;
    SrtRsGeom g;
    if (const int rc = srt_rs_geometry(fs_in, fs_out, h_table != nullptr, table_len, index_inc, who, &g)) return rc;
    if (channels < 1 || channels > 2 * SRT_MAX_STEMS) return rss_fail(-1, "srtResamplerStreamCreate: channels must be in 1..16");
    if (max_block < 1 || max_block > SRT_RSS_MAX_BLOCK) return rss_fail(-1, "srtResamplerStreamCreate: max_block must be in 1..2^20");
    size_t lds = 0;
    const int B = srt_rsstream_block(g, &lds);
    if (!B) return rss_fail(-1, "srtResamplerStreamCreate: filter too long for this rate pair (input window above 64 KiB)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return rss_fail(-3, "srtResamplerStreamCreate: no HIP device (this library has no CPU path)");
    srt_resampler_stream* s = new (std::nothrow) srt_resampler_stream();
    if (!s) return rss_fail(-2, "srtResamplerStreamCreate: out of host memory");
    memset(s, 0, sizeof *s);
    s->fs_in = fs_in; s->fs_out = fs_out; s->C = channels; s->maxBlock = max_block; s->B = B; s->ldsBytes = lds;
    s->cap = max_block + 2 * g.LO + 1;
    s->stream = (hipStream_t)stream;
    if (const int rc = srt_rs_filter_create(g, h_table, table_len, s->stream, who, &s->f)) { delete s; return rc; }
    const size_t bytes = (size_t)s->cap * channels * sizeof(float);
    hipError_t e = hipMalloc((void**)&s->d_ring, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_ring, 0, bytes, s->stream);
    if (e != hipSuccess) { srtResamplerStreamDestroy(s); return rss_fail(-2, "srtResamplerStreamCreate: HIP error: %s", hipGetErrorString(e)); }
    *out = s;
    return 0;
}

int srtResamplerStreamDestroy(srt_resampler_stream* s)
{
    if (!s) return 0;
    hipStreamSynchronize(s->stream);                                   // a NULL stream is the null stream: wait for it alone, not for the device
    srt_rs_filter_free(&s->f);
    if (s->d_ring) hipFree(s->d_ring);
    delete s;
    return 0;
}

int srtResamplerStreamHorizon(const srt_resampler_stream* s)
{
    if (!s) return rss_fail(-1, "srtResamplerStreamHorizon: null converter");
    return srt_rs_horizon(s->f.g);
}

int srtResamplerStreamReset(srt_resampler_stream* s)
{
    if (!s) return rss_fail(-1, "srtResamplerStreamReset: null converter");
    if (hipMemsetAsync(s->d_ring, 0, (size_t)s->cap * s->C * sizeof(float), s->stream) != hipSuccess) return rss_fail(-2, "srtResamplerStreamReset: HIP error");
    s->have = s->emitted = 0; s->ended = false;
    return 0;
}

// frames [emitted, upto) from the ring and the block d_in of n frames; the block joins the ring
static int rss_emit(srt_resampler_stream* s, const float* d_in, size_t in_stride, int n, long long upto, float* d_out, size_t out_stride, const char* who)
{
    SrtRsStreamArgs a; memset(&a, 0, sizeof a);
    a.ring = s->d_ring; a.cap = s->cap; a.C = s->C;
    a.in = d_in; a.inStride = (long long)in_stride; a.have = s->have; a.n = n; a.append = n > 0;
    a.shift = 0; a.end = s->have + n;
    a.out0 = s->emitted; a.nOut = (int)(upto - s->emitted);
    a.out = d_out; a.outStride = (long long)out_stride; a.outPos = 0; a.outMask = 0x7fffffff;
    a.B = s->B;
    if (srt_rsstream_launch(s->f, a, s->ldsBytes, s->stream)) { char fmt[96]; snprintf(fmt, sizeof fmt, "%s: kernel launch failed%%s", who); return rss_fail(-2, fmt, ""); }
    s->have += n; s->emitted = upto;
    return a.nOut;
}

int srtResamplerStreamProcess(srt_resampler_stream* s, const float* d_in, size_t in_stride, int n, float* d_out, size_t out_stride)
{
    if (!s) return rss_fail(-1, "srtResamplerStreamProcess: null converter");
    if (n < 0 || n > s->maxBlock) return rss_fail(-1, "srtResamplerStreamProcess: n must be in 0..max_block");
    if (s->ended) return rss_fail(-1, "srtResamplerStreamProcess: the stream was flushed (srtResamplerStreamReset starts a new one)");
    if (n == 0) return 0;
    if (!d_in) return rss_fail(-1, "srtResamplerStreamProcess: null input");
    if (in_stride != 0 && in_stride < (size_t)n) return rss_fail(-1, "srtResamplerStreamProcess: in_stride below n (0 means interleaved)");
    const long long upto = srt_rs_computable(s->f.g, s->have + n);
    if (upto > s->emitted && (!d_out || out_stride < (size_t)(upto - s->emitted))) return rss_fail(-1, "srtResamplerStreamProcess: null output or out_stride below the frames emitted");
    return rss_emit(s, d_in, in_stride, n, upto, d_out, out_stride, "srtResamplerStreamProcess");
}

int srtResamplerStreamFlush(srt_resampler_stream* s, float* d_out, size_t out_stride)
{
    if (!s) return rss_fail(-1, "srtResamplerStreamFlush: null converter");
    if (s->ended) return 0;
    long long upto = (long long)srtResampleLength((size_t)s->have, s->fs_in, s->fs_out);
    if (upto < s->emitted) upto = s->emitted;
    if (upto > s->emitted && (!d_out || out_stride < (size_t)(upto - s->emitted))) return rss_fail(-1, "srtResamplerStreamFlush: null output or out_stride below the frames emitted");
    const int rc = rss_emit(s, nullptr, 0, 0, upto, d_out, out_stride, "srtResamplerStreamFlush");
    if (rc >= 0) s->ended = true;
    return rc;
}
