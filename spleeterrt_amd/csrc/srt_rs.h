// srt_rs.h — what the offline converter (srt_resample.hip) and the streaming one (srt_rsstream.hip) share: the geometry of a rate pair, the
// weight function and the filter object (table + per-phase weight bank in HBM).  The arithmetic is described at the top of srt_resample.hip.
#pragma once
#include "srt_internal.h"

#define SRT_RS_BANK_BYTES (8u << 20)     // per-phase weight bank limit: every common rate pair fits (96 k -> 44.1 k: 147 phases x 200 taps = 118 KB)
#define SRT_RS_LDS_BYTES  (64u << 10)    // input window staged per workgroup
#define SRT_RS_MIN_RATE 8000
#define SRT_RS_MAX_RATE 384000

struct SrtRsGeom {
    long long P, Q;          // fs_in / g, fs_out / g
    long long inc, maxIdx;   // increment, (table_len - 2) << 12
    int LO, T4;              // window = input frames [i - LO, i - LO + T4); T4 = taps padded to a multiple of 4 (zero weights)
    double fi, scale;        // float_increment, float_increment / index_inc
};

// start of the filter for phase m = n mod Q  (src_sinc.c:468: double_to_fp(input_index * float_increment))
__device__ __host__ inline long long rs_start(const SrtRsGeom& g, long long m)
{
    const double frac = (double)((m * g.P) % g.Q) / (double)g.Q;
    return (long long)rint(frac * g.fi * 4096.0);
}

// weight of window tap t (input frame i - LO + t) for a frame whose filter starts at `start`; zero where the reference takes no tap
__device__ inline float rs_weight(const SrtRsGeom& g, const float* __restrict__ table, long long start, int t)
{
#pragma clang fp contract(off)
    const long long u = (long long)t - g.LO;
    long long f;
    if (u <= 0) f = start - u * g.inc;                          // left half, src_sinc.c:375-394
    else { f = g.inc - start + (u - 1) * g.inc; if (f <= 0) return 0.0f; }   // right half, :397-412 (filter index 0 excluded)
    if (f > g.maxIdx) return 0.0f;
    const long long k = f >> 12;
    const double fr = (double)(f & 4095) * (1.0 / 4096.0);
    const double c0 = table[k], c1 = table[k + 1];
    const double w = c0 + fr * (c1 - c0);
    return (float)(g.scale * w);
}

// The filter of one rate pair on the current device: the half-filter table and, where it fits SRT_RS_BANK_BYTES, the bank [T4/4][Q][4] that
// srt_resample_bank_kernel fills from it (onfly = 1: no bank, the kernels evaluate rs_weight per tap - same floats).
struct SrtRsFilter {
    SrtRsGeom g;
    int onfly;
    float* d_table; float* d_bank;
};
// Argument checks and geometry, no HIP call: 0, or -1 with srtLastError() = "<who>: ...".  table_len / index_inc are read only with has_table
// (otherwise the built-in filter's 22 438 / 491).
int srt_rs_geometry(int fs_in, int fs_out, bool has_table, int table_len, int index_inc, const char* who, SrtRsGeom* g);
// Uploads the table (h_table NULL: the built-in filter) and builds the bank on `stream`, synchronised on return.  0, or -2 with the error set; frees
// what it allocated on failure.
int srt_rs_filter_create(const SrtRsGeom& g, const float* h_table, int table_len, hipStream_t stream, const char* who, SrtRsFilter* f);
void srt_rs_filter_free(SrtRsFilter* f);

// ---- spans form (srtResampleSpans, and both ends of srtSeparateHostStreamRate's pieces): the arguments of the public call, on any filter and stream
struct SrtRsSpans {
    int pairs;
    const float* a; size_t a_stride; long long a0; size_t a_len;
    const float* b; size_t b_stride, b_len;
    size_t n_in, out0, n_out;
    float* out; size_t out_stride;
};
// frames per workgroup, pairs per workgroup (`pairs`, or 1 with a grid dimension over the pairs) and the LDS window of one pair in frames; -1: one pair does not fit
int srt_rs_spans_shape(const SrtRsGeom& g, int pairs, int* B, int* per_wg, int* win_len);
// every check of srtResampleSpans, then one launch: 0, -1 / -2 with srtLastError() = "<who>: ..."
int srt_rs_spans_launch(const SrtRsFilter& f, const SrtRsSpans& s, hipStream_t stream, const char* who);

// ---- streaming form (srt_rsstream.hip): the same frames computed from a device ring of past input plus the call's block
// frames a stream that has received n_in input frames can compute: those whose last weighted tap floor(j P / Q) + H, H = LO + 1, has arrived
static inline int srt_rs_horizon(const SrtRsGeom& g) { return g.LO + 1; }
static inline long long srt_rs_computable(const SrtRsGeom& g, long long n_in)
{
    const long long a = n_in - srt_rs_horizon(g);
    return a <= 0 ? 0 : (long long)(((__int128)a * g.Q + g.P - 1) / g.P);
}
struct SrtRsStreamArgs {
    SrtRsGeom g; const float* table; const float4* bank;
    float* ring; int cap, C;              // [cap][C] interleaved history: input frame s >= 0 at slot s mod cap
    const float* in; long long inStride;  // the call's block, input frames [have, have + n): interleaved [n][C] (inStride 0) or channel c at in + c * inStride
    long long have; int n, append;        // append: the launch also copies the block into the ring (slots no window of this launch reads)
    long long shift, end;                 // the window of output frame j starts at input frame floor(j P / Q) - LO + shift; frames < 0 or >= end read as zero
    long long out0; int nOut;             // output frames [out0, out0 + nOut); out0 may be negative
    float* out; long long outStride;      // channel c of frame out0 + k at out[c * outStride + ((outPos + k) & outMask)]
    int outPos, outMask;
    int B;                                // frames per workgroup (<= 256, one per thread)
};
int srt_rsstream_block(const SrtRsGeom& g, size_t* ldsBytes);      // B for this rate pair and its LDS window in bytes; 0: the filter is too long
int srt_rsstream_launch(const SrtRsFilter& f, SrtRsStreamArgs a, size_t ldsBytes, hipStream_t stream);   // fills g / table / bank from f; 0 or -1
