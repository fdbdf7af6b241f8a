// srt_wiener.hip — multichannel Wiener filter over a whole call (srtSetWiener / srtIstftWiener, include/spleeterrt_amd.h).
//
// What official Spleeter runs for `spleeter separate --mwf`: norbert.wiener(v, x, iterations = n, use_softmask = True, eps = 2^-23), with
//   x_c = 4096 spec_c, v_{j,c} = m_{j,c} |x_c| (bins < F), soft-mask start y_j = v_j / (eps + sum_i v_i) x, a = max(1, max |x| / 10), then n EM
//   iterations on y^ = y / a: v_j = (|y^_L|^2 + |y^_R|^2) / 2, R_j = sum_t y^ y^H / (eps + sum_t v_j), C = sum_j v_j R_j + sqrt(eps) I,
//   y^_j <- v_j R_j C^-1 x^; the stem's spectrum is a y^_j / 4096.
// Everything here runs in spectrum units (s = x / 4096).  The algebra is scale free except for the epsilon terms, which take the scale:
//   soft mask: v / (eps / 4096 + sum v) s;   R_j = sum_t y y^H / (eps al^2 + sum_t v_j);   C = sum_j v_j R_j + sqrt(eps) al^2 I,   al = a / 4096,
// and W_j s is already the output spectrum (the a of the normalisation cancels against the final a y^).
//
// Kernels (no atomics anywhere: every sum has one fixed order, so a call is bit-reproducible run to run and under graph replay):
//   srt_wiener_stats_kernel     pass p of n: grid (256-bin blocks, row chunks); a thread owns one bin and walks the chunk's rows, re-evaluating the
//                               chain (soft mask + p - 1 iterations) from the spectrum, the masks and the earlier R tables, and keeps the four sums
//                               |y_L|^2, |y_R|^2, Re / Im y_L y_R* per stem in registers; one store per (chunk, stem, sum, bin) into the slab.
//                               Pass 1 also takes max |s| over bins 0..2048 (per-block maximum: exact, order free).
//   srt_wiener_finalize_kernel  one thread per (stem, bin): adds the chunks' partials in chunk order, divides by the regularised weight sum, writes R.
//                               Pass 1 reduces the block maxima into a first.
//   srt_wiener_filter_kernel    the chain through all n iterations per (row, bin), writing every stem's filtered spectrum (bins >= F: the input
//                               spectrum, to which the inverse transform applies oob_weight as for masks).
// The 2 x 2 inverse is the closed form with det C = c00 c11 - |c01|^2 (real); C >= sqrt(eps) al^2 I keeps it away from zero, as in norbert.
// With per-call options (overlapped tiles, the average mask extension, the stem remix: srtIstftWienerEx / srtSeparateWiener) srt_wiener_stats_ov_kernel and
// srt_wiener_filter_opt_kernel at the end of this file take the places of the first and the third; with every option off the three above run as always.
// Both families exist per track of a packed batch as well (srtSeparateBatchWiener: the plain three; srtSeparateBatchWienerEx: the option pair, at the very end).
// A host stream held one piece at a time has the statistics kernel in a segmented form (srtSeparateHostWiener: srt_wiener_stats_seg_kernel) and, on overlapped
// tiles, the option pair in forms that blend a piece's first rows with the carry of the piece before (srtSeparateHostWienerOverlap: srt_wiener_stats_seg_ov_kernel,
// srt_wiener_filter_seam_kernel).
#include "srt_internal.h"
#include "srt_overlap.h"
#include "srt_wiener_chain.h"                     // W_EPS*, w_start, w_power, w_iter: the chain at one (row, bin), shared with the live hop (srt_dsp.hip)
#include <math.h>

#define W_FILTER_ROWS 16                          // rows per workgroup of the filter

__device__ __forceinline__ float w_block_max(float x, float* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    x = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return x;
}

// The row walk of the statistics pass, rows [T0, T1) of p.spec / p.masks in row order: max |s| (pass 1) and, in band, the chain through pass - 1 iterations and the
// four sums per stem, acc += term.  A macro, not a function: srt_wiener_stats_kernel and srt_wiener_stats_seg_kernel must agree bit for bit, so both hold THIS text,
// and the first keeps the instruction stream it had when the loop stood in its body (as an inline function the same statements were scheduled differently there).
// It uses the kernel's locals p, pass, k, S, inb, tf, sstride, delta, sLp, sRp, acc and mx.
#define W_STATS_ROWS(T0, T1) \
        for (int t = (T0); t < (T1); ++t) { \
            const float2 sL = sLp[(size_t)t * SRT_SPEC_LD], sR = sRp[(size_t)t * SRT_SPEC_LD]; \
            if (pass == 1) mx = fmaxf(mx, fmaxf(hypotf(sL.x, sL.y), hypotf(sR.x, sR.y))); \
            if (!inb) continue; \
            const float* m = p.masks + (size_t)(t / p.T) * 2 * tf + (size_t)(t % p.T) * p.F + k; \
            float2 yl[SRT_MAX_STEMS], yr[SRT_MAX_STEMS]; \
            w_start(yl, yr, sL, sR, m, sstride, tf, S); \
            for (int i = 0; i < pass - 1; ++i) \
                w_iter(yl, yr, sL, sR, reinterpret_cast<const float4*>(p.rtab) + (size_t)i * S * p.F + k, p.F, delta, S); \
            _Pragma("unroll") \
            for (int j = 0; j < SRT_MAX_STEMS; ++j) { \
                acc[j][0] += yl[j].x * yl[j].x + yl[j].y * yl[j].y; \
                acc[j][1] += yr[j].x * yr[j].x + yr[j].y * yr[j].y; \
                acc[j][2] += yl[j].x * yr[j].x + yl[j].y * yr[j].y;      /* y_L conj(y_R) */ \
                acc[j][3] += yl[j].y * yr[j].x - yl[j].x * yr[j].y; \
            } \
        }

__global__ void __launch_bounds__(256) srt_wiener_stats_kernel(const SrtWienerParams p, int pass)
{
    __shared__ float red[4];
    const int k = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, S = p.nstems;
    const int r0 = c * p.rpc, r1 = min(r0 + p.rpc, p.rows);
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf;
    const float al = (pass > 1 ? p.scal[0] : 1.0f) * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    const bool inb = k < p.F, anyb = k < SRT_HALF;
    const float2* sLp = p.spec + (anyb ? k : 0);
    const float2* sRp = sLp + p.spec_ch_stride;
    float acc[SRT_MAX_STEMS][4];
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) { acc[j][0] = 0.0f; acc[j][1] = 0.0f; acc[j][2] = 0.0f; acc[j][3] = 0.0f; }
    float mx = 0.0f;
    if (anyb) {
        W_STATS_ROWS(r0, r1)
    }
    if (inb) {
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S)
#pragma unroll
                for (int q = 0; q < 4; ++q) p.slab[(((size_t)c * S + j) * 4 + q) * p.F + k] = acc[j][q];
    }
    if (pass == 1) {                                             // (block-uniform branch: every thread reaches the barriers)
        mx = w_block_max(mx, red);
        if (threadIdx.x == 0) p.slab_max[c * SRT_WIENER_BINBLK + blockIdx.x] = mx;
    }
}

// srt_wiener_stats_kernel for rows [row0, row1) of a signal of p.rows rows whose spectrum and masks are resident one PIECE at a time (srtSeparateHostWiener,
// DESIGN.md 9.3): p.spec / p.spec_ch_stride / p.masks / p.ntiles describe the piece (row row0 of the signal is row 0 of the piece), p.rows / p.rpc / p.nchunks the
// whole signal.  Grid (bin blocks, the global chunks that intersect the piece), chunk c = c0 + blockIdx.y walks [max(c rpc, row0), min((c + 1) rpc, rows, row1)).
// A chunk an earlier piece began (c rpc < row0) continues: its accumulators start from the slab slots that piece's launch stored - and in pass 1 the running
// maximum from its slab_max entry - and go back to the same slots, so after the last piece a slot holds acc += term over the chunk's rows in row order, the
// sequence the whole-signal launch runs in registers.  No atomics: one workgroup owns a (chunk, bin block) per launch, and the launches of consecutive pieces
// are ordered on the compute stream.
__global__ void __launch_bounds__(256) srt_wiener_stats_seg_kernel(const SrtWienerParams p, int row0, int row1, int c0, int pass)
{
    __shared__ float red[4];
    const int k = blockIdx.x * 256 + threadIdx.x, c = c0 + blockIdx.y, S = p.nstems;
    const int g0 = c * p.rpc;                                                    // the chunk's first row in the signal
    const int r0 = max(g0, row0) - row0, r1 = min(min(g0 + p.rpc, p.rows), row1) - row0;      // rows of the PIECE
    const bool cont = g0 < row0;                                                 // (workgroup-uniform)
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf;
    const float al = (pass > 1 ? p.scal[0] : 1.0f) * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    const bool inb = k < p.F, anyb = k < SRT_HALF;
    const float2* sLp = p.spec + (anyb ? k : 0);
    const float2* sRp = sLp + p.spec_ch_stride;
    float acc[SRT_MAX_STEMS][4];
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) { acc[j][0] = 0.0f; acc[j][1] = 0.0f; acc[j][2] = 0.0f; acc[j][3] = 0.0f; }
    if (cont && inb) {
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[j][q] = p.slab[(((size_t)c * S + j) * 4 + q) * p.F + k];
    }
    float mx = pass == 1 && cont ? p.slab_max[c * SRT_WIENER_BINBLK + blockIdx.x] : 0.0f;
    if (anyb) {
        W_STATS_ROWS(r0, r1)
    }
    if (inb) {
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S)
#pragma unroll
                for (int q = 0; q < 4; ++q) p.slab[(((size_t)c * S + j) * 4 + q) * p.F + k] = acc[j][q];
    }
    if (pass == 1) {                                             // (block-uniform branch: every thread reaches the barriers)
        mx = w_block_max(mx, red);
        if (threadIdx.x == 0) p.slab_max[c * SRT_WIENER_BINBLK + blockIdx.x] = mx;
    }
}

__global__ void __launch_bounds__(256) srt_wiener_finalize_kernel(const SrtWienerParams p, int pass)
{
    __shared__ float red[4];
    const int S = p.nstems;
    float a;
    if (pass == 1) {                                             // every block reduces the same maxima: the same a everywhere
        float mx = 0.0f;
        for (int i = threadIdx.x; i < p.nchunks * SRT_WIENER_BINBLK; i += 256) mx = fmaxf(mx, p.slab_max[i]);
        mx = w_block_max(mx, red);
        a = fmaxf(1.0f, mx * 4096.0f / 10.0f);
        if (blockIdx.x == 0 && threadIdx.x == 0) p.scal[0] = a;
    } else a = p.scal[0];
    const int idx = blockIdx.x * 256 + threadIdx.x;              // j * F + k
    if (idx >= S * p.F) return;
    const int j = idx / p.F, k = idx - j * p.F;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (int c = 0; c < p.nchunks; ++c) {                        // chunk order: the same sums every call
        const float* q = p.slab + (((size_t)c * S + j) * 4) * p.F + k;
        s0 += q[0]; s1 += q[p.F]; s2 += q[2 * (size_t)p.F]; s3 += q[3 * (size_t)p.F];
    }
    const float al = a * (1.0f / 4096.0f);
    const float w = 0.5f * (s0 + s1);
    const float inv = 1.0f / (W_EPS * al * al + w);
    const size_t o = (size_t)(pass - 1) * S * p.F + idx;
    reinterpret_cast<float4*>(p.rtab)[o] = make_float4(s0 * inv, s1 * inv, s2 * inv, s3 * inv);
    p.wsum[o] = w;
}

__global__ void __launch_bounds__(256) srt_wiener_filter_kernel(const SrtWienerParams p, int iters)
{
    const int k = blockIdx.x * 256 + threadIdx.x, S = p.nstems;
    if (k >= SRT_HALF) return;
    const int r0 = blockIdx.y * W_FILTER_ROWS, r1 = min(r0 + W_FILTER_ROWS, p.rows);
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf, och = p.out_stem / 2;
    const float al = p.scal[0] * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    const bool inb = k < p.F;
    for (int t = r0; t < r1; ++t) {
        const size_t o = (size_t)t * SRT_SPEC_LD + k;
        const float2 sL = p.spec[o], sR = p.spec[p.spec_ch_stride + o];
        if (!inb) {                                              // bins >= F: the input spectrum (oob_weight is applied by the inverse transform)
#pragma unroll
            for (int j = 0; j < SRT_MAX_STEMS; ++j)
                if (j < S) { p.out[j * p.out_stem + o] = sL; p.out[j * p.out_stem + och + o] = sR; }
            continue;
        }
        const float* m = p.masks + (size_t)(t / p.T) * 2 * tf + (size_t)(t % p.T) * p.F + k;
        float2 yl[SRT_MAX_STEMS], yr[SRT_MAX_STEMS];
        w_start(yl, yr, sL, sR, m, sstride, tf, S);
        for (int i = 0; i < iters; ++i)
            w_iter(yl, yr, sL, sR, reinterpret_cast<const float4*>(p.rtab) + (size_t)i * S * p.F + k, p.F, delta, S);
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S) { p.out[j * p.out_stem + o] = yl[j]; p.out[j * p.out_stem + och + o] = yr[j]; }
    }
}

int srt_launch_wiener_stats(const SrtWienerParams& p, int pass, hipStream_t s)
{
    if (pass < 1 || pass > SRT_WIENER_MAX_ITERS || p.nchunks < 1 || p.nchunks > SRT_WIENER_MAX_CHUNKS || p.nstems < 1 || p.nstems > SRT_MAX_STEMS ||
        p.F < 1 || p.F > SRT_HALF - 1 || (size_t)p.nchunks * p.rpc < (size_t)p.rows || (size_t)p.ntiles * p.T < (size_t)p.rows) return -1;
    const int bx = pass == 1 ? SRT_WIENER_BINBLK : (p.F + 255) / 256;      // pass 1 also covers the out-of-band bins for max |x|
    SRT_LAUNCH(srt_wiener_stats_kernel, dim3(bx, p.nchunks), dim3(256), 0, s, p, pass);
    return srt_launch_status();
}

int srt_launch_wiener_stats_seg(const SrtWienerParams& p, size_t row0, size_t nrows, int pass, hipStream_t s)
{
    if (pass < 1 || pass > SRT_WIENER_MAX_ITERS || p.nchunks < 1 || p.nchunks > SRT_WIENER_MAX_CHUNKS || p.nstems < 1 || p.nstems > SRT_MAX_STEMS ||
        p.F < 1 || p.F > SRT_HALF - 1 || p.rpc < 1 || p.rows < 1 || (size_t)p.nchunks * p.rpc < (size_t)p.rows) return -1;
    // the piece lies inside the signal, its masks and spectrum hold its rows, and every chunk it touches has a slab slot
    if (nrows < 1 || row0 + nrows > (size_t)p.rows || p.T < 1 || p.ntiles < 1 || (size_t)p.ntiles * p.T < nrows || p.spec_ch_stride < nrows * SRT_SPEC_LD) return -1;
    const int c0 = (int)(row0 / p.rpc), c1 = (int)((row0 + nrows - 1) / p.rpc);
    if (c1 >= p.nchunks) return -1;
    const int bx = pass == 1 ? SRT_WIENER_BINBLK : (p.F + 255) / 256;      // pass 1 also covers the out-of-band bins for max |x|
    SRT_LAUNCH(srt_wiener_stats_seg_kernel, dim3(bx, c1 - c0 + 1), dim3(256), 0, s, p, (int)row0, (int)(row0 + nrows), c0, pass);
    return srt_launch_status();
}

int srt_launch_wiener_finalize(const SrtWienerParams& p, int pass, hipStream_t s)
{
    if (pass < 1 || pass > SRT_WIENER_MAX_ITERS) return -1;
    SRT_LAUNCH(srt_wiener_finalize_kernel, dim3((p.nstems * p.F + 255) / 256), dim3(256), 0, s, p, pass);
    return srt_launch_status();
}

int srt_launch_wiener_filter(const SrtWienerParams& p, int iters, hipStream_t s)
{
    if (iters < 1 || iters > SRT_WIENER_MAX_ITERS || p.rows < 1 || (size_t)p.ntiles * p.T < (size_t)p.rows || p.out_stem != 2 * (size_t)p.rows * SRT_SPEC_LD) return -1;
    SRT_LAUNCH(srt_wiener_filter_kernel, dim3(SRT_WIENER_BINBLK, (p.rows + W_FILTER_ROWS - 1) / W_FILTER_ROWS), dim3(256), 0, s, p, iters);
    return srt_launch_status();
}

// ------------------------------------------------------------------------------------------- per track of a packed batch (srtSeparateBatchWiener)
// The three kernels above with "the call" replaced by "the track": a track's statistics window is its own rows [0, rows_k) - not the rows that pad it to its
// tile boundary, not another track - its a is the maximum over those rows, and its chunks follow wiener_issue's rule on rows_k.  The per-row arithmetic
// (w_start / w_iter), the accumulation statements and the order of every sum are the ones above, so track k's R tables, weight sums and a are the
// single-signal launches' on that track alone, bit for bit, whatever else the batch holds and wherever the track sits in it.
// Chunks are numbered through the call (track k: [chunk0, chunk0 + nchunks)); slab and slab_max are indexed by that number, the tables by track.

// the track of global chunk c: the last k with chunk0(k) <= c.  c is workgroup-uniform, so every probe is a uniform (scalar) load, as in srt_batch_track
__device__ __forceinline__ int w_chunk_track(const SrtBatchWiener* __restrict__ w, int ntracks, int c)
{
    int lo = 0, hi = ntracks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (w[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// the track of packed tile `tile`: the last k with tile0(k) <= tile
__device__ __forceinline__ int w_tile_track(const SrtBatchTrack* __restrict__ t, int ntracks, int tile)
{
    int lo = 0, hi = ntracks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256) srt_wiener_stats_batch_kernel(const SrtWienerParams p, const SrtBatchTrack* __restrict__ tracks,
                                                                     const SrtBatchWiener* __restrict__ wt, int ntracks, int pass)
{
    __shared__ float red[4];
    const int k = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, S = p.nstems;
    const int trk = w_chunk_track(wt, ntracks, c);
    const SrtBatchWiener g = wt[trk];
    const int rows = tracks[trk].rows, tile0 = tracks[trk].tile0;
    const int r0 = (c - g.chunk0) * g.rpc, r1 = min(r0 + g.rpc, rows);           // rows of the TRACK
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf;
    const float* scal = p.scal + g.tab;
    const float4* rtab = reinterpret_cast<const float4*>(p.rtab) + (size_t)g.tab * SRT_WIENER_MAX_ITERS * S * p.F;
    const float al = (pass > 1 ? scal[0] : 1.0f) * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    const bool inb = k < p.F, anyb = k < SRT_HALF;
    const float2* sLp = p.spec + (size_t)tile0 * p.T * SRT_SPEC_LD + (anyb ? k : 0);       // the track's first packed row
    const float2* sRp = sLp + p.spec_ch_stride;
    const float* masks = p.masks + (size_t)tile0 * 2 * tf;                                 // ... and first packed tile
    float acc[SRT_MAX_STEMS][4];
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) { acc[j][0] = 0.0f; acc[j][1] = 0.0f; acc[j][2] = 0.0f; acc[j][3] = 0.0f; }
    float mx = 0.0f;
    if (anyb) {
        for (int t = r0; t < r1; ++t) {
            const float2 sL = sLp[(size_t)t * SRT_SPEC_LD], sR = sRp[(size_t)t * SRT_SPEC_LD];
            if (pass == 1) mx = fmaxf(mx, fmaxf(hypotf(sL.x, sL.y), hypotf(sR.x, sR.y)));
            if (!inb) continue;
            const float* m = masks + (size_t)(t / p.T) * 2 * tf + (size_t)(t % p.T) * p.F + k;
            float2 yl[SRT_MAX_STEMS], yr[SRT_MAX_STEMS];
            w_start(yl, yr, sL, sR, m, sstride, tf, S);
            for (int i = 0; i < pass - 1; ++i)
                w_iter(yl, yr, sL, sR, rtab + (size_t)i * S * p.F + k, p.F, delta, S);
#pragma unroll
            for (int j = 0; j < SRT_MAX_STEMS; ++j) {
                acc[j][0] += yl[j].x * yl[j].x + yl[j].y * yl[j].y;
                acc[j][1] += yr[j].x * yr[j].x + yr[j].y * yr[j].y;
                acc[j][2] += yl[j].x * yr[j].x + yl[j].y * yr[j].y;      // y_L conj(y_R)
                acc[j][3] += yl[j].y * yr[j].x - yl[j].x * yr[j].y;
            }
        }
    }
    if (inb) {
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S)
#pragma unroll
                for (int q = 0; q < 4; ++q) p.slab[(((size_t)c * S + j) * 4 + q) * p.F + k] = acc[j][q];
    }
    if (pass == 1) {                                             // (block-uniform branch: every thread reaches the barriers)
        mx = w_block_max(mx, red);
        if (threadIdx.x == 0) p.slab_max[c * SRT_WIENER_BINBLK + blockIdx.x] = mx;
    }
}

// grid (ceil(S F / 256), ntracks): blockIdx.y is the track
__global__ void __launch_bounds__(256) srt_wiener_finalize_batch_kernel(const SrtWienerParams p, const SrtBatchWiener* __restrict__ wt, int pass)
{
    __shared__ float red[4];
    const int S = p.nstems;
    const SrtBatchWiener g = wt[blockIdx.y];
    float* scal = p.scal + g.tab;
    float a;
    if (pass == 1) {                                             // every block of a track reduces the track's maxima: the same a everywhere
        float mx = 0.0f;
        const float* smax = p.slab_max + (size_t)g.chunk0 * SRT_WIENER_BINBLK;
        for (int i = threadIdx.x; i < g.nchunks * SRT_WIENER_BINBLK; i += 256) mx = fmaxf(mx, smax[i]);
        mx = w_block_max(mx, red);
        a = fmaxf(1.0f, mx * 4096.0f / 10.0f);
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[0] = a;
    } else a = scal[0];
    const int idx = blockIdx.x * 256 + threadIdx.x;              // j * F + k
    if (idx >= S * p.F) return;
    const int j = idx / p.F, k = idx - j * p.F;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (int c = g.chunk0; c < g.chunk0 + g.nchunks; ++c) {      // the track's chunks in chunk order: the same sums every call
        const float* q = p.slab + (((size_t)c * S + j) * 4) * p.F + k;
        s0 += q[0]; s1 += q[p.F]; s2 += q[2 * (size_t)p.F]; s3 += q[3 * (size_t)p.F];
    }
    const float al = a * (1.0f / 4096.0f);
    const float w = 0.5f * (s0 + s1);
    const float inv = 1.0f / (W_EPS * al * al + w);
    const size_t o = ((size_t)g.tab * SRT_WIENER_MAX_ITERS + (pass - 1)) * S * p.F + idx;
    reinterpret_cast<float4*>(p.rtab)[o] = make_float4(s0 * inv, s1 * inv, s2 * inv, s3 * inv);
    p.wsum[o] = w;
}

// blocks of W_FILTER_ROWS packed rows: T is a multiple of 64, so a block lies in one tile, hence in one track; rows at or past the track's own are skipped
// (the batched inverse never reads them)
__global__ void __launch_bounds__(256) srt_wiener_filter_batch_kernel(const SrtWienerParams p, const SrtBatchTrack* __restrict__ tracks,
                                                                      const SrtBatchWiener* __restrict__ wt, int ntracks, int iters)
{
    const int k = blockIdx.x * 256 + threadIdx.x, S = p.nstems;
    if (k >= SRT_HALF) return;
    const int r0 = blockIdx.y * W_FILTER_ROWS;                                   // packed rows
    const int trk = w_tile_track(tracks, ntracks, r0 / p.T);
    const int tab = wt[trk].tab;
    const int r1 = min(r0 + W_FILTER_ROWS, tracks[trk].tile0 * p.T + tracks[trk].rows);
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf, och = p.out_stem / 2;
    const float4* rtab = reinterpret_cast<const float4*>(p.rtab) + (size_t)tab * SRT_WIENER_MAX_ITERS * S * p.F;
    const float al = p.scal[tab] * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    const bool inb = k < p.F;
    for (int t = r0; t < r1; ++t) {
        const size_t o = (size_t)t * SRT_SPEC_LD + k;
        const float2 sL = p.spec[o], sR = p.spec[p.spec_ch_stride + o];
        if (!inb) {                                              // bins >= F: the input spectrum (oob_weight is applied by the inverse transform)
#pragma unroll
            for (int j = 0; j < SRT_MAX_STEMS; ++j)
                if (j < S) { p.out[j * p.out_stem + o] = sL; p.out[j * p.out_stem + och + o] = sR; }
            continue;
        }
        const float* m = p.masks + (size_t)(t / p.T) * 2 * tf + (size_t)(t % p.T) * p.F + k;      // packed tile = the track's first + the tile within it
        float2 yl[SRT_MAX_STEMS], yr[SRT_MAX_STEMS];
        w_start(yl, yr, sL, sR, m, sstride, tf, S);
        for (int i = 0; i < iters; ++i)
            w_iter(yl, yr, sL, sR, rtab + (size_t)i * S * p.F + k, p.F, delta, S);
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S) { p.out[j * p.out_stem + o] = yl[j]; p.out[j * p.out_stem + och + o] = yr[j]; }
    }
}

int srt_batch_wiener_geometry(const SrtBatchTrack* t, SrtBatchWiener* w, int ntracks)
{
    long c = 0;
    for (int k = 0; k < ntracks; ++k) {
        const int rows = t[k].rows;
        if (rows < 1) return -1;
        int nch = (rows + 15) / 16; if (nch > SRT_WIENER_MAX_CHUNKS) nch = SRT_WIENER_MAX_CHUNKS;     // wiener_issue's rule on the track's rows
        w[k].rpc = (rows + nch - 1) / nch; w[k].nchunks = (rows + w[k].rpc - 1) / w[k].rpc;
        w[k].chunk0 = (int)c; w[k].tab = k;
        c += w[k].nchunks;
        if (c > 65535) return -1;                                // the statistics grid's y extent
    }
    return (int)c;
}

static bool w_batch_args_ok(const SrtWienerParams& p, int ntracks)
{
    return ntracks >= 1 && ntracks <= p.ntiles && p.nstems >= 1 && p.nstems <= SRT_MAX_STEMS && p.F >= 1 && p.F <= SRT_HALF - 1 && p.T >= W_FILTER_ROWS &&
           p.T % W_FILTER_ROWS == 0 && p.rows == p.ntiles * p.T && p.nchunks >= ntracks && p.nchunks <= 65535;
}

int srt_launch_wiener_stats_batch(const SrtWienerParams& p, const SrtBatchTrack* d_tracks, const SrtBatchWiener* d_wt, int ntracks, int pass, hipStream_t s)
{
    if (pass < 1 || pass > SRT_WIENER_MAX_ITERS || !w_batch_args_ok(p, ntracks)) return -1;
    const int bx = pass == 1 ? SRT_WIENER_BINBLK : (p.F + 255) / 256;      // pass 1 also covers the out-of-band bins for max |x|
    SRT_LAUNCH(srt_wiener_stats_batch_kernel, dim3(bx, p.nchunks), dim3(256), 0, s, p, d_tracks, d_wt, ntracks, pass);
    return srt_launch_status();
}

int srt_launch_wiener_finalize_batch(const SrtWienerParams& p, const SrtBatchWiener* d_wt, int ntracks, int pass, hipStream_t s)
{
    if (pass < 1 || pass > SRT_WIENER_MAX_ITERS || !w_batch_args_ok(p, ntracks) || ntracks > 65535) return -1;
    SRT_LAUNCH(srt_wiener_finalize_batch_kernel, dim3((p.nstems * p.F + 255) / 256, ntracks), dim3(256), 0, s, p, d_wt, pass);
    return srt_launch_status();
}

int srt_launch_wiener_filter_batch(const SrtWienerParams& p, const SrtBatchTrack* d_tracks, const SrtBatchWiener* d_wt, int ntracks, int iters, hipStream_t s)
{
    if (iters < 1 || iters > SRT_WIENER_MAX_ITERS || !w_batch_args_ok(p, ntracks) || p.rows / W_FILTER_ROWS > 65535 || p.out_stem != 2 * (size_t)p.rows * SRT_SPEC_LD) return -1;
    SRT_LAUNCH(srt_wiener_filter_batch_kernel, dim3(SRT_WIENER_BINBLK, p.rows / W_FILTER_ROWS), dim3(256), 0, s, p, d_tracks, d_wt, ntracks, iters);
    return srt_launch_status();
}

// ------------------------------------------------------------------------------------------- per-call options (srtIstftWienerEx / srtSeparateWiener)
// Overlapped tiles, the average mask extension and the stem remix under the filter.  The kernels above are not touched: with every option off the entry
// points launch them as always.  An overlap changes the one thing the filter reads of the network - the mask value of a (stem, row, channel, bin) becomes
// the cross-faded value of the row's two tiles (srt_ov_row / srt_blend, srt_overlap.h: the inverse transform's own helpers) - and nothing else: a spectrum
// row enters the statistics once however many tiles hold it, and the window, a, the row chunks and the order of every sum stay wiener_issue's.

// w_start on mask VALUES (already fetched, and blended where the row lies in two tiles) instead of a mask pointer: the same statements in the same order
__device__ __forceinline__ void w_start_v(float2 (&yl)[SRT_MAX_STEMS], float2 (&yr)[SRT_MAX_STEMS], float2 sL, float2 sR,
                                          const float (&ml)[SRT_MAX_STEMS], const float (&mr)[SRT_MAX_STEMS], int S)
{
    const float aL = hypotf(sL.x, sL.y), aR = hypotf(sR.x, sR.y);
    float vl[SRT_MAX_STEMS], vr[SRT_MAX_STEMS], suml = 0.0f, sumr = 0.0f;
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) {
        vl[j] = 0.0f; vr[j] = 0.0f;
        if (j < S) { vl[j] = ml[j] * aL; vr[j] = mr[j] * aR; suml += vl[j]; sumr += vr[j]; }
    }
    const float il = 1.0f / (W_EPS_SOFT + suml), ir = 1.0f / (W_EPS_SOFT + sumr);
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) {
        const float gl = vl[j] * il, gr = vr[j] * ir;
        yl[j] = make_float2(gl * sL.x, gl * sL.y);
        yr[j] = make_float2(gr * sR.x, gr * sR.y);
    }
}

// the mask values of row t, bin k in the overlapped layout: the row's primary tile, cross-faded with row k + S of the previous tile inside an overlap.
// t is workgroup-uniform (a loop counter from blockIdx), so srt_ov_row is scalar arithmetic and `two` a uniform branch: the second row is loaded only then.
__device__ __forceinline__ void w_masks_ov(float (&ml)[SRT_MAX_STEMS], float (&mr)[SRT_MAX_STEMS], const SrtWienerParams& p, int O, int t, int k, int S)
{
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf;
    const OvRow ov = srt_ov_row(t, p.T, O, p.ntiles);
    const float* b = p.masks + (size_t)ov.j1 * 2 * tf + (size_t)ov.k * p.F + k;
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) {
        ml[j] = 0.0f; mr[j] = 0.0f;
        if (j < S) { ml[j] = b[j * sstride]; mr[j] = b[j * sstride + tf]; }
    }
    if (ov.two) {
        const float* a = b - 2 * tf + (size_t)(p.T - O) * p.F;
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S) { ml[j] = srt_blend(a[j * sstride], ml[j], ov.w); mr[j] = srt_blend(a[j * sstride + tf], mr[j], ov.w); }
    }
}

// A piece of a longer stream (srtSeparateHostWienerOverlap): after w_masks_ov on the piece's own tiles, rows [0, O) of its first tile (srt_ov_seam)
// blend with the mask seam carry [nstems][2][O][F] the previous piece left (srt_mask_seam_save_kernel) - a = carry[stem][channel][k], b = the row's own value, the
// same w and the same srt_blend as inside one signal.  seam = nullptr (the stream's first piece) or any other row: nothing happens.  t is workgroup-uniform.
__device__ __forceinline__ void w_masks_seam(float (&ml)[SRT_MAX_STEMS], float (&mr)[SRT_MAX_STEMS], const SrtWienerParams& p, int O, const float* __restrict__ seam, int t, int k, int S)
{
    const OvRow ov = srt_ov_row(t, p.T, O, p.ntiles);
    if (!srt_ov_seam(ov, O, seam)) return;
    const size_t a_ch = (size_t)O * p.F, a_stem = 2 * a_ch;
    const float* a = seam + (size_t)ov.k * p.F + k;
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j)
        if (j < S) { ml[j] = srt_blend(a[j * a_stem], ml[j], ov.w); mr[j] = srt_blend(a[j * a_stem + a_ch], mr[j], ov.w); }
}

// W_STATS_ROWS on blended masks: the mask fetch is w_masks_ov, then SEAM_STMT (empty inside one signal; the seam blend of a piece), and the chain runs through
// w_start_v / w_iter<true>.  A macro for the reason given at W_STATS_ROWS: srt_wiener_stats_ov_kernel and srt_wiener_stats_seg_ov_kernel must agree bit for bit, so
// both hold THIS text.  It uses the kernel's locals p, O, pass, k, S, inb, delta, sLp, sRp, acc and mx.
#define W_STATS_ROWS_OV(T0, T1, SEAM_STMT) \
        for (int t = (T0); t < (T1); ++t) { \
            const float2 sL = sLp[(size_t)t * SRT_SPEC_LD], sR = sRp[(size_t)t * SRT_SPEC_LD]; \
            if (pass == 1) mx = fmaxf(mx, fmaxf(hypotf(sL.x, sL.y), hypotf(sR.x, sR.y))); \
            if (!inb) continue; \
            float ml[SRT_MAX_STEMS], mr[SRT_MAX_STEMS]; \
            w_masks_ov(ml, mr, p, O, t, k, S); \
            SEAM_STMT \
            float2 yl[SRT_MAX_STEMS], yr[SRT_MAX_STEMS]; \
            w_start_v(yl, yr, sL, sR, ml, mr, S); \
            for (int i = 0; i < pass - 1; ++i) \
                w_iter<true>(yl, yr, sL, sR, reinterpret_cast<const float4*>(p.rtab) + (size_t)i * S * p.F + k, p.F, delta, S); \
            _Pragma("unroll") \
            for (int j = 0; j < SRT_MAX_STEMS; ++j) { \
                acc[j][0] += yl[j].x * yl[j].x + yl[j].y * yl[j].y; \
                acc[j][1] += yr[j].x * yr[j].x + yr[j].y * yr[j].y; \
                acc[j][2] += yl[j].x * yr[j].x + yl[j].y * yr[j].y;      /* y_L conj(y_R) */ \
                acc[j][3] += yl[j].y * yr[j].x - yl[j].x * yr[j].y; \
            } \
        }

// srt_wiener_stats_kernel with the mask fetch replaced (launched only with an overlap: at O = 0 that kernel runs, and the R tables are its own bit for bit)
__global__ void __launch_bounds__(256) srt_wiener_stats_ov_kernel(const SrtWienerParams p, int O, int pass)
{
    __shared__ float red[4];
    const int k = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, S = p.nstems;
    const int r0 = c * p.rpc, r1 = min(r0 + p.rpc, p.rows);
    const float al = (pass > 1 ? p.scal[0] : 1.0f) * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    const bool inb = k < p.F, anyb = k < SRT_HALF;
    const float2* sLp = p.spec + (anyb ? k : 0);
    const float2* sRp = sLp + p.spec_ch_stride;
    float acc[SRT_MAX_STEMS][4];
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) { acc[j][0] = 0.0f; acc[j][1] = 0.0f; acc[j][2] = 0.0f; acc[j][3] = 0.0f; }
    float mx = 0.0f;
    if (anyb) {
        W_STATS_ROWS_OV(r0, r1, )
    }
    if (inb) {
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S)
#pragma unroll
                for (int q = 0; q < 4; ++q) p.slab[(((size_t)c * S + j) * 4 + q) * p.F + k] = acc[j][q];
    }
    if (pass == 1) {                                             // (block-uniform branch: every thread reaches the barriers)
        mx = w_block_max(mx, red);
        if (threadIdx.x == 0) p.slab_max[c * SRT_WIENER_BINBLK + blockIdx.x] = mx;
    }
}

// srt_wiener_stats_seg_kernel on the overlapped tiles of a PIECE (srtSeparateHostWienerOverlap): rows [row0, row1) of a signal of p.rows rows are the
// rows the piece OWNS, the first of the rows its p.ntiles tiles cover (p.spec / p.spec_ch_stride / p.masks / p.ntiles describe the piece; row row0 of the signal is
// its row 0).  The chunks, the continuation from and back into the slab and the ordering argument are srt_wiener_stats_seg_kernel's; the mask fetch is
// srt_wiener_stats_ov_kernel's on piece-local rows, with the seam rule (w_masks_seam) for the first O rows of a later piece.  No atomics.
__global__ void __launch_bounds__(256) srt_wiener_stats_seg_ov_kernel(const SrtWienerParams p, int O, const float* __restrict__ seam, int row0, int row1, int c0, int pass)
{
    __shared__ float red[4];
    const int k = blockIdx.x * 256 + threadIdx.x, c = c0 + blockIdx.y, S = p.nstems;
    const int g0 = c * p.rpc;                                                    // the chunk's first row in the signal
    const int r0 = max(g0, row0) - row0, r1 = min(min(g0 + p.rpc, p.rows), row1) - row0;      // rows of the PIECE
    const bool cont = g0 < row0;                                                 // (workgroup-uniform)
    const float al = (pass > 1 ? p.scal[0] : 1.0f) * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    const bool inb = k < p.F, anyb = k < SRT_HALF;
    const float2* sLp = p.spec + (anyb ? k : 0);
    const float2* sRp = sLp + p.spec_ch_stride;
    float acc[SRT_MAX_STEMS][4];
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) { acc[j][0] = 0.0f; acc[j][1] = 0.0f; acc[j][2] = 0.0f; acc[j][3] = 0.0f; }
    if (cont && inb) {
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[j][q] = p.slab[(((size_t)c * S + j) * 4 + q) * p.F + k];
    }
    float mx = pass == 1 && cont ? p.slab_max[c * SRT_WIENER_BINBLK + blockIdx.x] : 0.0f;
    if (anyb) {
        W_STATS_ROWS_OV(r0, r1, w_masks_seam(ml, mr, p, O, seam, t, k, S);)
    }
    if (inb) {
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S)
#pragma unroll
                for (int q = 0; q < 4; ++q) p.slab[(((size_t)c * S + j) * 4 + q) * p.F + k] = acc[j][q];
    }
    if (pass == 1) {                                             // (block-uniform branch: every thread reaches the barriers)
        mx = w_block_max(mx, red);
        if (threadIdx.x == 0) p.slab_max[c * SRT_WIENER_BINBLK + blockIdx.x] = mx;
    }
}

// The remix of the filter's outputs (srt_mix_gains' / srt_mix_chain's arithmetic on filtered values): one rounded product and one fused multiply-add per stem,
// nothing else contracted, so a one-hot row gives stem m's bits.  The matrix is read from the launch arguments where it is used (m is a uniform loop counter).
#pragma clang fp contract(off)
// in band, per complex component: h = G[m][S] s, then h = fmaf(G[m][j], y_j, h) for j ascending
__device__ __forceinline__ float2 w_mix_inband(const SrtWienerOpt& q, int m, int S, float2 s, const float2 (&y)[SRT_MAX_STEMS])
{
    const float g = q.mix[m][S];
    float hx = g * s.x, hy = g * s.y;
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j)
        if (j < S) { const float gj = q.mix[m][j]; hx = fmaf(gj, y[j].x, hx); hy = fmaf(gj, y[j].y, hy); }
    return make_float2(hx, hy);
}
// above F: the gain h = G[m][S], then h = fmaf(G[m][j], g_j, h) for j ascending (g_j: stem j's gain of this row and channel)
__device__ __forceinline__ float w_mix_gain(const SrtWienerOpt& q, int m, int S, const float (&g)[SRT_MAX_STEMS])
{
    float h = q.mix[m][S];
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j)
        if (j < S) h = fmaf(q.mix[m][j], g[j], h);
    return h;
}
__device__ __forceinline__ float2 w_scale(float g, float2 s) { return make_float2(g * s.x, g * s.y); }
#pragma clang fp contract(fast)

// srt_wiener_filter_kernel for a call with any option on: one thread per bin, W_FILTER_ROWS rows per workgroup.  It writes the FINAL spectrum of every bin -
// in band y_j (or, with a remix, the mixes of the y_j); above F the gain times the input, the gain being oob[j], the extension table's e_j(row, channel) (q.ext, a
// run-time pointer; the address is workgroup-uniform: scalar loads) or, with a remix, their chain through the matrix - so the inverse transform behind it applies no
// gain at all.  OV: the masks are in the overlapped layout (w_masks_ov); else they are fetched as srt_wiener_filter_kernel does.
// The remix is a RUN-TIME branch (q.n_out, workgroup-uniform), not a second instantiation: a one-hot row must give the bits of the stem, and that holds by
// construction only when the mixes and the stems come out of one compiled copy of the chain - compiled apart, the two copies differed in which products and sums
// became fused multiply-adds, and the y_j in their last bits.
// The body is a macro for the reason given at W_STATS_ROWS: srt_wiener_filter_opt_kernel keeps the instruction stream it had when these statements stood in it, and
// the seam kernel below holds the same text.  OVC: the masks are in the overlapped layout; SEAM_STMT: empty, or the seam blend of a piece's first O rows (w_masks_seam).
// It uses the kernel's arguments p, q and iters.
#define W_FILTER_OPT_ROWS(OVC, SEAM_STMT) \
    const int k = blockIdx.x * 256 + threadIdx.x, S = p.nstems; \
    if (k >= SRT_HALF) return; \
    const int r0 = blockIdx.y * W_FILTER_ROWS, r1 = min(r0 + W_FILTER_ROWS, p.rows); \
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf, och = p.out_stem / 2; \
    const float al = p.scal[0] * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al; \
    const bool inb = k < p.F; \
    for (int t = r0; t < r1; ++t) { \
        const size_t o = (size_t)t * SRT_SPEC_LD + k; \
        const float2 sL = p.spec[o], sR = p.spec[p.spec_ch_stride + o]; \
        if (!inb) { \
            float gl[SRT_MAX_STEMS], gr[SRT_MAX_STEMS]; \
            _Pragma("unroll") \
            for (int j = 0; j < SRT_MAX_STEMS; ++j) { \
                gl[j] = 0.0f; gr[j] = 0.0f; \
                if (j < S) { \
                    if (q.ext) { const float* e = q.ext + (size_t)j * q.ext_stem + (size_t)t * 2; gl[j] = e[0]; gr[j] = e[1]; } \
                    else { gl[j] = q.oob[j]; gr[j] = gl[j]; } \
                } \
            } \
            if (q.n_out) { \
                for (int m = 0; m < q.n_out; ++m) { \
                    p.out[m * p.out_stem + o] = w_scale(w_mix_gain(q, m, S, gl), sL); \
                    p.out[m * p.out_stem + och + o] = w_scale(w_mix_gain(q, m, S, gr), sR); \
                } \
            } else { \
            _Pragma("unroll") \
                for (int j = 0; j < SRT_MAX_STEMS; ++j) \
                    if (j < S) { p.out[j * p.out_stem + o] = w_scale(gl[j], sL); p.out[j * p.out_stem + och + o] = w_scale(gr[j], sR); } \
            } \
            continue; \
        } \
        float2 yl[SRT_MAX_STEMS], yr[SRT_MAX_STEMS]; \
        if constexpr (OVC) { \
            float ml[SRT_MAX_STEMS], mr[SRT_MAX_STEMS]; \
            w_masks_ov(ml, mr, p, q.overlap, t, k, S); \
            SEAM_STMT \
            w_start_v(yl, yr, sL, sR, ml, mr, S); \
        } else { \
            const float* m = p.masks + (size_t)(t / p.T) * 2 * tf + (size_t)(t % p.T) * p.F + k; \
            w_start(yl, yr, sL, sR, m, sstride, tf, S); \
        } \
        for (int i = 0; i < iters; ++i) \
            w_iter<true>(yl, yr, sL, sR, reinterpret_cast<const float4*>(p.rtab) + (size_t)i * S * p.F + k, p.F, delta, S); \
        if (q.n_out) { \
            for (int m = 0; m < q.n_out; ++m) { \
                p.out[m * p.out_stem + o] = w_mix_inband(q, m, S, sL, yl); \
                p.out[m * p.out_stem + och + o] = w_mix_inband(q, m, S, sR, yr); \
            } \
        } else { \
            _Pragma("unroll") \
            for (int j = 0; j < SRT_MAX_STEMS; ++j) \
                if (j < S) { p.out[j * p.out_stem + o] = yl[j]; p.out[j * p.out_stem + och + o] = yr[j]; } \
        } \
    }
template <bool OV>
__global__ void __launch_bounds__(256) srt_wiener_filter_opt_kernel(const SrtWienerParams p, const SrtWienerOpt q, int iters)
{
    W_FILTER_OPT_ROWS(OV, )
}
// the overlapped form over the rows a piece of a longer stream owns (srtSeparateHostWienerOverlap): p.rows = those rows, p.ntiles the piece's tiles,
// p.spec_ch_stride the rows its spectrum holds, `seam` the carry its first O rows blend with
__global__ void __launch_bounds__(256) srt_wiener_filter_seam_kernel(const SrtWienerParams p, const SrtWienerOpt q, int iters, const float* __restrict__ seam)
{
    W_FILTER_OPT_ROWS(true, w_masks_seam(ml, mr, p, q.overlap, seam, t, k, S);)
}

// masks of p.ntiles tiles at this overlap cover rows 0 .. p.rows - 1 (srt_ov_row then stays inside the masks: row k < T of tile j1 < ntiles, and k + S < T of tile j1 - 1)
static bool w_layout_ok(const SrtWienerParams& p, int overlap)
{
    if (p.T < 1 || p.ntiles < 1 || overlap < 0 || overlap > p.T / 2) return false;
    return (size_t)(p.ntiles - 1) * (p.T - overlap) + p.T >= (size_t)p.rows;
}

int srt_launch_wiener_stats_ov(const SrtWienerParams& p, int overlap, int pass, hipStream_t s)
{
    if (pass < 1 || pass > SRT_WIENER_MAX_ITERS || p.nchunks < 1 || p.nchunks > SRT_WIENER_MAX_CHUNKS || p.nstems < 1 || p.nstems > SRT_MAX_STEMS ||
        p.F < 1 || p.F > SRT_HALF - 1 || (size_t)p.nchunks * p.rpc < (size_t)p.rows || overlap < 1 || !w_layout_ok(p, overlap)) return -1;
    const int bx = pass == 1 ? SRT_WIENER_BINBLK : (p.F + 255) / 256;      // pass 1 also covers the out-of-band bins for max |x|
    SRT_LAUNCH(srt_wiener_stats_ov_kernel, dim3(bx, p.nchunks), dim3(256), 0, s, p, overlap, pass);
    return srt_launch_status();
}

int srt_launch_wiener_stats_seg_ov(const SrtWienerParams& p, int overlap, const float* seam, size_t row0, size_t nrows, int pass, hipStream_t s)
{
    if (pass < 1 || pass > SRT_WIENER_MAX_ITERS || p.nchunks < 1 || p.nchunks > SRT_WIENER_MAX_CHUNKS || p.nstems < 1 || p.nstems > SRT_MAX_STEMS ||
        p.F < 1 || p.F > SRT_HALF - 1 || p.rpc < 1 || p.rows < 1 || (size_t)p.nchunks * p.rpc < (size_t)p.rows || overlap < 1) return -1;
    // the piece's owned rows lie inside the signal, its tiles at this overlap cover them and its spectrum holds them, and every chunk it touches has a slab slot
    if (nrows < 1 || row0 + nrows > (size_t)p.rows || p.T < 1 || p.ntiles < 1 || overlap > p.T / 2 || (size_t)(p.ntiles - 1) * (p.T - overlap) + p.T < nrows ||
        p.spec_ch_stride < nrows * SRT_SPEC_LD) return -1;
    const int c0 = (int)(row0 / p.rpc), c1 = (int)((row0 + nrows - 1) / p.rpc);
    if (c1 >= p.nchunks) return -1;
    const int bx = pass == 1 ? SRT_WIENER_BINBLK : (p.F + 255) / 256;      // pass 1 also covers the out-of-band bins for max |x|
    SRT_LAUNCH(srt_wiener_stats_seg_ov_kernel, dim3(bx, c1 - c0 + 1), dim3(256), 0, s, p, overlap, seam, (int)row0, (int)(row0 + nrows), c0, pass);
    return srt_launch_status();
}

int srt_launch_wiener_filter_opt(const SrtWienerParams& p, const SrtWienerOpt& q, int iters, hipStream_t s, const float* seam)
{
    if (iters < 1 || iters > SRT_WIENER_MAX_ITERS || p.rows < 1 || p.nstems < 1 || p.nstems > SRT_MAX_STEMS || p.F < 1 || p.F > SRT_HALF - 1 ||
        !w_layout_ok(p, q.overlap) || p.out_stem != 2 * (size_t)p.rows * SRT_SPEC_LD || p.spec_ch_stride < (size_t)p.rows * SRT_SPEC_LD) return -1;
    if (q.n_out < 0 || q.n_out > p.nstems || (q.ext && q.ext_stem < (size_t)p.rows * 2)) return -1;      // the spectrum workspace holds nstems spectra
    const dim3 grid(SRT_WIENER_BINBLK, (p.rows + W_FILTER_ROWS - 1) / W_FILTER_ROWS), block(256);
    if (seam) {                                          // a later piece of a longer stream
        if (q.overlap <= 0) return -1;
        SRT_LAUNCH(srt_wiener_filter_seam_kernel, grid, block, 0, s, p, q, iters, seam);
    } else if (q.overlap > 0) SRT_LAUNCH(srt_wiener_filter_opt_kernel<true>, grid, block, 0, s, p, q, iters);
    else SRT_LAUNCH(srt_wiener_filter_opt_kernel<false>, grid, block, 0, s, p, q, iters);
    return srt_launch_status();
}

// ------------------------------------------------------------------------------------------- per-call options per track of a packed batch (srtSeparateBatchWienerEx)
// The two option kernels above with "the call" replaced by "the track", as the batch kernels replace it in the plain ones: the in-track row walks the track's own
// rows, srt_ov_row is clamped by the track's own tile count (a blend partner is a tile of the same track), the mask base is the track's first packed tile and
// the stem stride the packed tile count.  Statistics, tables and a are indexed as in srt_wiener_stats_batch_kernel; finalize is srt_wiener_finalize_batch_kernel.

// w_masks_ov with the stem stride and the clamp apart (there both come from p.ntiles): `masks` is the first tile of the view, `ntiles` the view's tile count;
// the same statements in the same order
__device__ __forceinline__ void w_masks_ov_view(float (&ml)[SRT_MAX_STEMS], float (&mr)[SRT_MAX_STEMS], const float* __restrict__ masks, int T, int F, size_t sstride,
                                                int ntiles, int O, int t, int k, int S)
{
    const size_t tf = (size_t)T * F;
    const OvRow ov = srt_ov_row(t, T, O, ntiles);
    const float* b = masks + (size_t)ov.j1 * 2 * tf + (size_t)ov.k * F + k;
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) {
        ml[j] = 0.0f; mr[j] = 0.0f;
        if (j < S) { ml[j] = b[j * sstride]; mr[j] = b[j * sstride + tf]; }
    }
    if (ov.two) {
        const float* a = b - 2 * tf + (size_t)(T - O) * F;
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S) { ml[j] = srt_blend(a[j * sstride], ml[j], ov.w); mr[j] = srt_blend(a[j * sstride + tf], mr[j], ov.w); }
    }
}

// srt_wiener_stats_batch_kernel with the mask fetch replaced by the overlapped fetch on the track's view (launched only with an overlap); the chain and the
// accumulation are srt_wiener_stats_ov_kernel's
__global__ void __launch_bounds__(256) srt_wiener_stats_batch_ov_kernel(const SrtWienerParams p, const SrtBatchTrack* __restrict__ tracks,
                                                                        const SrtBatchWiener* __restrict__ wt, int ntracks, int O, int pass)
{
    __shared__ float red[4];
    const int k = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, S = p.nstems;
    const int trk = w_chunk_track(wt, ntracks, c);
    const SrtBatchWiener g = wt[trk];
    const int rows = tracks[trk].rows, tile0 = tracks[trk].tile0, tiles = tracks[trk].ntiles;
    const int r0 = (c - g.chunk0) * g.rpc, r1 = min(r0 + g.rpc, rows);           // rows of the TRACK
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf;
    const float* scal = p.scal + g.tab;
    const float4* rtab = reinterpret_cast<const float4*>(p.rtab) + (size_t)g.tab * SRT_WIENER_MAX_ITERS * S * p.F;
    const float al = (pass > 1 ? scal[0] : 1.0f) * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    const bool inb = k < p.F, anyb = k < SRT_HALF;
    const float2* sLp = p.spec + (size_t)tile0 * p.T * SRT_SPEC_LD + (anyb ? k : 0);       // the track's first packed row
    const float2* sRp = sLp + p.spec_ch_stride;
    const float* masks = p.masks + (size_t)tile0 * 2 * tf;                                 // ... and first packed tile
    float acc[SRT_MAX_STEMS][4];
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j) { acc[j][0] = 0.0f; acc[j][1] = 0.0f; acc[j][2] = 0.0f; acc[j][3] = 0.0f; }
    float mx = 0.0f;
    if (anyb) {
        for (int t = r0; t < r1; ++t) {
            const float2 sL = sLp[(size_t)t * SRT_SPEC_LD], sR = sRp[(size_t)t * SRT_SPEC_LD];
            if (pass == 1) mx = fmaxf(mx, fmaxf(hypotf(sL.x, sL.y), hypotf(sR.x, sR.y)));
            if (!inb) continue;
            float ml[SRT_MAX_STEMS], mr[SRT_MAX_STEMS];
            w_masks_ov_view(ml, mr, masks, p.T, p.F, sstride, tiles, O, t, k, S);
            float2 yl[SRT_MAX_STEMS], yr[SRT_MAX_STEMS];
            w_start_v(yl, yr, sL, sR, ml, mr, S);
            for (int i = 0; i < pass - 1; ++i)
                w_iter<true>(yl, yr, sL, sR, rtab + (size_t)i * S * p.F + k, p.F, delta, S);
#pragma unroll
            for (int j = 0; j < SRT_MAX_STEMS; ++j) {
                acc[j][0] += yl[j].x * yl[j].x + yl[j].y * yl[j].y;
                acc[j][1] += yr[j].x * yr[j].x + yr[j].y * yr[j].y;
                acc[j][2] += yl[j].x * yr[j].x + yl[j].y * yr[j].y;      // y_L conj(y_R)
                acc[j][3] += yl[j].y * yr[j].x - yl[j].x * yr[j].y;
            }
        }
    }
    if (inb) {
#pragma unroll
        for (int j = 0; j < SRT_MAX_STEMS; ++j)
            if (j < S)
#pragma unroll
                for (int q = 0; q < 4; ++q) p.slab[(((size_t)c * S + j) * 4 + q) * p.F + k] = acc[j][q];
    }
    if (pass == 1) {                                             // (block-uniform branch: every thread reaches the barriers)
        mx = w_block_max(mx, red);
        if (threadIdx.x == 0) p.slab_max[c * SRT_WIENER_BINBLK + blockIdx.x] = mx;
    }
}

// w_mix_inband / w_mix_gain on a matrix ROW in device memory (the track's, from the batch gain table: g[j] the gain of stem j, g[S] of the input) instead of the
// launch arguments: the same statements in the same order.  The row's address is workgroup-uniform, so its entries are scalar loads.
#pragma clang fp contract(off)
__device__ __forceinline__ float2 w_mix_inband(const float* __restrict__ row, int S, float2 s, const float2 (&y)[SRT_MAX_STEMS])
{
    const float g = row[S];
    float hx = g * s.x, hy = g * s.y;
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j)
        if (j < S) { const float gj = row[j]; hx = fmaf(gj, y[j].x, hx); hy = fmaf(gj, y[j].y, hy); }
    return make_float2(hx, hy);
}
__device__ __forceinline__ float w_mix_gain(const float* __restrict__ row, int S, const float (&g)[SRT_MAX_STEMS])
{
    float h = row[S];
#pragma unroll
    for (int j = 0; j < SRT_MAX_STEMS; ++j)
        if (j < S) h = fmaf(row[j], g[j], h);
    return h;
}
#pragma clang fp contract(fast)

// srt_wiener_filter_opt_kernel per track of a packed batch: blocks of W_FILTER_ROWS packed rows as in srt_wiener_filter_batch_kernel (a block lies in one tile,
// hence in one track - rows_k <= ntiles_k * T holds with an overlap too; rows at or past the track's own are skipped), the FINAL spectrum of every bin of the
// q.n_out mixes or of every stem as in the single-signal kernel.  The extension table is indexed by packed row; the remix reads the track's own matrix
// q.gains + trk * n_out * (S + 1).  The remix stays a run-time branch inside one compiled copy per OV (see srt_wiener_filter_opt_kernel).
template <bool OV>
__global__ void __launch_bounds__(256) srt_wiener_filter_batch_opt_kernel(const SrtWienerParams p, const SrtBatchWienerOpt q, const SrtBatchTrack* __restrict__ tracks,
                                                                          const SrtBatchWiener* __restrict__ wt, int ntracks, int iters)
{
    const int k = blockIdx.x * 256 + threadIdx.x, S = p.nstems;
    if (k >= SRT_HALF) return;
    const int r0 = blockIdx.y * W_FILTER_ROWS;                                   // packed rows
    const int trk = w_tile_track(tracks, ntracks, r0 / p.T);
    const int tab = wt[trk].tab;
    const int row0 = tracks[trk].tile0 * p.T;                                    // the track's first packed row
    const int r1 = min(r0 + W_FILTER_ROWS, row0 + tracks[trk].rows);
    const size_t tf = (size_t)p.T * p.F, sstride = (size_t)p.ntiles * 2 * tf, och = p.out_stem / 2;
    const float4* rtab = reinterpret_cast<const float4*>(p.rtab) + (size_t)tab * SRT_WIENER_MAX_ITERS * S * p.F;
    const float al = p.scal[tab] * (1.0f / 4096.0f), delta = W_SQRT_EPS * al * al;
    const float* gains = q.gains + (size_t)trk * q.n_out * (S + 1);             // (not dereferenced with n_out = 0)
    const bool inb = k < p.F;
    for (int t = r0; t < r1; ++t) {
        const size_t o = (size_t)t * SRT_SPEC_LD + k;
        const float2 sL = p.spec[o], sR = p.spec[p.spec_ch_stride + o];
        if (!inb) {
            float gl[SRT_MAX_STEMS], gr[SRT_MAX_STEMS];
#pragma unroll
            for (int j = 0; j < SRT_MAX_STEMS; ++j) {
                gl[j] = 0.0f; gr[j] = 0.0f;
                if (j < S) {
                    if (q.ext) { const float* e = q.ext + (size_t)j * q.ext_stem + (size_t)t * 2; gl[j] = e[0]; gr[j] = e[1]; }
                    else { gl[j] = q.oob[j]; gr[j] = gl[j]; }
                }
            }
            if (q.n_out) {
                for (int m = 0; m < q.n_out; ++m) {
                    p.out[m * p.out_stem + o] = w_scale(w_mix_gain(gains + m * (S + 1), S, gl), sL);
                    p.out[m * p.out_stem + och + o] = w_scale(w_mix_gain(gains + m * (S + 1), S, gr), sR);
                }
            } else {
#pragma unroll
                for (int j = 0; j < SRT_MAX_STEMS; ++j)
                    if (j < S) { p.out[j * p.out_stem + o] = w_scale(gl[j], sL); p.out[j * p.out_stem + och + o] = w_scale(gr[j], sR); }
            }
            continue;
        }
        float2 yl[SRT_MAX_STEMS], yr[SRT_MAX_STEMS];
        if constexpr (OV) {
            float ml[SRT_MAX_STEMS], mr[SRT_MAX_STEMS];
            w_masks_ov_view(ml, mr, p.masks + (size_t)tracks[trk].tile0 * 2 * tf, p.T, p.F, sstride, tracks[trk].ntiles, q.overlap, t - row0, k, S);
            w_start_v(yl, yr, sL, sR, ml, mr, S);
        } else {
            const float* m = p.masks + (size_t)(t / p.T) * 2 * tf + (size_t)(t % p.T) * p.F + k;      // packed tile = the track's first + the tile within it
            w_start(yl, yr, sL, sR, m, sstride, tf, S);
        }
        for (int i = 0; i < iters; ++i)
            w_iter<true>(yl, yr, sL, sR, rtab + (size_t)i * S * p.F + k, p.F, delta, S);
        if (q.n_out) {
            for (int m = 0; m < q.n_out; ++m) {
                p.out[m * p.out_stem + o] = w_mix_inband(gains + m * (S + 1), S, sL, yl);
                p.out[m * p.out_stem + och + o] = w_mix_inband(gains + m * (S + 1), S, sR, yr);
            }
        } else {
#pragma unroll
            for (int j = 0; j < SRT_MAX_STEMS; ++j)
                if (j < S) { p.out[j * p.out_stem + o] = yl[j]; p.out[j * p.out_stem + och + o] = yr[j]; }
        }
    }
}

// (the table's ntiles / rows per track come from batch_forward's plan at the same overlap, so srt_ov_row stays inside the track's tiles: w_layout_ok per track)
int srt_launch_wiener_stats_batch_ov(const SrtWienerParams& p, const SrtBatchTrack* d_tracks, const SrtBatchWiener* d_wt, int ntracks, int overlap, int pass, hipStream_t s)
{
    if (pass < 1 || pass > SRT_WIENER_MAX_ITERS || !w_batch_args_ok(p, ntracks) || overlap < 1 || overlap > p.T / 2) return -1;
    const int bx = pass == 1 ? SRT_WIENER_BINBLK : (p.F + 255) / 256;      // pass 1 also covers the out-of-band bins for max |x|
    SRT_LAUNCH(srt_wiener_stats_batch_ov_kernel, dim3(bx, p.nchunks), dim3(256), 0, s, p, d_tracks, d_wt, ntracks, overlap, pass);
    return srt_launch_status();
}

int srt_launch_wiener_filter_batch_opt(const SrtWienerParams& p, const SrtBatchWienerOpt& q, const SrtBatchTrack* d_tracks, const SrtBatchWiener* d_wt, int ntracks, int iters, hipStream_t s)
{
    if (iters < 1 || iters > SRT_WIENER_MAX_ITERS || !w_batch_args_ok(p, ntracks) || p.rows / W_FILTER_ROWS > 65535 || p.out_stem != 2 * (size_t)p.rows * SRT_SPEC_LD) return -1;
    if (q.overlap < 0 || q.overlap > p.T / 2 || q.n_out < 0 || q.n_out > p.nstems || (q.n_out && !q.gains) || (q.ext && q.ext_stem < (size_t)p.rows * 2)) return -1;
    const dim3 grid(SRT_WIENER_BINBLK, p.rows / W_FILTER_ROWS), block(256);
    if (q.overlap > 0) SRT_LAUNCH(srt_wiener_filter_batch_opt_kernel<true>, grid, block, 0, s, p, q, d_tracks, d_wt, ntracks, iters);
    else SRT_LAUNCH(srt_wiener_filter_batch_opt_kernel<false>, grid, block, 0, s, p, q, d_tracks, d_wt, ntracks, iters);
    return srt_launch_status();
}
