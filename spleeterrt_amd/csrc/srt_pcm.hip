// srt_pcm.hip — integer PCM at the host-stream boundary: interleaved stereo int16 or packed 24-bit <-> planar fp32 on the device, so that a
// long file crosses PCIe as the samples it is read from and written to.
//
// The 16-bit rule.  Unpack: x = (float)q * 2^-15 (exact).  Pack: v = rint(x * 2^15) with ties to even (the product only moves the exponent, so it is exact and
// contraction has nothing to fuse); NaN -> 0; otherwise clamped to [-32768, 32767].  A sample counts as CLIPPED when v lies outside that range or is NaN:
// +1.0f clips (v = 32768), -1.0f does not.
// The 24-bit rule (three bytes per sample, little-endian, two's complement): the same with 2^23 and [-8388608, 8388607]; the unpack sign-extends the three bytes.
// The dithered 16-bit rule: v = rint(x * 2^15 + d), d a TPDF value in (-1, 1) LSB that is a pure function of (seed, plane, sample index) - srt_dither below; the
// clamp, NaN and the clip count are the 16-bit rule's, applied to the dithered v.
//
// The kernels move bytes and little else: four stereo frames are one 16-byte int16 access and one float4 per plane (24-bit: eight frames are three 16-byte
// accesses and two float4 per plane), a lane handles one such group per trip of a grid-stride loop, and the grid is capped (SRT_PCM_MAX_WGS workgroups of 256
// lanes).  A pointer or stride that is not 16-byte aligned takes the same loop frame by frame; so does the count % 4 (24-bit: count % 8) tail.
// Clipped samples are counted without atomics: every workgroup of the pack writes its count, and a second launch adds a pair's counts, in a fixed order, to
// the pair's 64-bit counter (integer sums: the same bits every run).
#include "srt_internal.h"
#include "../../include/spleeterrt_amd.h"

#define SRT_PCM_MAX_WGS 2048          // 256 CUs x 8 workgroups of four waves: every SIMD holds eight waves with two 16-byte loads each in flight

struct alignas(16) SrtShort8 { short v[8]; };

__device__ __forceinline__ float srt_pcm16_to_float(short q) { return (float)q * (1.0f / 32768.0f); }

// v = rint(x * 32768); *clipped += (v outside [-32768, 32767] or NaN)
__device__ __forceinline__ short srt_float_to_pcm16(float x, unsigned& clipped)
{
    const float v = rintf(x * 32768.0f);
    const bool in = v >= -32768.0f && v <= 32767.0f;                      // false for NaN
    clipped += in ? 0u : 1u;
    return v != v ? (short)0 : (short)(int)fminf(fmaxf(v, -32768.0f), 32767.0f);
}

// in [n][2] -> L [n], R [n].  nvec: groups of four frames taken 16 bytes at a time (0 when something is unaligned); frames [4 nvec, n) one by one.
__global__ void __launch_bounds__(256) srt_pcm16_unpack_kernel(const short* __restrict__ in, size_t n, size_t nvec, float* __restrict__ L, float* __restrict__ R)
{
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    for (size_t g = tid; g < nvec; g += step) {
        const SrtShort8 q = reinterpret_cast<const SrtShort8*>(in)[g];
        float4 l, r;
        l.x = srt_pcm16_to_float(q.v[0]); r.x = srt_pcm16_to_float(q.v[1]);
        l.y = srt_pcm16_to_float(q.v[2]); r.y = srt_pcm16_to_float(q.v[3]);
        l.z = srt_pcm16_to_float(q.v[4]); r.z = srt_pcm16_to_float(q.v[5]);
        l.w = srt_pcm16_to_float(q.v[6]); r.w = srt_pcm16_to_float(q.v[7]);
        reinterpret_cast<float4*>(L)[g] = l;
        reinterpret_cast<float4*>(R)[g] = r;
    }
    for (size_t i = nvec * 4 + tid; i < n; i += step) {
        L[i] = srt_pcm16_to_float(in[2 * i]);
        R[i] = srt_pcm16_to_float(in[2 * i + 1]);
    }
}

// Pair p = blockIdx.y: planes + 2p * plane_stride (L) and + (2p + 1) * plane_stride (R), samples [0, count) -> out + p * out_stride * 2 as [count][2].
// partial (COUNT only): [pairs][gridDim.x] clipped samples of each workgroup.
template <bool COUNT>
__global__ void __launch_bounds__(256) srt_pcm16_pack_kernel(const float* __restrict__ planes, size_t plane_stride, size_t count, size_t nvec,
                                                              short* __restrict__ out, size_t out_stride, unsigned long long* __restrict__ partial)
{
    const int p = blockIdx.y;
    const float* L = planes + (size_t)(2 * p) * plane_stride;
    const float* R = L + plane_stride;
    short* o = out + (size_t)p * out_stride * 2;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    unsigned clipped = 0;                                                  // a lane sees count / (256 gridDim.x) frames: far below 2^32
    for (size_t g = tid; g < nvec; g += step) {
        const float4 l = reinterpret_cast<const float4*>(L)[g];
        const float4 r = reinterpret_cast<const float4*>(R)[g];
        SrtShort8 q;
        q.v[0] = srt_float_to_pcm16(l.x, clipped); q.v[1] = srt_float_to_pcm16(r.x, clipped);
        q.v[2] = srt_float_to_pcm16(l.y, clipped); q.v[3] = srt_float_to_pcm16(r.y, clipped);
        q.v[4] = srt_float_to_pcm16(l.z, clipped); q.v[5] = srt_float_to_pcm16(r.z, clipped);
        q.v[6] = srt_float_to_pcm16(l.w, clipped); q.v[7] = srt_float_to_pcm16(r.w, clipped);
        reinterpret_cast<SrtShort8*>(o)[g] = q;
    }
    for (size_t i = nvec * 4 + tid; i < count; i += step) {
        o[2 * i] = srt_float_to_pcm16(L[i], clipped);
        o[2 * i + 1] = srt_float_to_pcm16(R[i], clipped);
    }
    if (COUNT) {
        __shared__ unsigned long long s_wave[4];
        unsigned long long c = clipped;
#pragma unroll
        for (int d = 32; d; d >>= 1) c += __shfl_down(c, d, 64);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) partial[(size_t)p * gridDim.x + blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    }
}

// one wave per pair: clipped[p] += the pair's nwg workgroup counts (lane-strided, then the shuffle tree: a fixed order, and integer sums anyway)
__global__ void __launch_bounds__(64) srt_pcm16_count_kernel(const unsigned long long* __restrict__ partial, int nwg, unsigned long long* __restrict__ clipped)
{
    const int p = blockIdx.x;
    unsigned long long c = 0;
    for (int i = threadIdx.x; i < nwg; i += 64) c += partial[(size_t)p * nwg + i];
#pragma unroll
    for (int d = 32; d; d >>= 1) c += __shfl_down(c, d, 64);
    if (threadIdx.x == 0) clipped[p] += c;
}

// a workgroup's clipped samples -> partial[p][blockIdx.x] (the epilogue of srt_pcm16_pack_kernel<true>, for the kernels below)
__device__ __forceinline__ void srt_pcm_store_count(unsigned clipped, int p, unsigned long long* __restrict__ partial)
{
    __shared__ unsigned long long s_wave[4];
    unsigned long long c = clipped;
#pragma unroll
    for (int d = 32; d; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)p * gridDim.x + blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// ---- packed 24-bit: sample k of a run of bytes is bytes [3k, 3k + 3), little-endian two's complement
struct alignas(16) SrtWord4 { unsigned v[4]; };

__device__ __forceinline__ float srt_pcm24_to_float(int q) { return (float)q * (1.0f / 8388608.0f); }      // |q| <= 2^23: the conversion and the product are exact

// v = rint(x * 2^23) (the product is exact); *clipped += (v outside [-8388608, 8388607] or NaN); -> the clamped value's low 24 bits
__device__ __forceinline__ unsigned srt_float_to_pcm24(float x, unsigned& clipped)
{
    const float v = rintf(x * 8388608.0f);
    const bool in = v >= -8388608.0f && v <= 8388607.0f;                  // false for NaN
    clipped += in ? 0u : 1u;
    return v != v ? 0u : (unsigned)(int)fminf(fmaxf(v, -8388608.0f), 8388607.0f) & 0xffffffu;
}

// sample k (0 .. 15) of twelve words, sign-extended; k is a constant after unrolling, so every case is one or two shifts
__device__ __forceinline__ int srt_pcm24_get(const unsigned (&w)[12], int k)
{
    const int j = (3 * k) >> 2, o = (3 * k) & 3;
    const unsigned t = o == 0 ? w[j] : o == 1 ? w[j] >> 8 : (w[j] >> (8 * o)) | (w[j + 1] << (32 - 8 * o));
    return (int)(t << 8) >> 8;
}
__device__ __forceinline__ int srt_pcm24_get_bytes(const unsigned char* p) { return (int)((unsigned)p[0] << 8 | (unsigned)p[1] << 16 | (unsigned)p[2] << 24) >> 8; }
__device__ __forceinline__ void srt_pcm24_put_bytes(unsigned char* p, unsigned q) { p[0] = (unsigned char)q; p[1] = (unsigned char)(q >> 8); p[2] = (unsigned char)(q >> 16); }

// in [n][2][3] -> L [n], R [n].  nvec: groups of eight frames taken as three 16-byte loads (0 when something is unaligned); frames [8 nvec, n) byte by byte.
__global__ void __launch_bounds__(256) srt_pcm24_unpack_kernel(const unsigned char* __restrict__ in, size_t n, size_t nvec, float* __restrict__ L, float* __restrict__ R)
{
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    for (size_t g = tid; g < nvec; g += step) {
        unsigned w[12];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const SrtWord4 q = reinterpret_cast<const SrtWord4*>(in)[3 * g + a];
#pragma unroll
            for (int c = 0; c < 4; ++c) w[4 * a + c] = q.v[c];
        }
        float l[8], r[8];
#pragma unroll
        for (int f = 0; f < 8; ++f) { l[f] = srt_pcm24_to_float(srt_pcm24_get(w, 2 * f)); r[f] = srt_pcm24_to_float(srt_pcm24_get(w, 2 * f + 1)); }
        reinterpret_cast<float4*>(L)[2 * g] = make_float4(l[0], l[1], l[2], l[3]);
        reinterpret_cast<float4*>(L)[2 * g + 1] = make_float4(l[4], l[5], l[6], l[7]);
        reinterpret_cast<float4*>(R)[2 * g] = make_float4(r[0], r[1], r[2], r[3]);
        reinterpret_cast<float4*>(R)[2 * g + 1] = make_float4(r[4], r[5], r[6], r[7]);
    }
    for (size_t i = nvec * 8 + tid; i < n; i += step) {
        L[i] = srt_pcm24_to_float(srt_pcm24_get_bytes(in + 6 * i));
        R[i] = srt_pcm24_to_float(srt_pcm24_get_bytes(in + 6 * i + 3));
    }
}

// Pair p = blockIdx.y: planes + 2p * plane_stride (L) and + (2p + 1) * plane_stride (R), samples [0, count) -> out + p * out_stride * 6 as [count][2][3].
// partial (COUNT only): [pairs][gridDim.x] clipped samples of each workgroup.
template <bool COUNT>
__global__ void __launch_bounds__(256) srt_pcm24_pack_kernel(const float* __restrict__ planes, size_t plane_stride, size_t count, size_t nvec,
                                                              unsigned char* __restrict__ out, size_t out_stride, unsigned long long* __restrict__ partial)
{
    const int p = blockIdx.y;
    const float* L = planes + (size_t)(2 * p) * plane_stride;
    const float* R = L + plane_stride;
    unsigned char* o = out + (size_t)p * out_stride * 6;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    unsigned clipped = 0;                                                  // a lane sees count / (256 gridDim.x) frames: far below 2^32
    for (size_t g = tid; g < nvec; g += step) {
        const float4 l0 = reinterpret_cast<const float4*>(L)[2 * g], l1 = reinterpret_cast<const float4*>(L)[2 * g + 1];
        const float4 r0 = reinterpret_cast<const float4*>(R)[2 * g], r1 = reinterpret_cast<const float4*>(R)[2 * g + 1];
        const float x[16] = { l0.x, r0.x, l0.y, r0.y, l0.z, r0.z, l0.w, r0.w, l1.x, r1.x, l1.y, r1.y, l1.z, r1.z, l1.w, r1.w };
        unsigned w[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
        for (int k = 0; k < 16; ++k) {                                     // sample k lands at byte 3k: word j from bit 8 o, the rest in word j + 1
            const unsigned q = srt_float_to_pcm24(x[k], clipped);
            const int j = (3 * k) >> 2, sh = 8 * ((3 * k) & 3);
            w[j] |= q << sh;
            if (sh > 8) w[j + 1] |= q >> (32 - sh);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            SrtWord4 q;
#pragma unroll
            for (int c = 0; c < 4; ++c) q.v[c] = w[4 * a + c];
            reinterpret_cast<SrtWord4*>(o)[3 * g + a] = q;
        }
    }
    for (size_t i = nvec * 8 + tid; i < count; i += step) {
        srt_pcm24_put_bytes(o + 6 * i, srt_float_to_pcm24(L[i], clipped));
        srt_pcm24_put_bytes(o + 6 * i + 3, srt_float_to_pcm24(R[i], clipped));
    }
    if (COUNT) srt_pcm_store_count(clipped, p, partial);
}

// ---- TPDF dither for the 16-bit pack (the definition is in include/spleeterrt_amd.h).  All arithmetic is uint32 with wrap-around.
__device__ __forceinline__ unsigned srt_mix32(unsigned x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
// k of (seed, plane)
__device__ __forceinline__ unsigned srt_dither_key(unsigned long long seed, unsigned plane) { return srt_mix32((unsigned)seed ^ srt_mix32((unsigned)(seed >> 32) ^ srt_mix32(plane + 0x9e3779b9u))); }
// d of the key folded with the index's high word, kh = mix32(hi32(i) ^ k), and its low word: the difference of two 24-bit uniforms, exact in fp32
__device__ __forceinline__ float srt_dither_lo(unsigned kh, unsigned lo)
{
    const unsigned h = srt_mix32(lo ^ kh);
    const unsigned a = srt_mix32(h ^ 0x68bc21ebu) >> 8, b = srt_mix32(h ^ 0x02e5be93u) >> 8;
    return (float)((int)a - (int)b) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float srt_dither(unsigned k, unsigned long long i) { return srt_dither_lo(srt_mix32((unsigned)(i >> 32) ^ k), (unsigned)i); }

// v = rint(x * 32768 + d).  x * 32768 is exact, so the sum is rounded once whether or not the compiler contracts the two operations into an fma: the same bits
// either way.  Clamp, NaN and the clip count as srt_float_to_pcm16, on the dithered v.
__device__ __forceinline__ short srt_float_to_pcm16_dither(float x, float d, unsigned& clipped)
{
    const float v = rintf(x * 32768.0f + d);
    const bool in = v >= -32768.0f && v <= 32767.0f;                      // false for NaN
    clipped += in ? 0u : 1u;
    return v != v ? (short)0 : (short)(int)fminf(fmaxf(v, -32768.0f), 32767.0f);
}

// srt_pcm16_pack_kernel's layout with the dither: sample i of pair p's channel c takes d(seed, 2 (first_pair + p) + c, first_index + i).  A group of four frames
// shares the high word of its indices unless it straddles a multiple of 2^32 (then every sample folds its own).
template <bool COUNT>
__global__ void __launch_bounds__(256) srt_pcm16_pack_dither_kernel(const float* __restrict__ planes, size_t plane_stride, size_t count, size_t nvec,
                                                                     short* __restrict__ out, size_t out_stride, unsigned long long* __restrict__ partial,
                                                                     unsigned long long seed, unsigned first_pair, unsigned long long first_index)
{
    const int p = blockIdx.y;
    const float* L = planes + (size_t)(2 * p) * plane_stride;
    const float* R = L + plane_stride;
    short* o = out + (size_t)p * out_stride * 2;
    const unsigned kL = srt_dither_key(seed, 2u * (first_pair + (unsigned)p)), kR = srt_dither_key(seed, 2u * (first_pair + (unsigned)p) + 1u);
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    unsigned clipped = 0;                                                  // a lane sees count / (256 gridDim.x) frames: far below 2^32
    for (size_t g = tid; g < nvec; g += step) {
        const float4 l = reinterpret_cast<const float4*>(L)[g];
        const float4 r = reinterpret_cast<const float4*>(R)[g];
        const unsigned long long i0 = first_index + 4 * (unsigned long long)g;
        const unsigned lo = (unsigned)i0;
        float dl[4], dr[4];
        if (lo <= 0xfffffffcu) {
            const unsigned hL = srt_mix32((unsigned)(i0 >> 32) ^ kL), hR = srt_mix32((unsigned)(i0 >> 32) ^ kR);
#pragma unroll
            for (int j = 0; j < 4; ++j) { dl[j] = srt_dither_lo(hL, lo + j); dr[j] = srt_dither_lo(hR, lo + j); }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { dl[j] = srt_dither(kL, i0 + j); dr[j] = srt_dither(kR, i0 + j); }
        }
        SrtShort8 q;
        q.v[0] = srt_float_to_pcm16_dither(l.x, dl[0], clipped); q.v[1] = srt_float_to_pcm16_dither(r.x, dr[0], clipped);
        q.v[2] = srt_float_to_pcm16_dither(l.y, dl[1], clipped); q.v[3] = srt_float_to_pcm16_dither(r.y, dr[1], clipped);
        q.v[4] = srt_float_to_pcm16_dither(l.z, dl[2], clipped); q.v[5] = srt_float_to_pcm16_dither(r.z, dr[2], clipped);
        q.v[6] = srt_float_to_pcm16_dither(l.w, dl[3], clipped); q.v[7] = srt_float_to_pcm16_dither(r.w, dr[3], clipped);
        reinterpret_cast<SrtShort8*>(o)[g] = q;
    }
    for (size_t i = nvec * 4 + tid; i < count; i += step) {
        o[2 * i] = srt_float_to_pcm16_dither(L[i], srt_dither(kL, first_index + i), clipped);
        o[2 * i + 1] = srt_float_to_pcm16_dither(R[i], srt_dither(kR, first_index + i), clipped);
    }
    if (COUNT) srt_pcm_store_count(clipped, p, partial);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int srt_launch_pcm16_unpack(const int16_t* in, size_t n, float* L, float* R, hipStream_t s)
{
    if (!n) return 0;
    const size_t nvec = aligned16(in) && aligned16(L) && aligned16(R) ? n / 4 : 0;
    const size_t items = nvec ? nvec + (n & 3) : n, want = (items + 255) / 256;
    const unsigned wgs = (unsigned)(want < SRT_PCM_MAX_WGS ? want : SRT_PCM_MAX_WGS);
    SRT_LAUNCH(srt_pcm16_unpack_kernel, dim3(wgs), dim3(256), 0, s, (const short*)in, n, nvec, L, R);
    return srt_launch_status();
}

// workgroups per pair: the cap is shared by the pairs of a launch
static unsigned pack_wgs(size_t items, int pairs)
{
    const size_t want = (items + 255) / 256, cap = SRT_PCM_MAX_WGS / (size_t)pairs ? SRT_PCM_MAX_WGS / (size_t)pairs : 1;
    return (unsigned)(want < cap ? want : cap);
}
size_t srt_pcm16_pack_scratch(int pairs) { return pairs > SRT_PCM_MAX_WGS ? (size_t)pairs : (size_t)SRT_PCM_MAX_WGS; }

int srt_launch_pcm16_pack(const float* planes, size_t plane_stride, int pairs, size_t count, int16_t* out, size_t out_stride,
                          unsigned long long* clipped, unsigned long long* scratch, hipStream_t s)
{
    if (!count || pairs < 1) return 0;
    // every pair's three bases are 16-byte aligned when the first ones are and the strides are whole 16-byte units (4 floats; 4 frames of 4 bytes)
    const size_t nvec = aligned16(planes) && aligned16(out) && plane_stride % 4 == 0 && out_stride % 4 == 0 ? count / 4 : 0;
    const unsigned wgs = pack_wgs(nvec ? nvec + (count & 3) : count, pairs);
    if (clipped) {
        SRT_LAUNCH((srt_pcm16_pack_kernel<true>), dim3(wgs, pairs), dim3(256), 0, s, planes, plane_stride, count, nvec, (short*)out, out_stride, scratch);
        SRT_LAUNCH(srt_pcm16_count_kernel, dim3(pairs), dim3(64), 0, s, scratch, (int)wgs, clipped);
    } else
        SRT_LAUNCH((srt_pcm16_pack_kernel<false>), dim3(wgs, pairs), dim3(256), 0, s, planes, plane_stride, count, nvec, (short*)out, out_stride, (unsigned long long*)nullptr);
    return srt_launch_status();
}

int srt_launch_pcm24_unpack(const uint8_t* in, size_t n, float* L, float* R, hipStream_t s)
{
    if (!n) return 0;
    const size_t nvec = aligned16(in) && aligned16(L) && aligned16(R) ? n / 8 : 0;
    const size_t items = nvec ? nvec + (n & 7) : n, want = (items + 255) / 256;
    const unsigned wgs = (unsigned)(want < SRT_PCM_MAX_WGS ? want : SRT_PCM_MAX_WGS);
    SRT_LAUNCH(srt_pcm24_unpack_kernel, dim3(wgs), dim3(256), 0, s, (const unsigned char*)in, n, nvec, L, R);
    return srt_launch_status();
}

int srt_launch_pcm24_pack(const float* planes, size_t plane_stride, int pairs, size_t count, uint8_t* out, size_t out_stride,
                          unsigned long long* clipped, unsigned long long* scratch, hipStream_t s)
{
    if (!count || pairs < 1) return 0;
    // every pair's three bases are 16-byte aligned when the first ones are, the plane stride is whole 16-byte units (4 floats) and pair p's packed base, at
    // p * out_stride * 6 bytes, is too: out_stride a multiple of 8 frames
    const size_t nvec = aligned16(planes) && aligned16(out) && plane_stride % 4 == 0 && out_stride % 8 == 0 ? count / 8 : 0;
    const unsigned wgs = pack_wgs(nvec ? nvec + (count & 7) : count, pairs);
    if (clipped) {
        SRT_LAUNCH((srt_pcm24_pack_kernel<true>), dim3(wgs, pairs), dim3(256), 0, s, planes, plane_stride, count, nvec, (unsigned char*)out, out_stride, scratch);
        SRT_LAUNCH(srt_pcm16_count_kernel, dim3(pairs), dim3(64), 0, s, scratch, (int)wgs, clipped);
    } else
        SRT_LAUNCH((srt_pcm24_pack_kernel<false>), dim3(wgs, pairs), dim3(256), 0, s, planes, plane_stride, count, nvec, (unsigned char*)out, out_stride, (unsigned long long*)nullptr);
    return srt_launch_status();
}

int srt_launch_pcm16_pack_dither(const float* planes, size_t plane_stride, int pairs, size_t count, int16_t* out, size_t out_stride,
                                 unsigned long long* clipped, unsigned long long* scratch, unsigned long long seed, int first_pair, unsigned long long first_index, hipStream_t s)
{
    if (!count || pairs < 1) return 0;
    const size_t nvec = aligned16(planes) && aligned16(out) && plane_stride % 4 == 0 && out_stride % 4 == 0 ? count / 4 : 0;      // as srt_launch_pcm16_pack
    const unsigned wgs = pack_wgs(nvec ? nvec + (count & 3) : count, pairs);
    if (clipped) {
        SRT_LAUNCH((srt_pcm16_pack_dither_kernel<true>), dim3(wgs, pairs), dim3(256), 0, s, planes, plane_stride, count, nvec, (short*)out, out_stride, scratch,
                   seed, (unsigned)first_pair, first_index);
        SRT_LAUNCH(srt_pcm16_count_kernel, dim3(pairs), dim3(64), 0, s, scratch, (int)wgs, clipped);
    } else
        SRT_LAUNCH((srt_pcm16_pack_dither_kernel<false>), dim3(wgs, pairs), dim3(256), 0, s, planes, plane_stride, count, nvec, (short*)out, out_stride,
                   (unsigned long long*)nullptr, seed, (unsigned)first_pair, first_index);
    return srt_launch_status();
}

// ---- C ABI (include/spleeterrt_amd.h): device pointers of any alignment, asynchronous on `stream`
int srtPcm16Unpack(void* stream, const int16_t* d_in, size_t n, float* d_L, float* d_R)
{
    if (!d_in || !d_L || !d_R) return srt_set_error(-1, "%s: null argument", "srtPcm16Unpack");
    if (srt_launch_pcm16_unpack(d_in, n, d_L, d_R, (hipStream_t)stream)) return srt_set_error(-2, "%s: kernel launch failed", "srtPcm16Unpack");
    return 0;
}

int srtPcm24Unpack(void* stream, const uint8_t* d_in, size_t n, float* d_L, float* d_R)
{
    if (!d_in || !d_L || !d_R) return srt_set_error(-1, "%s: null argument", "srtPcm24Unpack");
    if (srt_launch_pcm24_unpack(d_in, n, d_L, d_R, (hipStream_t)stream)) return srt_set_error(-2, "%s: kernel launch failed", "srtPcm24Unpack");
    return 0;
}

// the checks the three packs share; 0, or -1 with the error set
static int pack_check(const char* who, const void* d_planes, size_t plane_stride, int pairs, size_t count, const void* d_out, size_t out_stride)
{
    if (!d_planes || !d_out) return srt_set_error(-1, "%s: null argument", who);
    if (pairs < 1) return srt_set_error(-1, "%s: need pairs >= 1", who);
    if (plane_stride < count || out_stride < count) return srt_set_error(-1, "%s: plane_stride and out_stride must be at least count", who);
    if (pairs > 65535) return srt_set_error(-1, "%s: at most 65535 pairs per call", who);          // grid y
    return 0;
}

// `launch(scratch)` with the workgroup counts of a counting pack: they live in stream-ordered memory of this call (allocated and freed on `stream`: nothing is
// shared between calls or streams); a device without memory pools gets a plain allocation, released once the stream has drained (that call is then not asynchronous)
template <class F>
static int pack_with_scratch(const char* who, hipStream_t s, int pairs, bool counting, F&& launch)
{
    unsigned long long* scratch = nullptr;
    bool pooled = true;
    if (counting && hipMallocAsync((void**)&scratch, srt_pcm16_pack_scratch(pairs) * sizeof(unsigned long long), s) != hipSuccess) {
        (void)hipGetLastError();
        pooled = false; scratch = nullptr;
        if (hipMalloc((void**)&scratch, srt_pcm16_pack_scratch(pairs) * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            return srt_set_error(-2, "%s: allocation of the clip counts failed", who);
        }
    }
    const int rc = launch(scratch);
    if (scratch && pooled) (void)hipFreeAsync(scratch, s);
    else if (scratch) { (void)hipStreamSynchronize(s); (void)hipFree(scratch); }
    return rc ? srt_set_error(-2, "%s: kernel launch failed", who) : 0;
}

int srtPcm16Pack(void* stream, const float* d_planes, size_t plane_stride, int pairs, size_t count, int16_t* d_out, size_t out_stride, unsigned long long* d_clipped)
{
    if (const int rc = pack_check("srtPcm16Pack", d_planes, plane_stride, pairs, count, d_out, out_stride)) return rc;
    if (!count) return 0;
    hipStream_t s = (hipStream_t)stream;
    return pack_with_scratch("srtPcm16Pack", s, pairs, d_clipped != nullptr, [&](unsigned long long* scratch) {
        return srt_launch_pcm16_pack(d_planes, plane_stride, pairs, count, d_out, out_stride, d_clipped, scratch, s); });
}

int srtPcm24Pack(void* stream, const float* d_planes, size_t plane_stride, int pairs, size_t count, uint8_t* d_out, size_t out_stride, unsigned long long* d_clipped)
{
    if (const int rc = pack_check("srtPcm24Pack", d_planes, plane_stride, pairs, count, d_out, out_stride)) return rc;
    if (!count) return 0;
    hipStream_t s = (hipStream_t)stream;
    return pack_with_scratch("srtPcm24Pack", s, pairs, d_clipped != nullptr, [&](unsigned long long* scratch) {
        return srt_launch_pcm24_pack(d_planes, plane_stride, pairs, count, d_out, out_stride, d_clipped, scratch, s); });
}

int srtPcm16PackDither(void* stream, const float* d_planes, size_t plane_stride, int pairs, size_t count, int16_t* d_out, size_t out_stride, unsigned long long* d_clipped,
                       uint64_t seed, int first_pair, uint64_t first_index)
{
    if (const int rc = pack_check("srtPcm16PackDither", d_planes, plane_stride, pairs, count, d_out, out_stride)) return rc;
    if (first_pair < 0 || first_pair > 0x3fffffff - pairs) return srt_set_error(-1, "%s: first_pair must be 0 .. 2^30 - pairs (the plane number is 32 bits)", "srtPcm16PackDither");
    if (!count) return 0;
    hipStream_t s = (hipStream_t)stream;
    return pack_with_scratch("srtPcm16PackDither", s, pairs, d_clipped != nullptr, [&](unsigned long long* scratch) {
        return srt_launch_pcm16_pack_dither(d_planes, plane_stride, pairs, count, d_out, out_stride, d_clipped, scratch, seed, first_pair, first_index, s); });
}

