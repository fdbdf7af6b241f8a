// srt_pcm.hip — 16-bit PCM at the host-stream boundary: interleaved stereo int16 <-> planar fp32 on the device, so that a long file crosses
// PCIe as the 16-bit samples it is read from and written to.
//
// The rule.  Unpack: x = (float)q * 2^-15 (exact).  Pack: v = rint(x * 2^15) with ties to even (the product only moves the exponent, so it is exact and
// contraction has nothing to fuse); NaN -> 0; otherwise clamped to [-32768, 32767].  A sample counts as CLIPPED when v lies outside that range or is NaN:
// +1.0f clips (v = 32768), -1.0f does not.
//
// Both kernels move bytes and nothing else: four stereo frames are one 16-byte int16 access and one float4 per plane, a lane handles one such group per
// trip of a grid-stride loop, and the grid is capped (SRT_PCM_MAX_WGS workgroups of 256 lanes).  A pointer or stride that is not 16-byte aligned takes the
// same loop frame by frame; so does the count % 4 tail.
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

// ---- C ABI (include/spleeterrt_amd.h): device pointers of any alignment, asynchronous on `stream`
int srtPcm16Unpack(void* stream, const int16_t* d_in, size_t n, float* d_L, float* d_R)
{
    if (!d_in || !d_L || !d_R) return srt_set_error(-1, "%s: null argument", "srtPcm16Unpack");
    if (srt_launch_pcm16_unpack(d_in, n, d_L, d_R, (hipStream_t)stream)) return srt_set_error(-2, "%s: kernel launch failed", "srtPcm16Unpack");
    return 0;
}

int srtPcm16Pack(void* stream, const float* d_planes, size_t plane_stride, int pairs, size_t count, int16_t* d_out, size_t out_stride, unsigned long long* d_clipped)
{
    if (!d_planes || !d_out) return srt_set_error(-1, "%s: null argument", "srtPcm16Pack");
    if (pairs < 1) return srt_set_error(-1, "%s: need pairs >= 1", "srtPcm16Pack");
    if (plane_stride < count || out_stride < count) return srt_set_error(-1, "%s: plane_stride and out_stride must be at least count", "srtPcm16Pack");
    if (pairs > 65535) return srt_set_error(-1, "%s: at most 65535 pairs per call", "srtPcm16Pack");          // grid y
    if (!count) return 0;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* scratch = nullptr;
    bool pooled = true;
    // the workgroup counts live in stream-ordered memory of this call (allocated and freed on `stream`: nothing is shared between calls or streams); a device
    // without memory pools gets a plain allocation, released once the stream has drained (that call is then not asynchronous)
    if (d_clipped && hipMallocAsync((void**)&scratch, srt_pcm16_pack_scratch(pairs) * sizeof(unsigned long long), s) != hipSuccess) {
        (void)hipGetLastError();
        pooled = false; scratch = nullptr;
        if (hipMalloc((void**)&scratch, srt_pcm16_pack_scratch(pairs) * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            return srt_set_error(-2, "%s: allocation of the clip counts failed", "srtPcm16Pack");
        }
    }
    const int rc = srt_launch_pcm16_pack(d_planes, plane_stride, pairs, count, d_out, out_stride, d_clipped, scratch, s);
    if (scratch && pooled) (void)hipFreeAsync(scratch, s);
    else if (scratch) { (void)hipStreamSynchronize(s); (void)hipFree(scratch); }
    return rc ? srt_set_error(-2, "%s: kernel launch failed", "srtPcm16Pack") : 0;
}
