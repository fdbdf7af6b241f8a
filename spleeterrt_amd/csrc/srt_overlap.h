// srt_overlap.h — the row rule and the cross-fade of overlapped network tiles, shared by the kernels that fetch masks by spectrum row (srt_dsp.hip: the
// transforms and the mask extension; srt_wiener.hip: the filter's option kernels).  Device code only; one definition, so every kernel blends the same bits.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)     // the blend is rounded step by step wherever it is inlined
// Overlapped network tiles (srtSetOverlap): consecutive tiles of a signal share O rows, stride S = T - O, tile j covers rows [jS, jS + T).
// Row f lives at row k of its primary tile j1 = min(f / S, ntiles - 1); when j1 > 0 and k < O it is row k + S of tile j1 - 1 as well, and its mask is
// a + w (b - a) with a from tile j1 - 1, b from tile j1, w = (k + 1/2) / O.  f is workgroup-uniform wherever this is used: scalar arithmetic.
struct OvRow { int j1, k; bool two; float w; };
__device__ __forceinline__ OvRow srt_ov_row(int f, int T, int O, int ntiles)
{
    const int S = T - O;
    OvRow r;
    r.j1 = min(f / S, ntiles - 1);
    r.k = f - r.j1 * S;
    r.two = r.j1 > 0 && r.k < O;
    r.w = ((float)r.k + 0.5f) / (float)O;
    return r;
}
// A piece of a longer stream (srtSeparateHostStreamOverlap): rows [0, O) of the piece's first tile have their partner in the PREVIOUS piece's last
// tile, rows [S, T), which that piece left in the mask seam carry [nstems][2][O][F] (srt_mask_seam_save_kernel).  True for those rows when a carry is given; the
// row then blends a = carry[stem][channel][k] with b = its own row under the same w.  Workgroup-uniform like everything above.
__device__ __forceinline__ bool srt_ov_seam(const OvRow& r, int O, const float* seam) { return seam != nullptr && r.j1 == 0 && r.k < O; }
// the cross-fade, rounded step by step (contract(off)): equal masks stay exactly equal (b - a = 0), so an all-ones mask stays the identity
__device__ __forceinline__ float srt_blend(float a, float b, float w)
{
    const float d = b - a;
    const float t = w * d;
    return a + t;
}
#pragma clang fp contract(fast)
