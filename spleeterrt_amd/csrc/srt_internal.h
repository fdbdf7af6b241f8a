// srt_internal.h — private declarations shared by the HIP translation units of libspleeterrt_amd.so.
// Nothing here is part of the C ABI (see include/*.h for that).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <utility>
#include <vector>

#define SRT_MAX_STEMS 8
#define SRT_FFT 4096
#define SRT_HOP 1024
#define SRT_HALF 2049
#define SRT_SPEC_LD 2052          // float2 elements per spectrum row (2049 padded to a 16-byte multiple)
#define SRT_COEFF_FLOATS 9822725u // sizeof(spleeterCoeff)/4, Executable/spleeter.h:5-31
#define SRT_ENC_MAX_CIN 256       // widest encoder input (down6)
#define SRT_COEFF_STRIDE 9822784u // per-stem stride inside the engine's single weight allocation (64-float aligned)

// error text behind srtLastError() (thread-local), settable from every translation unit of the library; returns `code`
int srt_set_error(int code, const char* fmt, const char* detail);

// Set-up paths (engine creation, weight upload, graph pre-warm, the drop-in Init functions) are serialised process-wide: they use the legacy
// null stream (synchronous copies, memsets, hipMemcpyToSymbol) and stream capture, and HIP refuses a null-stream operation issued by one host
// thread while another thread's stream is capturing ("operation would make the legacy stream depend on a capturing blocking stream") - two
// plugin instances initialised from two threads at once otherwise come up muted now and then.  Steady-state calls never take this lock: they
// use explicit streams only and replay graphs that already exist.
struct SrtSetupLock { SrtSetupLock(); ~SrtSetupLock(); };

// Owner of device and pinned host allocations: alloc() is one hipMalloc / hipHostMalloc of exactly `bytes` and records the pointer, release() frees one of them,
// clear() (and the destructor) what is left, in allocation order.  The live stream (srt_stream.hip) frees through this only.
struct SrtMem {
    std::vector<std::pair<void*, bool>> blocks;          // (pointer, pinned)
    SrtMem() = default; SrtMem(const SrtMem&) = delete;
    ~SrtMem() { clear(); }
    template <class T> hipError_t alloc(T** out, size_t bytes, bool pinned = false)
    {
        void* p = nullptr;
        const hipError_t er = pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (er == hipSuccess) { blocks.emplace_back(p, pinned); *out = (T*)p; }
        return er;
    }
    static void free_one(const std::pair<void*, bool>& b) { if (b.second) hipHostFree(b.first); else hipFree(b.first); }
    template <class T> void release(T*& q)               // q: null, or a pointer alloc() gave
    {
        for (size_t i = 0; q && i < blocks.size(); ++i) if (blocks[i].first == (void*)q) { free_one(blocks[i]); blocks.erase(blocks.begin() + i); q = nullptr; }
    }
    void clear() { for (const auto& b : blocks) free_one(b); blocks.clear(); }
};

enum { SRT_ACT_LEAKY = 0, SRT_ACT_RELU = 1, SRT_ACT_ELU = 2 };

// Run-time switches of a forward (A/B runs and the parity tests, which flip them inside one process; INTEGRATION.md mirrors this table).  Every entry point
// that issues a forward reads them ONCE (srt_read_switches, srt_engine.hip: the only place these names reach getenv) and hands the struct down to forward_range
// and the launchers that consult it.  The graph cache keys on the whole struct: a flipped switch captures a new graph instead of replaying the old form.
// Rules - FLAG: 1 unless the value starts with '0';  INT: atoi of the value when the variable is set;  INT_NONEMPTY: atoi of a non-empty value;  else the
// default.  Every field is an int (no padding: keys that hold the struct are compared with memcmp).     X(field, environment name, default, rule)
#define SRT_SWITCH_TABLE(X) \
    X(c8,        "SPLEETERRT_C8",        1,  FLAG)          /* fp16 storage, > 16 instances: down2..up5 channel-interleaved by eight (srt_nn5.hip); 0: planar (srt_nn3.hip) */ \
    X(c8l1,      "SPLEETERRT_C8L1",      1,  FLAG)          /* ... and down1's two outputs where it runs on its streamed kernels; 0: planar */ \
    X(d1f16,     "SPLEETERRT_D1F16",     1,  FLAG)          /* fp16 mode, C8 outputs: down1 on the fp16 MFMA, all stems in one launch; 0: the fp32-MFMA streamed kernels */ \
    X(m16,       "SPLEETERRT_M16",       1,  FLAG)          /* fp16 mode: srtSeparate's own masks as halves (masks16_wanted); 0: floats */ \
    X(d1s2,      "SPLEETERRT_D1S2",      1,  FLAG)          /* down1 of one or two stems on the two-wave streamed kernel; 0: the tiled kernel (and no C8 down1: srt_down1_c8_ok) */ \
    X(fuse_head, "SPLEETERRT_FUSE_HEAD", -1, INT_NONEMPTY)  /* up6 + head in one pass: 0 never, 1 wherever covered, -1 (unset): where it measured faster */ \
    X(c8_wgs,    "SPLEETERRT_C8_WGS",    0,  INT)           /* workgroups per C8 launch, overrides the table and the measurement; 0: those */ \
    X(c8_nr2,    "SPLEETERRT_C8_NR2",    1,  INT)           /* bit 0: two sub-tiles per wave in up2..up4; 0: one everywhere */ \
    X(c8_wres,   "SPLEETERRT_C8_WRES",   1,  INT)           /* the weight slab stays in LDS where a unit is one K chunk; 0: moved every step */ \
    X(c8_tune,   "SPLEETERRT_C8_TUNE",   1,  INT)           /* the first launch of a C8 layer shape measures its workgroup count; 0: table values, 2: and print the choice */ \
    X(wino_ph,   "SPLEETERRT_WINO_PH",   7,  INT)           /* fp32 Winograd decoder (srt_nn4.hip), barrier phase offset per layer group: bit 0 up1, bit 1 up2..up4, bit 2 up5; 0: every wave meets the barrier at quad 0 */ \
    X(wino_ac,   "SPLEETERRT_WINO_AC",   2,  INT)           /* fp32 Winograd decoder, all-class form (one wave per SIMD owns the four parity classes of its blocks) per layer group: bit 0 up1, bit 1 up2..up4, bit 2 up5 (built for up2..up4 only: the other bits select nothing); taken only where the group's WINO_PH bit is set too; 0: the class-split kernels */
enum { SRT_SW_FLAG, SRT_SW_INT, SRT_SW_INT_NONEMPTY };
#define SRT_SW_FIELD(field, name, dflt, rule) int field;
struct SrtSwitches { SRT_SWITCH_TABLE(SRT_SW_FIELD) };
#undef SRT_SW_FIELD
SrtSwitches srt_read_switches();

// Every kernel launch of the library goes through SRT_LAUNCH: besides launching, it notes WHICH kernel (host stub pointer + the
// launch expression's text) the calling thread launched first since srt_kernel_note_reset().  The engine's per-launch timers keep
// that with each entry, so srtGetTimingKernels() reports the kernel that actually ran a layer (the dispatch depends on batch
// size and geometry), not a table kept by hand.
void srt_kernel_note(const void* fn, const char* text);
void srt_kernel_note_reset();
// status of the launch just issued on this thread: 0, or -1 with the HIP error kept for the message srt_set_error builds next
void srt_note_hip_error(hipError_t e);
static inline int srt_launch_status() { const hipError_t e = hipGetLastError(); if (e != hipSuccess) srt_note_hip_error(e); return e == hipSuccess ? 0 : -1; }
#define SRT_LAUNCH(kernel, ...) do { srt_kernel_note((const void*)(kernel), #kernel); hipLaunchKernelGGL(kernel, __VA_ARGS__); } while (0)

// One convolution layer evaluated for nstems x ntiles independent instances.
// instance pointer = base + stem * *_stem + tile * *_tile   (strides in floats)
struct SrtConvParams {
    int Cin, Cout;        // channels
    int H, W;             // INPUT spatial size per instance (encoder output = H/2 x W/2, decoder output = 2H x 2W)
    int CA;               // channels [0,CA) come from srcA, [CA,Cin) from srcB (decoder skip concat by pointer)
    int ntiles, nstems;
    const float* srcA; size_t srcA_stem, srcA_tile;
    const float* srcB; size_t srcB_stem, srcB_tile;
    // Encoder layers 2..6 read the RAW (conv + bias) tensor of the previous layer and apply its batch-norm + activation
    // while staging: x = act(inScale[c] * raw + inShift[c]) (spleeter.c:188), per input channel c and per stem
    // (pointer = base + stem * coeff_stem + c).  nullptr: the source is used as it is (down1 reads magnitudes).
    const float* inScale; const float* inShift;
    // per-stem weights: pointer = base + stem * stride (all stems live in one allocation, so no pointer tables)
    const float* wraw;    // reference layout: encoder OIHW [Cout][Cin][5][5], decoder [Cin][Cout][5][5]
    const float* bias; const float* bnShift; const float* bnScale;   // bnScale == nullptr => no batch-norm (down6)
    size_t coeff_stem;    // stride (floats) between stems for wraw/bias/bnShift/bnScale
    const float* wpack;   // GEMM layout [Cin][25][CP], zero padded to CP output channels
    size_t wpack_stem;
    int CP;
    // stacked-M weight layouts (srt_nn2.hip): fill otherwise half-empty 32-row MFMA tiles of the Cout = 16 layers
    const float* wpack2;  // down1: [Cin][25][CP2] rows = stem*16+co over the `stack` stems of this launch (shared input);
                          // up5:   [Cin][15][32] per stem, rows = px*16+co, 15 = (ky, dx) pairs (two x-parity classes per tile)
    size_t wpack2_stem;
    int CP2, stack;
    int rowsplit;         // srt_down1_stream_kernel<.., NW = 2>: runs of intervals a column is cut into (one workgroup each); 0 / 1: whole columns
    // fp16-MFMA variant (srt_nn3.hip): [Cin/16][25][2][CP][8] IEEE halves (k-group of 8 channels innermost)
    const uint16_t* wpack16; size_t wpack16_stem;
    int nsplit;           // 1: activations rounded to fp16; 2: activations split hi+lo (two MFMAs per tap, ~fp32 products)
    // Split-K for small batches (srt_nn2.hip): when a layer's grid would leave most of the 256 CUs idle, its K loop (input
    // channels) is cut into `ksplit` slices that run as separate workgroups; each writes its partial sums to
    // ws[slice][same offsets as the output tensor] and srt_splitk_reduce adds the slices in slice order (bit-stable run to
    // run) and applies the layer's epilogue.  The launcher picks ksplit; ws_floats = capacity of ws (0: never split).
    float* ws; size_t ws_floats; int ksplit; size_t ws_slice;
    // fp16 activation storage (srt_config.precision == SRT_PREC_F16): the tensors behind srcA / srcB (in16) and outRaw / outAct
    // (out16) hold IEEE halves instead of floats - same planar layout, same strides IN ELEMENTS, half the HBM bytes.  The
    // pointers keep their float type in this struct; kernels that honour the flags reinterpret them.
    int in16, out16;
    // Large fp16-storage batches (round 6, srt_nn5.hip): the tensors between down2 and up5 are channel-interleaved by eight ("C8": element (c, y, x) at
    // ((c/8) H W + y W + x) 8 + c % 8 - the B-fragment layout of the fp16 MFMA, so patches go HBM -> LDS by DMA alone).  c8out: srt_enc_f16 (down2: planar
    // input) stores its raw + act outputs in that form.  wpack16cs: up5's class-stacked fp16 weights [Cin/16][15][2][32][8] (srt_pack16_classstack_kernel).
    int c8out;
    int c8srcB;           // up6 (srt_nn.hip): srcB = up5's output holds its 16 channels C8 (two groups of 8) instead of planar
    int c8srcA;           // ... and so does srcA, down1's raw skip tensor (batches whose down1 runs on the streamed kernels: srt_down1_c8_ok)
    const uint16_t* wpack16cs; size_t wpack16cs_stem;
    float* outRaw;        // encoder: conv+bias (the skip tensor AND the next encoder layer's input); decoder: unused
    float* outAct;        // decoder: bn(act(v)); encoder: unused (the BN + activation is applied by the consumer)
    size_t out_stem, out_tile;
    int act;              // activation kind of the stems whose elu_mask bit is clear (encoder: LeakyReLU, decoder: ReLU)
    unsigned elu_mask;    // bit s set: stem s of this launch uses ELU (stemMode != 0, spleeter.c:130-139)
    int variant;
};

struct SrtHeadParams {    // up7: 4x4 dilation-2 conv 1->2 channels + bias + sigmoid  (spleeter.c:156,295-300)
    int H, W, ntiles, nstems;
    const float* src; size_t src_stem, src_tile;
    const float* w; const float* bias; size_t coeff_stem;
    float* out; size_t out_stem, out_tile;    // [2][H][W] per instance
    int variant;
    int out16;            // the two mask planes leave as IEEE halves (same layout, strides in elements): the engine's own mask buffer between the network and the inverse
                          // transform of srtSeparate in the fp16 mode (srt_head_out16_ok); the masks srtForward hands to its caller are always floats
};
int  srt_head_out16_ok(const SrtHeadParams& p);      // the launch runs on srt_head_rows_kernel<.., 4, true>

// launchers (srt_nn.hip)
int  srt_launch_enc(const SrtConvParams& p, int impl, hipStream_t s);
int  srt_launch_dec(const SrtConvParams& p, int impl, hipStream_t s);
int  srt_launch_head(const SrtHeadParams& p, hipStream_t s);
int  srt_launch_up6_head(const SrtConvParams& p, const SrtHeadParams& h, const SrtSwitches& sw, hipStream_t s);   // both layers in one pass; 1: not covered / switched off
int  srt_launch_bn_act(const float* raw, int raw16, float* out, const float* scale, const float* shift, int C, size_t hw, int kind, int variant, hipStream_t s);
int  srt_launch_half_to_float(const void* src, float* dst, size_t n, hipStream_t s);
int  srt_launch_pack_enc(const float* w, float* wp, int Cin, int Cout, int CP, hipStream_t s);
int  srt_launch_pack_dec(const float* w, float* wp, int Cin, int Cout, int CP, hipStream_t s);
// v2 kernels (srt_nn2.hip): return 1 when the layer geometry is not covered (caller falls back to the v1 kernels)
int  srt_launch_enc2(const SrtConvParams& p, const SrtSwitches& sw, hipStream_t s);
int  srt_launch_down1_f16(const SrtConvParams& p, hipStream_t s);   // fp16 mode, C8 outputs: down1 on the fp16 MFMA, p.stack = 1..6 stems in one launch (1: not covered)
int  srt_down1_c8_ok(int H, int W, int ntiles, size_t out_stem, const SrtSwitches& sw);   // fp16 storage: down1 of this batch runs on the streamed kernels, which can write raw1 / act1 C8
int  srt_launch_dec2(const SrtConvParams& p, hipStream_t s);
int  srt_launch_pack_stemstack(const float* coeff_w0, size_t coeff_stem, int nstems, float* wp2, int Cin, int Cout, int CP2, hipStream_t s);
int  srt_launch_pack_classstack(const float* w, float* wp2, int Cin, int Cout, hipStream_t s);
// fp16-MFMA kernels (srt_nn3.hip): return 1 when the layer is not covered (caller uses the fp32 kernels)
int  srt_launch_enc_f16(const SrtConvParams& p, hipStream_t s);
int  srt_launch_dec_f16(const SrtConvParams& p, hipStream_t s);
int  srt_launch_pack16(const float* w, uint16_t* wp16, int Cin, int Cout, int CP, int dec, hipStream_t s);
// C8-form fp16 kernels (srt_nn5.hip): return 1 when the layer is not covered
int  srt_launch_enc_c8(const SrtConvParams& p, const SrtSwitches& sw, hipStream_t s);
int  srt_launch_dec_c8(const SrtConvParams& p, const SrtSwitches& sw, hipStream_t s);
int  srt_launch_pack16_classstack(const float* w, uint16_t* wp, int Cin, int Cout, hipStream_t s);
int  srt_launch_c8_to_float(const void* src, float* dst, int C, size_t hw, hipStream_t s);
int  srt_launch_count_not_fp16(const float* w, size_t n, unsigned* d_count, hipStream_t s);   // weights the fp16 pack would round (SRT_PREC_F16X2 guard)
int  srt_set_sigmoid_table(const float* tbl1026);
void srt_fp16_expand(const uint16_t* d_in, float* d_out, size_t n, hipStream_t s);
// Winograd decoder kernels (srt_nn4.hip): U = transformed weights [Cin/4][Cout/16][4][16][52] per stem; the launcher returns 1
// when the layer is not covered.  srt_wino_mask(): bit i set = up(i+1) runs this form (large batches, fp32 MFMA path).
int  srt_launch_pack_wino(const float* w, float* u, int Cin, int Cout, hipStream_t s);
int  srt_launch_dec_wino(const SrtConvParams& p, const float* U, size_t u_stem, const SrtSwitches& sw, hipStream_t s);
// encoder layers in Winograd form (srt_nn4.hip, srt_enc_wino32): U from the OIHW weights; the layer reads act(BN(raw)) of its input (srcA) and
int srt_enc_producer_copy();          // tuning builds: SRT_TUNE=...,enccopy=0 keeps the separate bn+act pass in front of the first Winograd-form encoder layer
// writes raw (outRaw) + optionally its own act(BN(.)) copy (outAct with bnScale / bnShift).  srt_enc_wino_covers: geometry test of the launcher.
int  srt_launch_pack_wino_enc(const float* w, float* u, int Cin, int Cout, hipStream_t s);
int  srt_launch_enc_wino(const SrtConvParams& p, const float* U, size_t u_stem, hipStream_t s);
int  srt_enc_wino_covers(int Cin, int Cout, int H, int W);
int  srt_launch_bn_act_batch(const float* raw, float* out, const float* scale, const float* shift, size_t coeff_stem, int nstems, int ntiles, int C, size_t hw,
                             int act, unsigned elu_mask, int variant, hipStream_t s);
int  srt_wino_mask();
int  srt_wino_force();

// DSP launchers (srt_dsp.hip)
struct SrtDspTables { const float* preWin; const float* postWin; const float2* twiddle; };
struct SrtStftParams {
    const float* L; const float* R; size_t nsamples;
    int frames_computed;      // frames that get an FFT (tail frame zero padded); rows beyond are zero
    int rows_total;           // rows to write (>= frames_computed): spectrum + magnitude rows (zero filled)
    float2* spec;             // [2][spec_rows][SRT_SPEC_LD]
    size_t spec_ch_stride;    // float2 elements between channels
    float* mag;               // [ntiles][2][T][F] or nullptr
    int T, F;
    SrtDspTables tab;
};
struct SrtIstftParams {
    const float2* spec; size_t spec_ch_stride;
    int frames;               // rows to synthesise
    const float* masks;       // [nstems][ntiles][2][T][F] or nullptr (all-ones)
    int masks16;              // the masks are halves (srt_istft_ola3_kernel<.., M16>: F <= 1024, no ratio); see SrtHeadParams::out16
    int nstems, ntiles, T, F;
    float oob[SRT_MAX_STEMS];
    int ratio;                // 1: masks are normalised across the stems while they are applied, m_s^2 / sum_j m_j^2 (srt_config.ratio_mask; needs masks of ALL nstems)
    float* frames_out;        // [nstems][2][frames][4096] windowed time frames (temp)
    float* out;               // [nstems][2][out_len]
    size_t out_len;           // frames*1024 + 3072
    SrtDspTables tab;
    const float* ext;         // average mask extension (srtSetMaskExtension): gains of bins >= F, [nstems][..][frames][2] with ext_stem floats between stems, written by
    size_t ext_stem;          // srt_launch_mask_ext from the same masks / ratio / overlap; nullptr: the constant rule (oob).  Batch: indexed by packed row
    // stem remix (srtSetMix): n_out > 0 - the launch writes n_out pairs [n_out][2][out_len] instead of nstems; output m applies the gain
    // h = mix[m][nstems], then h = fmaf(mix[m][s], g_s, h) for s ascending, g_s = the gain stem s would get (the srt_istft_ola*_mix_kernel forms).  0: off
    int n_out;
    float mix[SRT_MAX_STEMS][SRT_MAX_STEMS + 1];
};
// average mask extension: ext[s][r][c] = mean over k < F of the in-band gain the inverse transform applies to stem s, row r, channel c
struct SrtMaskExtParams {
    const float* masks;       // as SrtIstftParams::masks (never null), halves with masks16
    int masks16, nstems, ntiles, T, F;
    int rows;                 // rows to fill (batch: every packed row)
    int ratio;                // as SrtIstftParams::ratio
    float* ext; size_t ext_stem;
};
int srt_launch_mask_ext(const SrtMaskExtParams& p, hipStream_t s, int overlap = 0, const float* seam = nullptr);      // seam: as srt_launch_istft (the table of a piece)
// overlap > 0 (srtSetOverlap): consecutive network tiles share `overlap` rows - p.mag / p.masks are in the overlapped layout of ov_tiles / p.ntiles =
// srtOverlapTiles(rows) tiles and the kernels' overlap instantiations run; 0: the back-to-back layout and the kernels as they always were
int srt_launch_stft(const SrtStftParams& p, hipStream_t s, int overlap = 0, int ov_tiles = 0);
// seam (with overlap > 0 and float masks): the signal is a piece of a longer stream and `seam` the mask seam carry [nstems][2][overlap][F] of the piece before it
// (srt_launch_mask_seam_save) - the SEAM instantiations run, whose first `overlap` rows blend with the carry; nullptr: a whole signal, the kernels as they were
int srt_launch_istft(const SrtIstftParams& p, hipStream_t s, int overlap = 0, const float* seam = nullptr);
// rows [T - overlap, T) of the last of ntiles tiles of every stem and channel of masks [nstems][ntiles][2][T][F] (floats) -> seam [nstems][2][overlap][F]
int srt_launch_mask_seam_save(const float* masks, int nstems, int ntiles, int T, int F, int overlap, float* seam, hipStream_t s);
// packed batch of independent tracks (srtSeparateBatch): one row of the device-resident track table per track
struct SrtBatchTrack {
    const float* L; const float* R; size_t n;    // the track's PCM, n >= 4096 samples
    float* out; size_t out_len;                  // its stems [nstems][2][out_len], out_len = rows * 1024 + 3072
    int frames, rows;                            // srtStftFrames(n), srtStftRows(n)
    int tile0, ntiles;                           // packed tiles [tile0, tile0 + ntiles), ntiles = srtOverlapTiles(rows, T, O) = ceil(rows / T) at O = 0 (spectrum rows from tile0 * T)
    int wg_stft, wg_istft;                       // the track's first workgroup of the batched STFT / first run of the batched inverse (srt_batch_geometry)
};
struct SrtBatchGrid { int fpb, stft_blocks, G, istft_runs; };
int srt_batch_geometry(SrtBatchTrack* t, int ntracks, int T, int F, int nstems, SrtBatchGrid* g);       // host: fills wg_stft / wg_istft
// p as srt_launch_stft / srt_launch_istft on the packed buffers (mag required; p.ntiles = the packed tile count); the per-track fields are taken from d_tracks
// overlap > 0 (srtSeparateBatchOverlap): every track's magnitudes / masks are in the overlapped layout inside its own tiles, the table's ntiles =
// srtOverlapTiles(rows, T, overlap); the overlap is an argument of its own, as in srt_launch_stft / srt_launch_istft.  0: the kernels as they always were
int srt_launch_stft_batch(const SrtStftParams& p, const SrtBatchTrack* d_tracks, int ntracks, const SrtBatchGrid& g, hipStream_t s, int overlap = 0);
int srt_launch_istft_batch(const SrtIstftParams& p, const SrtBatchTrack* d_tracks, int ntracks, const SrtBatchGrid& g, hipStream_t s, int overlap = 0);
// the stem remix per track (srtSeparateBatchMix): p.n_out outputs per track, g from srt_batch_geometry with n_out in place of nstems; track k's matrix
// [n_out][nstems + 1] (srtSetMix's layout) at d_gains + k * n_out * (nstems + 1) in device memory.  p.masks: floats, required; p.mix is not read
int srt_launch_istft_batch_mix(const SrtIstftParams& p, const SrtBatchTrack* d_tracks, const float* d_gains, int ntracks, const SrtBatchGrid& g, hipStream_t s, int overlap = 0);
// the gain table of the average mask extension over the packed rows of such a batch (p.rows = p.ntiles * T packed rows; rows past a track's own are left alone)
int srt_launch_mask_ext_batch(const SrtMaskExtParams& p, const SrtBatchTrack* d_tracks, int ntracks, hipStream_t s, int overlap);

// residual chain of the offline CLI (main.c:845-866): res = spec - spec*mask (bins >= F: spec - spec*oob), |res|*4096 -> mag
struct SrtResidualParams {
    const float2* spec; float2* res; size_t spec_ch_stride;
    int rows, T, F;
    const float* mask;        // ONE stem: [ntiles][2][T][F]
    float oob;
    float* mag;               // [ntiles][2][T][F]
};
int srt_launch_residual(const SrtResidualParams& p, hipStream_t s);
// out[c][i] = (i < na ? a[c][i] : 0) - b[c][i] for lo <= i < min(hi, nb), two channels of plane length nb (time-domain residual, main.c:794-798, 924-928)
int srt_launch_time_residual(const float* aL, const float* aR, size_t na, const float* b, size_t nb, float* out, size_t lo, size_t hi, hipStream_t s);
// chunk stitching on the device: out[p][0:3072] += carry[p] (unless first), then carry[p] = out[p][tail : tail+3072] (unless last)
int srt_launch_carry(float* out, size_t plane_len, int nplanes, size_t tail, float* carry, int first, int last, hipStream_t s);
// 16-bit PCM at the host-stream boundary (srt_pcm.hip).  unpack: interleaved stereo int16 [n][2] -> planar fp32, x = q / 32768.
// pack: pair p's planes at planes + 2p * plane_stride (L) and + (2p + 1) * plane_stride (R), samples [0, count) -> out + p * out_stride * 2 as [count][2],
// q = clamp(rint(x * 32768)), NaN -> 0; clipped (may be NULL) [pairs]: the samples whose unclamped value fell outside the range are ADDED, through `scratch`
// (srt_pcm16_pack_scratch(pairs) 64-bit words the launch may overwrite; unused without `clipped`).  Any alignment: unaligned arguments take the frame-by-frame path.
int srt_launch_pcm16_unpack(const int16_t* in, size_t n, float* L, float* R, hipStream_t s);
size_t srt_pcm16_pack_scratch(int pairs);
int srt_launch_pcm16_pack(const float* planes, size_t plane_stride, int pairs, size_t count, int16_t* out, size_t out_stride,
                          unsigned long long* clipped, unsigned long long* scratch, hipStream_t s);
// ... packed 24-bit: [n][2][3] bytes, x = q / 2^23; the pack writes pair p at out + p * out_stride * 6, q = clamp(rint(x * 2^23)); clipped and
// scratch as above.  ... and the 16-bit pack with TPDF dither: q = clamp(rint(x * 32768 + d)), d of (seed, 2 (first_pair + p) + channel, first_index + i)
int srt_launch_pcm24_unpack(const uint8_t* in, size_t n, float* L, float* R, hipStream_t s);
int srt_launch_pcm24_pack(const float* planes, size_t plane_stride, int pairs, size_t count, uint8_t* out, size_t out_stride,
                          unsigned long long* clipped, unsigned long long* scratch, hipStream_t s);
int srt_launch_pcm16_pack_dither(const float* planes, size_t plane_stride, int pairs, size_t count, int16_t* out, size_t out_stride,
                                 unsigned long long* clipped, unsigned long long* scratch, unsigned long long seed, int first_pair, unsigned long long first_index, hipStream_t s);
// cross-stem ratio mask, in place on [nstems][count]: m_s <- (m_s^2 + eps/S) / (sum_j m_j^2 + eps)
int srt_launch_ratio_mask(float* masks, int nstems, size_t count, hipStream_t s);

// multichannel Wiener filter (srt_wiener.hip; norbert.wiener(v, x, n) as official Spleeter's --mwf runs it), in spectrum units: every x of the
// specification is 4096 * spec, which moves the scale into the epsilon terms (see the kernel file's header).
#define SRT_WIENER_MAX_ITERS 3
#define SRT_WIENER_MAX_CHUNKS 256    // row chunks of the statistics pass: partial sums per chunk, summed in chunk order by the finalize kernel
#define SRT_WIENER_BINBLK 9          // 256-bin blocks that cover bins 0..2048 (the first pass also takes max |x| over all of them)
struct SrtWienerParams {
    const float2* spec; size_t spec_ch_stride;   // [2][rows][SRT_SPEC_LD]
    int rows;
    const float* masks;                          // fp32 [nstems][ntiles][2][T][F], ntiles = ceil(rows / T)
    int nstems, ntiles, T, F;
    int nchunks, rpc;                            // row chunks of the statistics pass and rows per chunk
    float* slab;                                 // [SRT_WIENER_MAX_CHUNKS][nstems][4][F] per-chunk partial sums
    float* slab_max;                             // [SRT_WIENER_MAX_CHUNKS][SRT_WIENER_BINBLK] per-block max |spec|
    float* rtab;                                 // [SRT_WIENER_MAX_ITERS][nstems][F][4]: R_j (R00, R11, Re R01, Im R01)
    float* wsum;                                 // [SRT_WIENER_MAX_ITERS][nstems][F]: sum over rows of v_j, spectrum units
    float* scal;                                 // [0]: norbert's a = max(1, max |x| / 10)
    float2* out; size_t out_stem;                // filter: stem j's spectrum at out + j * out_stem, [2][rows][SRT_SPEC_LD]
};
int srt_launch_wiener_stats(const SrtWienerParams& p, int pass, hipStream_t s);      // pass 1..n: statistics of the estimates after pass - 1 iterations
int srt_launch_wiener_finalize(const SrtWienerParams& p, int pass, hipStream_t s);   // R tables of that pass (and a, pass 1)
// srt_launch_wiener_stats for rows [row0, row0 + nrows) of a signal held one piece at a time (srtSeparateHostWiener): p.spec / spec_ch_stride / masks / ntiles are
// the PIECE's (its row 0 is the signal's row0), p.rows / rpc / nchunks the whole signal's.  Chunks that straddle a piece boundary continue from their slab slots, so
// after the pieces have been launched in row order on one stream the slab (and slab_max) holds what one srt_launch_wiener_stats over the signal leaves, bit for bit.
int srt_launch_wiener_stats_seg(const SrtWienerParams& p, size_t row0, size_t nrows, int pass, hipStream_t s);
int srt_launch_wiener_filter(const SrtWienerParams& p, int iters, hipStream_t s);    // W_j x after `iters` iterations for every stem; bins >= F copied
// The filter with per-call options (srtIstftWienerEx / srtSeparateWiener).  p as above, except that with overlap > 0 p.masks is in the
// overlapped layout and p.ntiles = srtOverlapTiles(rows, T, overlap) (the masks' stem stride, and the count srt_ov_row clamps the primary tile with).
struct SrtWienerOpt {
    int overlap;                                 // rows consecutive network tiles share, 0: back-to-back tiles
    const float* ext; size_t ext_stem;           // average mask extension: stem j's gain of bins >= F at ext[j * ext_stem + row * 2 + channel] (srt_launch_mask_ext); nullptr: oob
    float oob[SRT_MAX_STEMS];                    // the constant rule: stem j's gain of bins >= F
    int n_out;                                   // 0: every stem's spectrum; 1..nstems: the mixes, output m at p.out + m * p.out_stem
    float mix[SRT_MAX_STEMS][SRT_MAX_STEMS + 1]; // srtSetMix's layout: G[m][j] the gain of stem j in output m, G[m][nstems] the gain of the input
};
// the statistics pass on blended masks (overlap > 0 only: at 0 the kernel above runs); finalize is srt_launch_wiener_finalize
int srt_launch_wiener_stats_ov(const SrtWienerParams& p, int overlap, int pass, hipStream_t s);
// the filter with any option on: the FINAL spectrum of every bin 0..2048 - in band y_j or the mix of the y_j, above F the gain (q.oob, q.ext or their chain
// through the matrix) times the input - of q.n_out outputs, or of every stem; the inverse transform that follows applies no gain
// seam (with q.overlap > 0): p describes the rows a piece of a longer stream owns (srtSeparateHostWienerOverlap) - p.rows of the p.spec_ch_stride / SRT_SPEC_LD rows its
// spectrum holds, under p.ntiles tiles - and `seam` is the mask seam carry [nstems][2][overlap][F] of the piece before it; nullptr: a whole signal, or the stream's first piece
int srt_launch_wiener_filter_opt(const SrtWienerParams& p, const SrtWienerOpt& q, int iters, hipStream_t s, const float* seam = nullptr);
// srt_launch_wiener_stats_seg on a piece's overlapped tiles (overlap > 0): rows [row0, row0 + nrows) are the rows the piece owns, masks fetched as srt_launch_wiener_stats_ov
// fetches them on piece-local rows, the first `overlap` of them blended with `seam` as above.  After the pieces in row order the slab holds what one
// srt_launch_wiener_stats_ov over the signal leaves, bit for bit.
int srt_launch_wiener_stats_seg_ov(const SrtWienerParams& p, int overlap, const float* seam, size_t row0, size_t nrows, int pass, hipStream_t s);
// The filter per track of a packed batch (srtSeparateBatchWiener): a second device table beside SrtBatchTrack's, one row per track - the track's row chunks of
// the statistics pass (wiener_issue's rule on the track's own rows) as a run [chunk0, chunk0 + nchunks) of the call's global chunk numbering.
struct SrtBatchWiener { int chunk0, nchunks, rpc, tab; };     // tab: the track's slot in the per-track tables (its index in the call)
int srt_batch_wiener_geometry(const SrtBatchTrack* t, SrtBatchWiener* w, int ntracks);      // host: fills every row; returns the call's chunk total
// p on the packed buffers: spec / spec_ch_stride / masks as the batched transforms see them, ntiles = the packed tile count (the masks' stem stride), rows =
// ntiles * T, nchunks = the call's chunk total (rpc unused); slab [nchunks][nstems][4][F], slab_max [nchunks][SRT_WIENER_BINBLK]; rtab / wsum / scal: slot 0 of
// the per-track tables [slots][SRT_WIENER_MAX_ITERS][nstems][F][4] / [slots][SRT_WIENER_MAX_ITERS][nstems][F] / [slots]; out: [nstems][2][rows][SRT_SPEC_LD].
// A track's statistics cover its own rows [0, rows_k) only, so its tables are those of the single-signal launches on it alone, bit for bit.
int srt_launch_wiener_stats_batch(const SrtWienerParams& p, const SrtBatchTrack* d_tracks, const SrtBatchWiener* d_wt, int ntracks, int pass, hipStream_t s);
int srt_launch_wiener_finalize_batch(const SrtWienerParams& p, const SrtBatchWiener* d_wt, int ntracks, int pass, hipStream_t s);
int srt_launch_wiener_filter_batch(const SrtWienerParams& p, const SrtBatchTrack* d_tracks, const SrtBatchWiener* d_wt, int ntracks, int iters, hipStream_t s);
// The per-track filter with per-call options (srtSeparateBatchWienerEx): SrtWienerOpt's fields for a packed batch.  The matrices do not travel
// by value - every track has its own - so the launch takes the device gain table (srt_launch_istft_batch_mix's d_gains); ext is indexed by packed row.
struct SrtBatchWienerOpt {
    int overlap;                                 // rows consecutive tiles of one track share (one value for the call: the packing depends on it), 0: back-to-back
    const float* ext; size_t ext_stem;           // as SrtWienerOpt, written by srt_launch_mask_ext[_batch] over the packed rows; nullptr: oob
    float oob[SRT_MAX_STEMS];
    int n_out;                                   // 0: every stem's spectrum; 1..nstems: the mixes
    const float* gains;                          // n_out > 0: track k's matrix [n_out][nstems + 1] at gains + k * n_out * (nstems + 1), device memory
};
// the statistics pass on blended masks per track (overlap > 0 only; the table's ntiles = srtOverlapTiles(rows, T, overlap)); finalize is srt_launch_wiener_finalize_batch
int srt_launch_wiener_stats_batch_ov(const SrtWienerParams& p, const SrtBatchTrack* d_tracks, const SrtBatchWiener* d_wt, int ntracks, int overlap, int pass, hipStream_t s);
// the filter with any option on: final spectra of q.n_out outputs, or of every stem, over the packed rows; the batched inverse behind it applies no gain
int srt_launch_wiener_filter_batch_opt(const SrtWienerParams& p, const SrtBatchWienerOpt& q, const SrtBatchTrack* d_tracks, const SrtBatchWiener* d_wt, int ntracks, int iters, hipStream_t s);
// batched inverse of per-stem spectra (the filter's output): stem s of every track reads p.spec + s * stem_stride (float2 elements) at its packed rows, no masks
// (all-ones in band, p.oob[s] above F) - srt_launch_istft's single-stem, mask-free form for every (track, stem) in one launch
int srt_launch_istft_batch_spec(const SrtIstftParams& p, size_t stem_stride, const SrtBatchTrack* d_tracks, int ntracks, const SrtBatchGrid& g, hipStream_t s);
struct srt_engine;
int srt_engine_wiener(const srt_engine* e);                                             // iterations switched on (srtSetWiener), 0: off
int srt_engine_overlap(const srt_engine* e);                                            // rows consecutive network tiles share (srtSetOverlap), 0: off
int srt_engine_mix(const srt_engine* e);                                                // outputs of the stem remix (srtSetMix), 0: off

// streaming (srt_dsp.hip kernels, srt_stream.hip host logic): one hop = 1 forward + n_stems masked inverse FFTs + 50 % OLA
struct SrtStreamHop {
    const float* ring;        // [2][4096] device copy of the input ring buffer
    int inPos;                // ring read origin (Spleeter4Stems.c:262)
    float2* specRow;          // [2 ch] rows of the spectrum buffer for this cursor: L at specRow, R at specRow + specChStride
    size_t specChStride;
    float* magRow;            // [2 ch] magnitude rows: L at magRow, R at magRow + magChStride
    size_t magChStride;
    const float* maskRow;     // stem s, channel c at maskRow + s*maskStemStride + c*maskChStride
    size_t maskStemStride, maskChStride;
    int F;
    int nstems;               // stems inverted per hop (one workgroup each), 1..SRT_MAX_STEMS
    float oob[SRT_MAX_STEMS]; // per stem: weight of bins F..2048 (the plugin: 0.25, 0, 0.25, 0.25)
    float* overlap;           // [2*nstems][1024]
    float* out;               // [1024][2*nstems] interleaved segment
    const float* analysisWnd; const float* synthesisWnd; const float2* twiddle;
};
int srt_launch_stream_hop(const SrtStreamHop& p, hipStream_t s);
// the hop inverse of a live stream with the stem remix and / or the average mask extension (srtLiveCreateEx): one workgroup per output
struct SrtLiveCombineHop {
    const float2* specRow; size_t specChStride;                               // as SrtStreamHop
    const float* maskRow; size_t maskStemStride, maskChStride;
    int F, nstems;
    int n_out;                // outputs (workgroups), 1..SRT_MAX_STEMS
    float oob[SRT_MAX_STEMS]; // gain of stem s above F under the constant rule
    const float* ext;         // average extension: stem s, channel c of the frame's row at ext[s * extStemStride + c]; nullptr: the constant rule
    size_t extStemStride;
    float gain[SRT_MAX_STEMS][SRT_MAX_STEMS + 1];                             // G[m][s], G[m][nstems] = the unmasked input (srtSetMix's layout)
    float* overlap;           // [2*n_out][1024]
    float* out;               // [1024][2*n_out] interleaved segment
    const float* synthesisWnd; const float2* twiddle;
};
int srt_launch_live_combine_hop(const SrtLiveCombineHop& q, const SrtStreamHop& p, hipStream_t s);
// Live window gather: dst[c][i] = ring[c][(i + rot) mod T] for the [2][T][F] magnitude ring (rows of F floats, F % 4 == 0)
int srt_launch_live_gather(const float* ring, float* dst, int T, int F, int rot, hipStream_t s);
// the hop inverse of a live stream with the Wiener filter (srtLiveCreateWiener): one workgroup per output; the prologue runs the filter's chain for
// every stem at the thread's nine bins from the joined run's tables and forms the output's spectrum (in band the remix chain of the filtered stems, above F the
// combining inverse's gain chain times the input)
struct SrtLiveWienerHop {
    const float2* specRow; size_t specChStride;                               // the DELAYED frame's row: L at specRow, R at specRow + specChStride
    const float* maskRow; size_t maskStemStride, maskChStride;                // as SrtStreamHop
    int F, nstems;
    int n_out;                // outputs (workgroups), 1..SRT_MAX_STEMS
    int iters;                // 1..SRT_WIENER_MAX_ITERS
    const float4* rtab;       // the joined run's R tables [iters][nstems][F] (SrtWienerParams::rtab)
    const float* scal;        // ... and its a (SrtWienerParams::scal)
    float oob[SRT_MAX_STEMS];
    const float* ext; size_t extStemStride;                                   // as SrtLiveCombineHop; nullptr: the constant rule
    float gain[SRT_MAX_STEMS][SRT_MAX_STEMS + 1];                             // as SrtLiveCombineHop (without a mix: the identity)
    float* overlap;           // [2*n_out][1024]
    float* out;               // [1024][2*n_out] interleaved segment
    const float* synthesisWnd; const float2* twiddle;
};
int srt_launch_live_wiener_hop(const SrtLiveWienerHop& q, const SrtStreamHop& p, hipStream_t s);      // p: the forward transform's fields, as srt_launch_live_combine_hop
// Live spectrum-window gather: dst[c][i] = ring[c][(i + rot) mod R] for i < T, rows of SRT_SPEC_LD complex values; ring [2][R][SRT_SPEC_LD], dst [2][T][SRT_SPEC_LD], T <= R
int srt_launch_live_spec_gather(const float2* ring, float2* dst, int T, int R, int rot, hipStream_t s);
struct srt_config;
// srtCreate's argument checks (no HIP call): 0, or the negative code with srtLastError() set and `who` naming the caller
int srt_check_config(const srt_config* cfg, const char* who);

// ---- multi-device host driver (srt_multi.hip) over the engine (srt_engine.hip)
struct srt_engine;
// One tile RANGE of a longer host-resident stream through engine `e` (chunked, copies overlapped with compute): h_out points at the range's first
// output sample inside planes of out_stride floats; h_tail (may be null: last range) receives the range's last 3072 samples per plane - the overlap-add
// contribution to the next range's first samples; head: a previous range will add its tail to this range's first 3072 samples.  cli_stems 0 | 2 | 3.
int srt_engine_host_range(srt_engine* e, const float* h_L, const float* h_R, size_t n, size_t frames, size_t rows, float* h_out, size_t out_stride,
                          float* h_tail, bool head, unsigned flags, int cli_stems);
const float* srt_engine_coeff_device(const srt_engine* e, int stem);      // the stem's fp32 spleeterCoeff blob in the engine's HBM (valid after srtSetCoeff*)
int srt_engine_device(const srt_engine* e);
void* srt_engine_stream(const srt_engine* e);
