/*
 * spleeterrt_amd.h — device-resident C ABI of the MI355X separation engine (libspleeterrt_amd.so).
 *
 * Plain C, no torch / HIP types in the signatures: `stream` is a hipStream_t passed as void*, every `d_*`
 * pointer is a device (HBM) address, every `h_*` pointer is host memory.  All functions return 0 on success
 * and a negative code on failure (srtLastError() gives the text); nothing here ever falls back to a CPU path.
 *
 * This is the batched, HBM-resident form of the reference's per-tile calls.  What each entry point replaces
 * (file:line under the reference tree):
 *   srtCreate / srtDestroy      allocateSpleeterStr + initSpleeter + freeSpleeter   Executable/spleeter.c:111-176,310-320
 *                               and InitSTFT / FreeSTFT                             Executable/stftFix.c:302-362
 *   srtSetCoeff*                the borrowed `coeff` argument of initSpleeter        Executable/spleeter.c:129
 *                               / lib2stem_loadCoefficients (fp16 container)         Executable/main.c:423-443
 *   srtForward                  processSpleeter for nstems x ntiles tiles at once    Executable/spleeter.c:177-301
 *   srtStft                     stft + the magnitude loop of processMT               Executable/stftFix.c:363-495, main.c:462-471
 *   srtIstft                    the mask loop of processMT + istft                   Executable/main.c:473-494, stftFix.c:496-579
 *   srtSeparate                 main()'s stft -> processMT -> istft sequence         Executable/main.c:776-785
 *   srtSeparateCli              main()'s two- and three-output flows incl. residuals  Executable/main.c:776-798, 845-928
 * The drop-in, host-pointer forms with the reference's exact signatures are in spleeter.h / stftFix.h.
 */
#ifndef SPLEETERRT_AMD_H
#define SPLEETERRT_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SRT_API __attribute__((visibility("default")))
#define SRT_MAX_STEMS 8
#define SRT_VARIANT_EXE 0   /* LUT sigmoid + ELU clamp  (Executable/spleeter.c:29-56) */
#define SRT_VARIANT_VST 1   /* exact sigmoid, plain ELU (VST/Source/spleeter.c:56-77) */
#define SRT_IMPL_MFMA   0   /* MFMA implicit-GEMM kernels (product path) */
#define SRT_IMPL_NAIVE  1   /* one-thread-per-output HIP kernels (debug cross-check, still GPU) */
#define SRT_PREC_F32    0   /* v_mfma_f32_32x32x2_f32: exact fp32 products (default; the headline path) */
#define SRT_PREC_F16    1   /* v_mfma_f32_32x32x16_f16, activations rounded to fp16 (BASELINE configs[4]; mask tolerance 2e-2).  Large batches: the network's input
                             * magnitudes are rounded to halves too (saturating at 65504, ~60x what full-scale PCM gives), and srtSeparate keeps its own masks as halves;
                             * STFT / iSTFT and every mask handed to a caller stay fp32 */
#define SRT_PREC_F16X2  2   /* same MFMA, activations split hi+lo: products exact in fp32 BECAUSE the weights are fp16 values - srtSetCoeff* checks
                             * every conv weight of the blob and refuses (-5, srtLastError names the count) one that the fp16 pack would round, e.g. a raw
                             * fp32 .dat blob with 24-bit mantissas: nothing is rounded silently in this mode */

typedef struct srt_engine srt_engine;

typedef struct srt_config {
    int   F;                        /* analyseBinLimit: tile width in bins, multiple of 64, <= 2048   main.c:701 */
    int   T;                        /* timeStep: tile height in frames, multiple of 64                main.c:702 */
    int   n_stems;                  /* sub-networks evaluated per tile, 1..SRT_MAX_STEMS */
    int   stem_mode[SRT_MAX_STEMS]; /* 0: LeakyReLU/ReLU, !=0: ELU/ELU                                spleeter.c:130-139 */
    float oob_weight[SRT_MAX_STEMS];/* weight of bins F..2048 ("unaffectedWeight" = 0.1)              main.c:773; ignored under SRT_MASK_EXT_AVERAGE */
    int   variant;                  /* SRT_VARIANT_* */
    int   max_tiles;                /* capacity: tiles per batch */
    int   impl;                     /* SRT_IMPL_* */
    int   precision;                /* SRT_PREC_*: arithmetic of the conv contraction (accumulation and everything else is fp32) */
    int   ratio_mask;               /* 0 (reference behaviour: raw sigmoid masks) | 1: srtSeparate / srtSeparateEx / srtSeparateHostStream normalise
                                     * m_s^2 / sum_j m_j^2 across stems (README.MD:82-85).  The CLI flows (srtSeparateCli*) reject it: their
                                     * sub-networks run one after the other on different inputs, so there is no stem axis to normalise over. */
    int   batch_invariant;          /* 0 (default): the fastest kernel per launch - small launches (<= 16 instances) cut the deep layers' K loops
                                     * into slices (split-K) and keep the direct kernels, larger ones run up1..up5 and down3..down6 in Winograd form, so the
                                     * same tile can differ in the last bits (<= 2e-5 on masks) with the batch it is evaluated in.
                                     * 1: kernel choice by layer geometry only, no split-K: a tile's result is bit-identical whatever the batch
                                     * size, tile slot, stem range or rank partition (what the reference's CPU path guarantees); small batches
                                     * run slower.  The environment variable SPLEETERRT_BATCH_INVARIANT=1 forces it for every engine. */
} srt_config;

SRT_API int  srtCreate(const srt_config *cfg, void *stream, srt_engine **out);
SRT_API void srtDestroy(srt_engine *e);
SRT_API const char *srtLastError(void);
SRT_API size_t srtCoeffBytes(void);                                           /* == getCoeffSize() == 39 290 900 */

/* weights for one sub-network, layout of spleeterCoeff (spleeter.h).  The data is copied; nothing is borrowed. */
SRT_API int  srtSetCoeffHost(srt_engine *e, int stem, const void *h_coeff);
SRT_API int  srtSetCoeffDevice(srt_engine *e, int stem, const void *d_coeff);
SRT_API int  srtSetCoeffFp16Host(srt_engine *e, int stem, const uint16_t *h_halfs);   /* spleeterQuantizedSubNet */
SRT_API int  srtGetCoeffHost(srt_engine *e, int stem, void *h_coeff);                 /* read the stored fp32 blob back (srtCoeffBytes() bytes): tests of the fp16 expansion */

/* d_mag: [ntiles][2][T][F] magnitudes; d_masks: [n_stems][ntiles][2][T][F] */
SRT_API int  srtForward(srt_engine *e, const float *d_mag, int ntiles, float *d_masks);

/* the same for sub-networks [stem0, stem0+nstems) only; d_masks keeps the all-stem layout (stem s at s*ntiles*2*T*F) */
SRT_API int  srtForwardStems(srt_engine *e, const float *d_mag, int ntiles, float *d_masks, int stem0, int nstems);
/* in place on d_masks [n_stems][ntiles][2][T][F]: m_s <- (m_s^2 + 1e-10/S) / (sum_j m_j^2 + 1e-10)  (official-Spleeter ratio mask; not in the reference) */
SRT_API int  srtRatioMask(srt_engine *e, float *d_masks, int ntiles);

/* geometry helpers for an n-sample stereo signal (n >= 4096) */
SRT_API size_t srtStftRows(size_t n);            /* ceil(n/1024): rows the reference allocates          stftFix.c:367 */
SRT_API size_t srtStftFrames(size_t n);          /* rows that actually receive a transform              stftFix.c:378 */
SRT_API size_t srtIstftLength(size_t rows);      /* rows*1024 + 3072                                    stftFix.c:500 */

/* STFT of planar stereo PCM resident in HBM.  d_spec: [2][rows][2052] interleaved (re,im) with the reference's
 * conjugate convention; rows = srtStftRows(n).  d_mag (optional, may be NULL): [ceil(rows/T)][2][T][F]. */
SRT_API int  srtStft(srt_engine *e, const float *d_L, const float *d_R, size_t n, float *d_spec, float *d_mag);
/* d_masks: [n_stems][ntiles][2][T][F] (NULL = all-ones for bins < F; bins F..2048 always get oob_weight[stem]).  d_out: [n_stems][2][srtIstftLength(rows)] */
SRT_API int  srtIstft(srt_engine *e, const float *d_spec, size_t rows, const float *d_masks, float *d_out);
/* whole hot path, everything in HBM: PCM -> STFT -> |.| -> U-Nets -> mask -> iSTFT.  d_out as in srtIstft. */
SRT_API int  srtSeparate(srt_engine *e, const float *d_L, const float *d_R, size_t n, float *d_out);
/* Explicit-geometry forms for streams cut into tile ranges (shards / chunks): transform `frames` frames (frame i starts at
 * sample i*1024, zero padded past n) and emit `rows` >= frames rows (the extra rows are zero, as the reference's calloc). */
SRT_API int  srtStftEx(srt_engine *e, const float *d_L, const float *d_R, size_t n, size_t frames, size_t rows, float *d_spec, float *d_mag);
SRT_API int  srtSeparateEx(srt_engine *e, const float *d_L, const float *d_R, size_t n, size_t frames, size_t rows, float *d_out);

/* ---- overlapped network tiles with cross-faded masks.  By default a signal is cut into back-to-back tiles of T frames (the reference's
 * processMT): a frame next to a tile boundary sees zero padding where its neighbours should be, and the masks jump every T hops.  With an overlap of
 * O rows (0 <= O <= T/2) consecutive tiles of one signal share O rows: stride S = T - O, tile j covers spectrum rows [jS, jS + T), and a signal of `rows`
 * rows takes srtOverlapTiles(rows, T, O) tiles = 1 for rows <= T, else ceil((rows - O) / S) (rows of a tile past the signal's last row hold zero
 * magnitudes).  Row r has the primary tile j1 = min(r / S, tiles - 1) at offset k = r - j1 S; when j1 > 0 and k < O it is row k + S of tile j1 - 1 as
 * well, and its mask is a + w (b - a) with a from tile j1 - 1, b from tile j1 and w = (k + 1/2) / O; every other row takes its primary tile's mask.
 * With ratio_mask the blended masks are normalised (blend first); the fp16 mode's half masks are converted, then blended.
 * srtSetOverlap: per engine, off (0) by default, takes effect for later calls; -1 outside 0..T/2.  While it is on:
 *   srtStft / srtStftEx   write d_mag as [srtOverlapTiles(rows, T, O)][2][T][F] in that layout (d_spec is unchanged);
 *   srtForward            is unchanged (it takes any tile batch);
 *   srtIstft              reads d_masks [n_stems][srtOverlapTiles(rows, T, O)][2][T][F] in that layout and blends;
 *   srtSeparate[Ex]       compose the three; the signal must fit max_tiles OVERLAPPED tiles.
 * Refused with -1, an error text that says "overlap" and nothing written while O > 0: srtSeparateHostStream[Ex], srtSeparateCli, srtSeparateCliHost,
 * srtSeparateBatch (srtSeparateBatchOverlap takes an overlap of its own), srtMultiSeparate*Host, srtIstftWiener and srtSeparate[Ex] with the Wiener filter on.
 * O = 0 is the back-to-back path, bit for bit.
 * In graph mode the overlap is part of the captured call's key.
 * srtOverlapTiles is pure host arithmetic (no device, like srtBatchPlan): 0 for rows = 0; 0 with srtLastError() text for T < 1 or O outside 0..T/2. */
SRT_API int  srtSetOverlap(srt_engine *e, int overlap_rows);
SRT_API size_t srtOverlapTiles(size_t rows, int T, int overlap_rows);

/* ---- mask extension: the gain of the bins above the analysed band.  The networks see bins 0..F-1; by default every separation path multiplies
 * bins F..2048 of stem s by the constant oob_weight[s] (the reference's unaffectedWeight; official Spleeter's mask_extension = "zeros" is oob_weight = 0).
 * SRT_MASK_EXT_AVERAGE is official Spleeter's mask_extension = "average": bins F..2048 of spectrum row r, channel c of stem s are multiplied by
 *   e_s(r, c) = (sum over k < F of g_s(r, c, k)) / F,
 * g = the in-band gain the inverse transform really applies: the mask value (the fp16 mode's half masks converted), cross-faded when srtSetOverlap is on,
 * normalised across the stems when ratio_mask is on and n_stems > 1 - in that order.  fp32, one fixed summation order per F (a row of equal masks gives
 * exactly that value), a true division by F.  Without masks (srtIstft with d_masks = NULL: all-ones) e = 1.  oob_weight is IGNORED while the mode is on.
 * With ratio_mask the gains of the stems sum to 1 in every bin, so the stems then sum to the input over the whole band, not only below F.
 * srtSetMaskExtension: per engine, SRT_MASK_EXT_CONSTANT by default (the paths and kernels as they always were, bit for bit), takes effect for later calls;
 * switching to SRT_MASK_EXT_AVERAGE allocates the engine's gain table [n_stems][max_tiles * T][2] once (call it before capturing; kept until srtDestroy).
 * -1 with srtLastError() text for a null engine, an unknown mode, or the Wiener filter on.  Honoured by srtIstft, srtSeparate[Ex] (ratio_mask, srtSetOverlap, the
 * fp16 mode's half masks, graph mode: the mode is part of the captured call's key), srtSeparateBatch and srtSeparateHostStream[Ex|Io] (the gain is row-local:
 * chunk seams need nothing), and by engines borrowed from a multi-device object.  Refused with -1 while the mode is on: srtSeparateCli* (its complex-domain
 * residual chain subtracts oob_weight * spectrum), srtIstftWiener, srtSeparateBatchWiener and srtSetWiener(n > 0) (the filter's gains above F are a follow-up).  The live
 * stream has the mode as an option of its own handle (srtLiveCreateEx); the plugin surface (Spleeter4Stems*) keeps the constant rule.
 * srtCopyTensor(e, "mask_ext", stem, 0, h, 2 * rows) returns the table the last such call left for that stem: [rows][2] (L, R); after srtSeparateBatch the
 * rows are the packed rows (track k from row tile0[k] * T). */
#define SRT_MASK_EXT_CONSTANT 0
#define SRT_MASK_EXT_AVERAGE  1
SRT_API int  srtSetMaskExtension(srt_engine *e, int mode);

/* ---- stem remix inside the inverse transform.  Most callers want a mix of the stems (karaoke = everything minus the vocals, an accompaniment
 * next to the vocals, one gain per stem, the stems plus their residual), not the stems.  The masking is linear, out_m = iSTFT(X * sum_s G[m][s] g_s), so the
 * mix is formed on the gains in the inverse transform's prologue: M mixes cost M inverse transforms instead of n_stems, and only the M results exist in memory
 * or cross the bus.
 * n_out = 0 (h_gain ignored): off, the default - every path and kernel as it always was, bit for bit.
 * 1 <= n_out <= SRT_MAX_STEMS: h_gain is [n_out][n_stems + 1], row-major, copied.
 *   G[m][s], s < n_stems: gain of stem s in output m.
 *   G[m][n_stems]: gain of the unmasked input.
 * Takes effect for later calls.
 * While the mix is on, srtIstft (also with d_masks = NULL), srtSeparate[Ex] (ratio_mask, srtSetOverlap, both mask-extension modes, graph mode: a changed
 * matrix never replays a graph captured with the old one) and srtSeparateHostStream[Ex|Io] (staging, seam carry, download and the 16-bit pack over n_out
 * planes; h_clipped has n_out entries) write n_out stereo pairs [n_out][2][len] instead of n_stems.  Output m, channel c, spectrum row r, bin k is the
 * inverse transform of X(r,c,k) * h_m(r,c,k),
 *   h = G[m][n_stems];  for s = 0 .. n_stems-1 (ascending):  h = fmaf(G[m][s], g_s(r,c,k), h)
 * in fp32, one fused multiply-add per stem in that fixed order.  g_s is the gain the inverse transform applies for stem s with the mix off: in band (k < F)
 * the mask value (1 without masks), cross-faded under srtSetOverlap, then normalised across the stems with ratio_mask and n_stems > 1 (blend first, then
 * normalise); above F oob_weight[s], or under SRT_MASK_EXT_AVERAGE the table value e_s(r,c) (1 without masks).  A row that is 1 on stem m and 0 elsewhere
 * reproduces stem m bit for bit; G[m] = (0, .., 0, 1) is the plain STFT -> iSTFT round trip.  The fp16 mode keeps its masks as floats while the mix is on.
 * srtSetMix returns -1 with srtLastError() text (before any device work) for a null engine, n_out outside 0..SRT_MAX_STEMS, a null h_gain with n_out > 0, an
 * entry that is not finite, or the Wiener filter on; srtSetWiener(n > 0) returns -1 while the mix is on.
 * Refused with -1, a text that says "mix" and nothing launched or written while the mix is on: srtSeparateCli, srtSeparateCliHost[Io] (no stem axis),
 * srtIstftWiener, srtSeparateBatchWiener (follow-ups), srtSeparateBatch[Overlap] (the batch takes the mix per track and per call: srtSeparateBatchMix)
 * and srtMultiSeparate*Host when any engine of the object has it on.  The live
 * stream has the mix on its own handle (srtLiveCreateEx, srtLiveSetMix); the plugin surface (Spleeter4Stems*) writes every stem. */
SRT_API int srtSetMix(srt_engine *e, int n_out, const float *h_gain);
SRT_API int srtMixOutputs(const srt_engine *e);   /* n_out while on, 0 while off or for a null engine */

/* Many independent tracks in one packed batch.  Track k of a batch occupies the packed tiles [tile0[k], tile0[k] + ceil(srtStftRows(n[k]) / T)).
 * srtBatchPlan is pure host arithmetic (no device, like srtRankSpan): tile0 may be NULL; *total_tiles = the sum.  -1 for ntracks < 1, T < 1 or any n[k] < 4096.
 * srtSeparateBatch: K whole tracks (srtSeparate geometry each) in one launch sequence - one batched STFT, one srtForward over the packed tiles, one batched
 * inverse transform - with each track's stems equal to what srtSeparate gives for it alone (bit for bit with batch_invariant; ratio_mask and the fp16
 * mode's half masks as in srtSeparate).  d_L, d_R, n, d_out: host arrays of ntracks entries (device pointers); d_out[k]: [n_stems][2][srtIstftLength(srtStftRows(n[k]))].
 * The track table is uploaded in stream order into engine memory, so the host arrays may be reused once the call returns; the call does not wait for the GPU
 * (it only waits for the table upload it issued four calls earlier).  It always launches eagerly, also in graph mode, and is refused inside a stream capture.
 * -1, with nothing launched, for ntracks < 1, a null array or entry, any n[k] < 4096, more than max_tiles packed tiles, or the Wiener filter on (its
 * statistics have to be per track: srtSeparateBatchWiener).  srtCopyTensor afterwards addresses the packed tiles: tile = tile0[k] + the tile within track k. */
SRT_API int  srtBatchPlan(const size_t *n, int ntracks, int T, size_t *tile0, size_t *total_tiles);
SRT_API int  srtSeparateBatch(srt_engine *e, int ntracks, const float *const *d_L, const float *const *d_R,
                              const size_t *n, float *const *d_out);

/* srtSeparateBatch with overlapped tiles inside every track: the overlap of srtSetOverlap, per track of a packed batch.
 * srtBatchPlanOverlap: track k takes srtOverlapTiles(srtStftRows(n[k]), T, overlap_rows) packed tiles from tile0[k]; overlap_rows = 0 is srtBatchPlan.  Pure host
 * arithmetic; -1 with srtLastError() text for everything srtBatchPlan refuses and for overlap_rows outside 0..T/2.
 * srtSeparateBatchOverlap: arguments, output layout, track-table upload and slot ring as srtSeparateBatch; always eager, refused inside a stream capture.
 * overlap_rows holds for this call whatever srtSetOverlap says - the engine's own setting is neither read nor changed - and 0 issues exactly the launches of
 * srtSeparateBatch.  With O = overlap_rows in 1..T/2 track k's spectrum stays at the packed rows from tile0[k] * T (rows <= tiles * T), its magnitudes and masks
 * use the overlapped layout inside its own tiles [tile0[k], tile0[k] + tiles_k) - no row of a track is ever written to or blended with a tile of another - and
 * its stems are what srtSeparate gives for that track alone after srtSetOverlap(e, O): bit for bit with batch_invariant, up to the network's batch-dependent
 * kernel choice otherwise.  ratio_mask (blend, then normalise), the fp16 mode's half masks and both mask-extension modes as in srtSeparate; after a call with
 * SRT_MASK_EXT_AVERAGE srtCopyTensor("mask_ext") holds track k's rows from packed row tile0[k] * T (rows between a track's last row and its next tile boundary
 * are not written).
 * -1, with nothing launched or written, for everything srtSeparateBatch refuses except the engine's overlap setting, overlap_rows outside 0..T/2, more than
 * max_tiles overlapped packed tiles (srtBatchPlanOverlap counts them), the engine's stem remix on (srtSeparateBatchMix), or the Wiener filter on; -5 when a stem's weights are not set.
 * srtSeparateBatch keeps refusing while srtSetOverlap > 0, and srtSeparateBatchWiener keeps refusing an overlap. */
SRT_API int  srtBatchPlanOverlap(const size_t *n, int ntracks, int T, int overlap_rows, size_t *tile0, size_t *total_tiles);
SRT_API int  srtSeparateBatchOverlap(srt_engine *e, int ntracks, const float *const *d_L, const float *const *d_R,
                                     const size_t *n, float *const *d_out, int overlap_rows);

/* srtSeparateBatchOverlap with a stem remix per track: every track of a queue carries its own request - vocals only for one upload, karaoke at
 * -3 dB for the next - so the matrix of srtSetMix is an argument per track here.  Tracks, packing (srtBatchPlanOverlap), track-table upload and slot ring as
 * srtSeparateBatchOverlap; always eager, refused inside a stream capture; the only host wait is the one for the upload issued four calls earlier.
 * overlap_rows (0..T/2), n_out and the matrices hold for this call: the engine's own srtSetOverlap and srtSetMix state is neither read nor changed, the call works
 * with either on or off, and srtMixOutputs(e) is the same afterwards.
 * 1 <= n_out <= SRT_MAX_STEMS, one number for the call: d_out[k] is [n_out][2][srtIstftLength(srtStftRows(n[k]))].  h_gain is host memory and is copied; track k's
 *   matrix is [n_out][n_stems + 1], row-major in srtSetMix's layout, at h_gain + k * gain_stride.  gain_stride = 0: every track uses the one matrix at h_gain;
 *   otherwise gain_stride >= n_out * (n_stems + 1).  The matrices go up in stream order beside the track table, into a device table the first such call allocates.
 * Output m of track k is what srtSeparate writes for that track alone after srtSetOverlap(e, overlap_rows) and srtSetMix(e, n_out, G_k) - srtSetMix's chain
 *   h = G_k[m][n_stems]; h = fmaf(G_k[m][s], g_s, h) for s ascending, over the same g_s (mask, cross-fade, ratio_mask; above F oob_weight[s] or the table value of
 *   SRT_MASK_EXT_AVERAGE) - bit for bit with batch_invariant, up to the network's batch-dependent kernel choice otherwise.  The fp16 mode keeps its masks as floats
 *   for this call, as with srtSetMix.
 * n_out = 0: srtSeparateBatchOverlap(.., overlap_rows), launch for launch; h_gain and gain_stride are ignored.
 * -1 with srtLastError() text that names srtSeparateBatchMix, and nothing launched or written, for everything srtSeparateBatchOverlap refuses except the engine's
 * mix setting, n_out outside 0..SRT_MAX_STEMS, a null h_gain with n_out > 0, a non-zero gain_stride below n_out * (n_stems + 1), an entry that is not finite
 * (the text names the track), or the Wiener filter on; -5 when a stem's weights are not set.
 * The mix under the Wiener filter per track: srtSeparateBatchWienerEx.  Follow-ups: a per-track n_out, graph capture of batch calls. */
SRT_API int  srtSeparateBatchMix(srt_engine *e, int ntracks, const float *const *d_L, const float *const *d_R,
                                 const size_t *n, float *const *d_out, int overlap_rows,
                                 int n_out, const float *h_gain, size_t gain_stride);

/* A long HOST-resident stream through one GPU: cut into chunks of max_tiles tiles, upload / compute / download overlapped on
 * three HIP streams with double buffers, chunk overlaps (3072 samples) added on the device.  Geometry as srtSeparateEx.
 * h_out: [n_stems][2][srtIstftLength(rows)].  Synchronous; replaces main()'s whole-file stft -> processMT -> istft
 * (Executable/main.c:776-785) for inputs of any length (the reference holds the full 4096-wide spectrogram in RAM). */
SRT_API int  srtSeparateHostStream(srt_engine *e, const float *h_L, const float *h_R, size_t n, size_t frames, size_t rows, float *h_out);
/* The same with flags.  SRT_HOST_PINNED: h_L, h_R and h_out are already page-locked (hipHostMalloc / hipHostRegister), so the
 * call registers nothing (registering GBs of pageable memory per call costs more than the separation itself).  The device
 * double buffers, copy streams and events are kept in the engine between calls either way. */
#define SRT_HOST_PINNED 1u
SRT_API int  srtSeparateHostStreamEx(srt_engine *e, const float *h_L, const float *h_R, size_t n, size_t frames, size_t rows, float *h_out, unsigned flags);

/* The offline CLI's flows (Executable/main.c:776-798 for stems == 2, :845-928 for stems == 3), everything in HBM.
 * Sub-network 0 = the CLI's net[0] (drum, stem_mode 1), sub-network 1 = net[1] (vocal, stem_mode 0)  (main.c:759-760).
 * d_out: [stems][2][srtIstftLength(srtStftRows(n))] in the CLI's output order: Vocal, Accompaniment | Drum, Vocal, Accompaniment. */
SRT_API int  srtSeparateCli(srt_engine *e, const float *d_L, const float *d_R, size_t n, int stems, float *d_out);
/* host buffers, synchronous.  Its device staging (whole-file PCM + outputs when the file fits max_tiles, chunk double buffers otherwise) is
 * grow-only and kept for later calls, like srtSeparateHostStream's; a one-shot caller frees it with srtReleaseStaging. */
SRT_API int  srtSeparateCliHost(srt_engine *e, const float *h_L, const float *h_R, size_t n, int stems, float *h_out);

/* ---- 16-bit PCM at the host-stream boundary: the file path is bound by PCIe, and its callers read and write 16-bit WAV data.
 * Unpack: x = (float)q / 32768 (exact).  Pack: q = rint(x * 32768), ties to even, clamped to [-32768, 32767], NaN -> 0; a sample is CLIPPED when the
 * unclamped value lies outside that range or is NaN (+1.0f clips, -1.0f does not).
 * srtPcm16Unpack: d_in interleaved stereo [n][2] -> planar d_L [n], d_R [n].
 * srtPcm16Pack: `pairs` stereo pairs of planar fp32, pair p at d_planes + 2p * plane_stride (L) and + (2p + 1) * plane_stride (R), samples [0, count)
 * -> d_out + p * out_stride * 2 as [count][2] (a WAV data chunk's bytes).  d_clipped (may be NULL) [pairs]: each pair's clipped samples are ADDED to it,
 * exactly and reproducibly (no atomics).  Both: device pointers of any alignment (16-byte aligned pointers and strides of a multiple of 4 take the
 * vector path), asynchronous on `stream`, capturable; -1 before any device work for a null pointer, pairs < 1, or a stride below count. */
SRT_API int  srtPcm16Unpack(void *stream, const int16_t *d_in, size_t n, float *d_L, float *d_R);
SRT_API int  srtPcm16Pack(void *stream, const float *d_planes, size_t plane_stride, int pairs, size_t count, int16_t *d_out, size_t out_stride,
                          unsigned long long *d_clipped);
/* srtSeparateHostStreamEx / srtSeparateCliHost with 16-bit host buffers: the conversion runs on the device, per chunk, so half the bytes cross the bus.
 * SRT_HOST_IN_PCM16: h_in is int16 interleaved stereo [n][2] and h_in2 must be NULL (otherwise h_in = h_L, h_in2 = h_R, floats).
 * SRT_HOST_OUT_PCM16: h_out is int16 [stems][srtIstftLength(rows)][2] (otherwise float [stems][2][len]); h_clipped (may be NULL) [stems] receives each stem's
 * clipped samples.  The two flags are independent; the seam arithmetic stays fp32 and every output sample is quantised once.  Without either flag these are the
 * float calls (h_clipped, when given, is zeroed); SRT_HOST_PINNED keeps its meaning.  With a PCM16 flag srtSeparateCliHostIo always takes the chunked
 * pipeline (one chunk when the file fits).  -1 as the float forms (overlap, Wiener), and for SRT_HOST_IN_PCM16 with h_in2 != NULL or unknown flag bits. */
#define SRT_HOST_IN_PCM16  2u
#define SRT_HOST_OUT_PCM16 4u
SRT_API int  srtSeparateHostStreamIo(srt_engine *e, const void *h_in, const void *h_in2, size_t n, size_t frames, size_t rows,
                                     void *h_out, unsigned flags, unsigned long long *h_clipped);
SRT_API int  srtSeparateCliHostIo(srt_engine *e, const void *h_in, const void *h_in2, size_t n, int stems,
                                  void *h_out, unsigned flags, unsigned long long *h_clipped);

/* ---- 24-bit PCM and dithered 16-bit output: the rest of the sample-format axis of the calls that take `flags`.
 * 24-bit, packed: three bytes per sample, little-endian, two's complement, interleaved stereo (a WAV format-1 data chunk with block align 6).
 *   Unpack: q is the sign-extended 24-bit integer, x = (float)q * 2^-23 (exact).  Pack: v = rint(x * 2^23), ties to even (the product is exact); NaN -> 0,
 *   otherwise clamped to [-8388608, 8388607].  CLIPPED as the 16-bit rule defines it: v outside the range, or NaN (+1.0f clips, -1.0f does not).
 * Dithered 16-bit: v = rint(x * 32768 + d) with d a TPDF (triangular probability density) value in (-1, 1) LSB; x * 32768 is exact, so the sum is rounded
 *   once.  Clamp, NaN and the clip count are the 16-bit rule's, applied to the dithered v.  d depends on nothing but (seed, plane, i): plane = 2 * pair + channel
 *   in output order, i the 64-bit index of the sample in its output plane for the whole call - so a stream gets the same noise whatever max_tiles, chunking or
 *   piece plan cut it, and a run is reproducible.  All arithmetic below is uint32 with wrap-around:
 *       mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *       k = mix32(lo32(seed) ^ mix32(hi32(seed) ^ mix32(plane + 0x9e3779b9)))
 *       h = mix32(lo32(i) ^ mix32(hi32(i) ^ k))
 *       a = mix32(h ^ 0x68bc21eb) >> 8;   b = mix32(h ^ 0x02e5be93) >> 8        (two 24-bit uniforms)
 *       d = (float)((int)a - (int)b) * 2^-24                                     (exact)
 *   Dither with 24-bit output is refused: above |x| = 2^-1 a float's own spacing is already the 24-bit LSB, so there is nothing below the LSB to decorrelate.
 *   Noise shaping (sequential per channel) and 32-bit integer PCM are not provided.
 * srtPcm24Unpack: d_in [n][2][3] bytes -> planar d_L [n], d_R [n].  srtPcm24Pack: as srtPcm16Pack, pair p -> d_out + p * out_stride * 6 as [count][2][3] bytes.
 * srtPcm16PackDither: srtPcm16Pack with the dither; pair p's planes are 2 * (first_pair + p) and + 1, and sample 0 of the launch has plane index first_index
 * (a caller that packs a long output in several launches passes each launch's offset and gets the bytes of one launch).
 * All three: device pointers of any alignment (the 24-bit vector path wants 16-byte aligned bases, plane_stride % 4 == 0 and out_stride % 8 == 0), asynchronous
 * on `stream`, capturable; -1 before any device work for a null pointer, pairs < 1, pairs > 65535, a stride below count, or first_pair < 0. */
SRT_API int  srtPcm24Unpack(void *stream, const uint8_t *d_in, size_t n, float *d_L, float *d_R);
SRT_API int  srtPcm24Pack(void *stream, const float *d_planes, size_t plane_stride, int pairs, size_t count, uint8_t *d_out, size_t out_stride,
                          unsigned long long *d_clipped);
SRT_API int  srtPcm16PackDither(void *stream, const float *d_planes, size_t plane_stride, int pairs, size_t count, int16_t *d_out, size_t out_stride,
                                unsigned long long *d_clipped, uint64_t seed, int first_pair, uint64_t first_index);
/* The flags of every call that takes `flags` (srtSeparateHostStreamIo / Overlap / Rate, srtSeparateHostWiener / WienerOverlap, srtSeparateCliHostIo):
 * SRT_HOST_IN_PCM24: h_in is uint8 [n][2][3] and h_in2 must be NULL.  SRT_HOST_OUT_PCM24: h_out is uint8 [outputs][len][2][3]; h_clipped as for 16 bits.
 * SRT_HOST_OUT_DITHER: with SRT_HOST_OUT_PCM16, the pack is srtPcm16PackDither under the engine's seed (srtSetDitherSeed), i running over the whole output.
 * -1, with a text that names the function and before any device work: both IN formats, both OUT formats, SRT_HOST_OUT_DITHER without SRT_HOST_OUT_PCM16, any
 * of these bits on a tile range of a multi-device stream.  Bit 8 and the bits from 128 up are unknown.  A call that sets none of the three issues exactly the
 * launches it issued before they existed. */
#define SRT_HOST_IN_PCM24   16u
#define SRT_HOST_OUT_PCM24  32u
#define SRT_HOST_OUT_DITHER 64u
/* the seed of SRT_HOST_OUT_DITHER (default 0): read once per call into the call's resolved options */
SRT_API int  srtSetDitherSeed(srt_engine *e, uint64_t seed);

/* Low-latency callers that repeat the same call (same device pointers and sizes) over and over - the real-time plugin, the tile
 * API on one pair of buffers: with graph mode on, srtForward and srtSeparate / srtSeparateEx capture their launch sequence into
 * a hipGraph the first time an argument tuple is seen and replay it afterwards (one host call instead of ~25 launches; 4 cached
 * tuples, least recently used evicted).  Needs an explicit stream (the legacy null stream cannot be captured: the engine then
 * keeps launching eagerly).  Results are identical either way.  Off by default. */
SRT_API int  srtSetGraphMode(srt_engine *e, int enable);
/* Everything the first srtForward(e, d_mag, ntiles, d_masks) would otherwise do lazily - the split-K workspace allocation and, in
 * graph mode, the capture + instantiation of the launch sequence for exactly this argument tuple - done NOW and synchronised, so
 * that the first real call (on a real-time audio thread) is a plain graph launch.  Runs the networks once: d_masks is overwritten.
 * The drop-in layers call it from their Init functions for every buffer pair they will use. */
SRT_API int  srtPrepareForward(srt_engine *e, const float *d_mag, int ntiles, float *d_masks);
/* free the grow-only device staging of the host-buffer entry points (srtSeparateHostStream*, srtSeparateCliHost, srtSeparateHostWiener and its store); the
 * next such call re-allocates */
SRT_API int  srtReleaseStaging(srt_engine *e);

/* ---- multichannel Wiener filter: official Spleeter's `separate --mwf` post-processing, norbert.wiener(v, x, n) with its defaults (soft-mask start,
 * eps = 2^-23), over the stereo image - a stem's left output can draw on the mixture's right channel.  v_{j,c} = mask * |x_c| in band (x = 4096 * spectrum, the
 * networks' scale); n EM iterations, each with a 2x2 spatial covariance R_j per (stem, bin) summed over EVERY row of the call, then W_j = v_j R_j C^-1
 * applied to x.  Bins >= F keep the engine's rule (oob_weight * spectrum).  On the GPU: one statistics pass + one finalize per iteration (fixed-order
 * sums, no atomics: bit-reproducible, also under graph replay), one filter pass, one inverse transform per stem.
 * srtSetWiener: 0 = off (the default; nothing changes), 1..3 = iterations (Spleeter's default is 1).  Allocates its workspace for max_tiles tiles now
 * (call it before capturing).  -1 with ratio_mask set or iterations outside 0..3.  While it is on, srtSeparate / srtSeparateEx apply it (srtSeparateEx:
 * the statistics window is the call's own `rows`, so a tile range of a longer stream is filtered with its own covariance), in the fp16 mode too (the
 * masks then stay fp32).  Refused with -1 because the statistics span the whole signal: srtSeparateHostStream* (chunks; srtSeparateHostWiener is the filter
 * over a host stream of any length), srtSeparateCli* (no stem axis either) and srtMultiSeparate* (ranges per device).  In graph mode the iteration count is part of the captured call's key. */
SRT_API int  srtSetWiener(srt_engine *e, int iterations);
/* the filter + inverse transform for a caller-given spectrum [2][rows][2052] (srtStft layout) and fp32 masks [n_stems][ntiles][2][T][F] of all stems,
 * `iterations` 1..3 whatever srtSetWiener says; d_out as srtIstft.  srtCopyTensor(e, "wiener_cov", stem, iteration, h, 5F + 1) then returns R_j of
 * that iteration of the last filtered call as [F][4] (R00, R11, Re R01, Im R01), the weight sums sum_t v_j [F] (spectrum units) and a [1]. */
SRT_API int  srtIstftWiener(srt_engine *e, const float *d_spec, size_t rows, const float *d_masks, int iterations, float *d_out);
/* ---- the filter with overlapped tiles, the average mask extension and the stem remix, for a single signal.  srtSetWiener / srtIstftWiener
 * refuse those three (see each of them); these two entry points take them as options that hold FOR THE CALL ONLY: the engine's srtSetWiener, srtSetOverlap,
 * srtSetMaskExtension and srtSetMix state is neither read nor changed (srtMixOutputs and the overlap are the same afterwards), and the calls work with any of
 * them on or off.  d_out is [n_out ? n_out : n_stems][2][srtIstftLength(rows)].
 *   overlap_rows O > 0: d_masks (and the magnitudes srtSeparateWiener builds) are in srtSetOverlap's layout, srtOverlapTiles(rows, T, O) tiles.  The filter sees
 *     ONE mask value per (stem, row, channel, bin): the blended value a + w (b - a) of srtSetOverlap's rule, formed by the inverse transform's own helper; that
 *     value enters v = m |x| in the soft-mask start of every pass.  Every spectrum row enters the statistics exactly once, however many tiles hold it; the
 *     window, a = max(1, max |x| / 10), the row chunks and the summation order depend on `rows` only, as in srtIstftWiener.
 *   SRT_MASK_EXT_CONSTANT: stem j's bins >= F are oob_weight[j] * spectrum, as in srtIstftWiener (oob_weight = 0 is what official Spleeter's --mwf does).
 *   SRT_MASK_EXT_AVERAGE: stem j's bins >= F of row r, channel c are e_j(r, c) * spectrum, e_j the table srtSetMaskExtension's kernel writes from the same masks
 *     with the same overlap (no ratio); oob_weight is ignored.  A deliberate definition: the extension follows the NETWORK's (blended) mask, not the filter -
 *     the filter's gain is a 2x2 matrix per bin and has no scalar mean.  The first such call allocates the engine's gain table if srtSetMaskExtension never did.
 *   n_out > 0: h_gain is [n_out][n_stems + 1] in srtSetMix's layout, host memory, copied.  In band output m is formed per complex component as
 *     h = G[m][n_stems] * s;  for j ascending: h = fmaf(G[m][j], y_j, h)     (y_j: stem j's filtered value; one rounded product, one fused multiply-add per stem);
 *     above F it is h * s with h = G[m][n_stems]; h = fmaf(G[m][j], g_j, h), g_j = oob_weight[j] or e_j(r, c): srtSetMix's chain.  A one-hot row gives that
 *     stem's bits.  Only n_out spectra are written and only n_out inverse transforms run.
 * With overlap_rows = 0, SRT_MASK_EXT_CONSTANT and n_out = 0 both calls issue exactly the launches of srtIstftWiener / of srtSeparate under
 * srtSetWiener(iterations): the same kernels, the same bits.  srtSeparateWiener: geometry as srtSeparate; one STFT in the overlapped layout, one forward over
 * srtOverlapTiles(rows, T, O) tiles (fp32 masks in the fp16 mode too), then the body of srtIstftWienerEx.  Both always launch eagerly, in graph mode too (a
 * graph key for the options is a follow-up); inside a caller's stream capture they return -1 when a workspace they need is not allocated yet.
 * -1 with srtLastError() text that names the function, before any device work and with nothing written: a null argument or opts, iterations outside 1..3,
 * overlap_rows outside 0..T/2, an unknown mask_extension, n_out outside 0..n_stems (the filter's spectrum workspace holds n_stems spectra), a null h_gain with
 * n_out > 0, a gain that is not finite, ratio_mask set, more than max_tiles overlapped tiles, n < 4096; -5 when a stem's weights are not set (srtSeparateWiener).
 * srtCopyTensor "wiener_cov" works afterwards as after srtIstftWiener, "mask_ext" after a call with the average extension.
 * The same options per track of a packed batch: srtSeparateBatchWienerEx.  Follow-ups: graph capture, n_out > n_stems, the filter folded into the inverse
 * transform's prologue. */
typedef struct srt_wiener_opts {
    int iterations;       /* 1..3 */
    int overlap_rows;     /* 0..T/2; masks / magnitudes in srtSetOverlap's layout, srtOverlapTiles(rows, T, O) tiles */
    int mask_extension;   /* SRT_MASK_EXT_CONSTANT | SRT_MASK_EXT_AVERAGE */
    int n_out;            /* 0: every stem; 1..n_stems: outputs of the mix */
    const float *h_gain;  /* [n_out][n_stems + 1], srtSetMix's layout, host memory, copied */
} srt_wiener_opts;
SRT_API int  srtIstftWienerEx(srt_engine *e, const float *d_spec, size_t rows, const float *d_masks, const srt_wiener_opts *opts, float *d_out);
SRT_API int  srtSeparateWiener(srt_engine *e, const float *d_L, const float *d_R, size_t n, const srt_wiener_opts *opts, float *d_out);
/* srtSeparateBatch with the filter per track: arguments, layout, track table and packing as srtSeparateBatch (srtBatchPlan; d_out[k]:
 * [n_stems][2][srtIstftLength(srtStftRows(n[k]))]); `iterations` 1..3 whatever srtSetWiener says (the engine's setting may be on or off).  One batched STFT,
 * one srtForward over the packed tiles (fp32 masks, in the fp16 mode too), `iterations` x (statistics + finalize) and one filter pass over the packed rows,
 * one batched inverse transform.  Track k's stems are what srtSeparate gives for track k alone with srtSetWiener(e, iterations) - bit for bit with
 * batch_invariant, up to the network's batch-dependent kernel choice otherwise: the statistics window is the track's own srtStftRows(n[k]) rows (not the
 * rows that pad it to its tile boundary, not another track), a = max(1, max |x| / 10) is the track's, and its row chunks follow the single call's rule, so
 * its R tables equal the single call's whatever else the batch holds and wherever the track sits in it.  Always eager, refused inside a stream capture,
 * the only host wait is the table upload issued four calls earlier; the workspace (per-track tables, a statistics slab of max_tiles * T / 16 + max_tiles
 * chunks) is allocated by the first call and kept until srtDestroy.  -1, with nothing launched or written, for everything srtSeparateBatch refuses,
 * iterations outside 1..3, ratio_mask set, srtSetOverlap > 0 and SRT_MASK_EXT_AVERAGE; -5 when a stem's weights are not set.
 * srtCopyTensor(e, "wiener_cov", stem, 4 * k + iteration, h, 5F + 1) then returns track k's tables (as after srtIstftWiener: R, weight sums, a). */
SRT_API int  srtSeparateBatchWiener(srt_engine *e, int ntracks, const float *const *d_L, const float *const *d_R,
                                    const size_t *n, float *const *d_out, int iterations);
/* srtSeparateBatchWiener with srtSeparateWiener's options per call: the filter over a packed batch with overlapped tiles inside every track,
 * the average mask extension and a stem remix per track.  Tracks, track-table upload and slot ring as srtSeparateBatchWiener; packing as srtBatchPlanOverlap(n,
 * ntracks, T, overlap_rows, ..); d_out[k] is [n_out ? n_out : n_stems][2][srtIstftLength(srtStftRows(n[k]))] and nothing past those planes is written.  Always
 * eager, refused inside a stream capture; the only host wait is the one for the upload issued four calls earlier.
 * All five options hold for this call only: the engine's srtSetWiener, srtSetOverlap, srtSetMaskExtension and srtSetMix state is neither read nor changed, and
 * the call works with any of them on or off (the one batch call that takes the rule for bins >= F from its arguments, not from srtSetMaskExtension).
 * Output m of track k is what srtSeparateWiener(e, L_k, R_k, n_k, {iterations, overlap_rows, mask_extension, n_out, G_k}, out) writes for that track alone - bit
 *   for bit with batch_invariant, up to the network's batch-dependent kernel choice otherwise.  Everything the filter derives from "the call" is the track's: the
 *   statistics window is its own srtStftRows(n[k]) rows, each entering once however many of its tiles hold it; a is its own; its row chunks follow the single
 *   call's rule; a blend partner is a tile of the same track; the table e_j(r, c) of SRT_MASK_EXT_AVERAGE comes from its own blended masks (no ratio).
 *   h_gain is host memory and is copied; track k's matrix G_k is [n_out][n_stems + 1] in srtSetMix's layout at h_gain + k * gain_stride (srtSeparateBatchMix's
 *   rule: gain_stride = 0 - one matrix for every track).  n_out is one number for the call, 1..n_stems (the filter's spectrum workspace holds n_stems spectra).
 * With overlap_rows = 0, SRT_MASK_EXT_CONSTANT and n_out = 0 the call issues exactly the launches of srtSeparateBatchWiener(.., iterations): the same kernels,
 * the same bits.  Otherwise: one batched STFT, one srtForward over the overlapped packed tiles (fp32 masks in the fp16 mode too), iterations x (statistics +
 * finalize), the gain table with SRT_MASK_EXT_AVERAGE, one filter launch that writes final spectra, one batched inverse of n_out (or n_stems) spectra per track.
 * -1 with srtLastError() text that names srtSeparateBatchWienerEx, before any device work and with nothing written: a null engine, opts or array or a null entry,
 * everything srtSeparateBatch refuses of its track arrays, iterations outside 1..3, overlap_rows outside 0..T/2, an unknown mask_extension, n_out outside
 * 0..n_stems, a null h_gain with n_out > 0, a non-zero gain_stride below n_out * (n_stems + 1), a gain that is not finite (the text names the track), ratio_mask
 * set, more than max_tiles overlapped packed tiles (srtBatchPlanOverlap counts them), more than 65535 blocks of 16 packed rows, a call inside a stream capture;
 * -5 when a stem's weights are not set.
 * srtCopyTensor(e, "wiener_cov", stem, 4 * k + iteration, ..) works as after srtSeparateBatchWiener; after a call with the average extension
 * srtCopyTensor(e, "mask_ext", ..) holds track k's rows from packed row tile0[k] * T, as after srtSeparateBatchOverlap.
 * Follow-ups: a per-track overlap, iteration count or n_out, n_out > n_stems, graph capture of batch calls. */
typedef struct srt_batch_wiener_opts {
    int iterations;        /* 1..3 */
    int overlap_rows;      /* 0..T/2, one value for the call (the packing depends on it: srtBatchPlanOverlap) */
    int mask_extension;    /* SRT_MASK_EXT_CONSTANT | SRT_MASK_EXT_AVERAGE */
    int n_out;             /* 0: every stem; 1..n_stems: outputs of the mix, one number for the call */
    const float *h_gain;   /* track k's [n_out][n_stems + 1] at h_gain + k * gain_stride, host memory, copied (srtSeparateBatchMix's rule) */
    size_t gain_stride;    /* 0: one matrix for every track; else >= n_out * (n_stems + 1) */
} srt_batch_wiener_opts;
SRT_API int  srtSeparateBatchWienerEx(srt_engine *e, int ntracks, const float *const *d_L, const float *const *d_R,
                                      const size_t *n, float *const *d_out, const srt_batch_wiener_opts *opts);
/* ---- the filter over a HOST stream of any length: srtSeparateWiener for host-resident PCM that need not fit max_tiles tiles - the albums,
 * DJ sets and hour-long streams srtSeparateHostStream* exists for, and which it refuses with the filter on.  Geometry: the whole stream (rows = srtStftRows(n),
 * frames = srtStftFrames(n)).  h_in, h_in2, h_out, flags (SRT_HOST_PINNED | SRT_HOST_IN_PCM16 | SRT_HOST_OUT_PCM16) and h_clipped exactly as in
 * srtSeparateHostStreamIo; h_out is [n_out ? n_out : n_stems][2][srtIstftLength(rows)] floats, or int16 [..][len][2] with the out flag, and nothing past those
 * planes is written.  Synchronous, always eager, refused inside a stream capture.  Any n >= 4096 works, one piece (a signal that fits max_tiles) included.
 * What it equals: srtSeparateWiener(e, L, R, n, opts, out) on an engine large enough to hold the signal.  The R tables, weight sums and a are that call's BIT FOR
 *   BIT (with batch_invariant; up to the network's batch-dependent kernel choice otherwise): the stream is walked in pieces of max_tiles tiles, and a statistics
 *   chunk that straddles a piece boundary continues its partial sum from the slab (srt_wiener_stats_seg_kernel), so every sum keeps the whole-signal launch's
 *   order.  The samples agree up to the association of the overlap-add at the piece seams (the 3072-sample seam is added on the device as in
 *   srtSeparateHostStream: 2e-6 of the peak); a signal of one piece gives srtSeparateWiener's bits.
 * How: sweep A uploads each piece and writes its spectrum and fp32 masks (in the fp16 mode too) into a device store that holds them for the whole stream, with
 *   statistics pass 1; passes 2..iterations walk the store (no network, no PCIe); sweep B filters, inverts and downloads piece by piece.  The store takes
 *   2 * 2052 * 8 + n_stems * 2 * F * 4 bytes per row, the masks padded to the tile boundary (about 65 KB per row at 4 stems and F = 1024, roughly 10 GB per hour
 *   of audio); it is grow-only and kept with the host staging, srtReleaseStaging frees it.  srtHostWienerBytes(cfg, n) returns its size - pure host arithmetic, no
 *   device - so a caller can check first; 0 with srtLastError() text for a null or bad config or n < 4096.  If the store cannot be allocated the call returns -2,
 *   the text names the bytes asked for, and the engine stays usable.
 * opts hold for the call only: the engine's srtSetWiener, srtSetOverlap, srtSetMaskExtension and srtSetMix state is neither read nor changed, and the call works
 *   with any of them on or off.  Honoured: iterations 1..3, mask_extension (both modes), n_out / h_gain (1..n_stems, srtSetMix's layout) - all row-local once the
 *   tables exist.  Refused: overlap_rows must be 0 (-1, the text says "overlap"): srtSeparateHostWienerOverlap below is the entry point that takes one.
 * -1 with srtLastError() text that names srtSeparateHostWiener, before any device work and with nothing written: a null argument, unknown flag bits or
 * SRT_HOST_IN_PCM16 with h_in2 != NULL, everything srtSeparateWiener refuses of its options except the max_tiles limit, ratio_mask set, n < 4096; -5 when a
 * stem's weights are not set.  srtCopyTensor "wiener_cov" works afterwards as after srtSeparateWiener.
 * srtSeparateHostStream*, srtSeparateCli* and srtMultiSeparate* keep refusing the engine's srtSetWiener.  Follow-ups: the multi-device host, the CLI flows,
 * n_out > n_stems, graph capture.  (Overlapped tiles across piece seams: built, srtSeparateHostWienerOverlap.) */
SRT_API int    srtSeparateHostWiener(srt_engine *e, const void *h_in, const void *h_in2, size_t n,
                                     const srt_wiener_opts *opts, void *h_out, unsigned flags, unsigned long long *h_clipped);
SRT_API size_t srtHostWienerBytes(const srt_config *cfg, size_t n);
/* ---- the filter with overlapped tiles over a HOST stream of any length: srtSeparateHostWiener with opts->overlap_rows honoured (0..T/2) - the
 * quality configuration (`--mwf` on overlapped tiles) on the path for albums and hour-long streams.  Buffers, flags, h_clipped, the output planes, the options
 * honoured (iterations 1..3, both mask_extension modes, n_out / h_gain) and the rule that the engine's setter state is neither read nor changed are exactly
 * srtSeparateHostWiener's.  Synchronous, always eager, refused inside a stream capture.  Any n >= 4096 works, one piece included.
 * What it equals: srtSeparateWiener(e_big, L, R, n, opts, out) on an engine with max_tiles >= srtOverlapTiles(srtStftRows(n), T, overlap_rows).  The R tables,
 *   weight sums and a are that call's BIT FOR BIT (with batch_invariant): every spectrum row enters the statistics exactly once, with the blended mask value
 *   a + w (b - a) of srtSetOverlap's rule, in the whole-signal launch's summation order (the chunking depends on the row count alone).  Every row gets the same gain;
 *   the samples agree up to the association of the overlap-add at the piece seams (2e-6 of the peak); a signal of one piece gives srtSeparateWiener's bits.
 *   overlap_rows = 0 is srtSeparateHostWiener: the same launches, the same bits.
 * How: the stream is walked in the pieces of srtHostOverlapPieces(rows, T, overlap_rows, max_tiles) on srtSeparateHostWiener's two-sweep schedule.  A piece
 *   analyses stft_rows rows into the overlapped layout of its own tiles (its last tile reaches O rows into the next piece: those rows are uploaded and transformed
 *   twice), but only the own_rows rows it owns enter the statistics, the filter, the inverse and the download.  Rows [0, O) of a later piece blend with rows [S, T)
 *   of the previous piece's last tile, which sweep A copies into a carry of n_stems * 2 * O * F floats per piece boundary, kept in the store.
 * The store (kept with the host staging, grow-only, srtReleaseStaging frees it) holds per piece its spectrum - the look-ahead rows included -, its fp32 masks and
 *   its carry: with S = T - O, N = srtOverlapTiles(rows, T, O) and P = max_tiles, every piece but the last takes
 *   2 * ((P - 1) S + T) * 2052 * 8 + n_stems * P * 2 * T * F * 4 + n_stems * 2 * O * F * 4 bytes, and the last one 2 * stft_rows * 2052 * 8 + n_stems * tiles * 2 * T * F * 4
 *   (about T / S times srtHostWienerBytes).  srtHostWienerOverlapBytes(cfg, n, overlap_rows) returns the total - pure host arithmetic, no device; at
 *   overlap_rows = 0 it is srtHostWienerBytes(cfg, n); 0 with srtLastError() text for a null or bad config, n < 4096 or overlap_rows outside 0..T/2.  If the
 *   store cannot be allocated the call returns -2, the text names the bytes asked for, and the engine stays usable.
 * -1 with srtLastError() text that names srtSeparateHostWienerOverlap, before any device work and with nothing written: everything srtSeparateHostWiener
 * refuses except the overlap; overlap_rows outside 0..T/2 (the text says "overlap"); -5 when a stem's weights are not set.  After a call with the average mask
 * extension srtCopyTensor("mask_ext") holds the LAST piece's owned rows.  Not built: the multi-device host, the CLI flows, n_out > n_stems, graph capture, a
 * store of halves. */
SRT_API int    srtSeparateHostWienerOverlap(srt_engine *e, const void *h_in, const void *h_in2, size_t n,
                                            const srt_wiener_opts *opts, void *h_out, unsigned flags, unsigned long long *h_clipped);
SRT_API size_t srtHostWienerOverlapBytes(const srt_config *cfg, size_t n, int overlap_rows);

/* ---- overlapped network tiles over a HOST stream of any length: srtSeparate under srtSetOverlap(e, overlap_rows) for host-resident PCM that need
 * not fit max_tiles overlapped tiles.  Geometry: the whole stream (rows = srtStftRows(n), frames = srtStftFrames(n)).  h_in, h_in2, h_out, flags (SRT_HOST_PINNED |
 * SRT_HOST_IN_PCM16 | SRT_HOST_OUT_PCM16) and h_clipped exactly as in srtSeparateHostStreamIo; h_out is [n_out ? n_out : n_stems][2][srtIstftLength(rows)] floats, or
 * int16 [..][len][2] with the out flag.  Synchronous and always eager.  Any n >= 4096 works, one piece included.
 * overlap_rows (0..T/2) holds for this call only: the engine's srtSetOverlap is neither read nor changed, and the call works with it on or off.  Everything else
 *   comes from the engine as in srtSeparateHostStreamIo: ratio_mask (blend, then normalise), srtSetMaskExtension in both modes, srtSetMix.  With overlap_rows > 0
 *   the masks stay floats in the fp16 mode, as they do under srtSetMix.  overlap_rows = 0 is srtSeparateHostStreamIo(e, .., n, frames, rows, ..): the same
 *   launches, the same bits.
 * What it equals: srtSeparate on an engine large enough to hold the signal after srtSetOverlap(e, overlap_rows).  Every spectrum row gets the same gain, bit for
 *   bit with batch_invariant (up to the network's batch-dependent kernel choice otherwise); the samples agree up to the association of the overlap-add at the
 *   piece seams (2e-6 of the peak, as in srtSeparateHostStream); a signal of one piece gives srtSeparate's bits.
 * How: the stream is walked in pieces of max_tiles overlapped tiles (srtHostOverlapPieces).  With S = T - O, piece p holds tiles [tile0, tile0 + tiles), owns -
 *   inverts and downloads - the own_rows rows from row0 = tile0 * S, and analyses stft_rows >= own_rows rows from row0: its last tile reaches O rows into the next
 *   piece, which are uploaded and transformed twice (O / (max_tiles * S) of the work).  Rows [0, O) of every later piece blend with rows [S, T) of the previous
 *   piece's last tile, which a small kernel keeps in a carry of n_stems * 2 * O * F floats beside the host staging (grow-only, srtReleaseStaging frees it).
 *   After a call with the average mask extension srtCopyTensor("mask_ext") holds the LAST piece's rows.
 * srtHostOverlapPieces: the plan - pure host arithmetic, no device (like srtBatchPlanOverlap).  Returns the piece count and fills pieces[0 .. min(count,
 *   max_pieces)) when pieces is not NULL; 0 for rows = 0; 0 with srtLastError() text for T < 1, overlap_rows outside 0..T/2 or max_tiles < 1.  overlap_rows = 0 is
 *   the chunking of srtSeparateHostStream (max_tiles * T rows per piece, stft_rows = own_rows).
 * -1 with srtLastError() text that names srtSeparateHostStreamOverlap, before any device work and with nothing written: a null argument, unknown flag bits,
 * SRT_HOST_IN_PCM16 with h_in2 != NULL, n < 4096, overlap_rows outside 0..T/2, the Wiener filter on (the text says "Wiener"); -5 when a stem's weights are not set.
 * srtSeparateHostStream*, srtSeparateCli*, srtMultiSeparate* and srtSeparateHostWiener keep their refusals (the filter under an overlap over a host stream: srtSeparateHostWienerOverlap).  Not built: the CLI
 * flows, multi-device ranges, a half-precision carry, graph capture. */
typedef struct srt_host_piece { size_t tile0, tiles, row0, own_rows, stft_rows; } srt_host_piece;
SRT_API size_t srtHostOverlapPieces(size_t rows, int T, int overlap_rows, int max_tiles, srt_host_piece *pieces, size_t max_pieces);
SRT_API int    srtSeparateHostStreamOverlap(srt_engine *e, const void *h_in, const void *h_in2, size_t n, int overlap_rows,
                                            void *h_out, unsigned flags, unsigned long long *h_clipped);

/* ---- host streams at the caller's sample rate: srtSeparateHostStreamIo / srtSeparateHostStreamOverlap for host PCM at in_rate, outputs at
 * out_rate (either may be 44100: no converter on that side).  Both conversions run on the device inside the chunk pipeline, with the built-in filter of
 * srtResamplerCreate, so every sample, at either rate, crosses the bus once and the host holds no 44.1 kHz copy.  h_in, h_in2, flags (SRT_HOST_PINNED |
 * SRT_HOST_IN_PCM16 | SRT_HOST_OUT_PCM16) and h_clipped as in srtSeparateHostStreamIo; n counts frames at in_rate.  overlap_rows as in
 * srtSeparateHostStreamOverlap: it holds for the call only, the engine's srtSetOverlap is neither read nor changed.  ratio_mask, srtSetMaskExtension, srtSetMix
 * and the precision come from the engine.  Synchronous and always eager.
 * What it equals: with n44 = srtResampleLength(n, in_rate, 44100) (n at 44100) and x44 = srtResample of the input, y44 = srtSeparateHostStreamOverlap(e, x44, n44,
 *   overlap_rows, ..) as floats, [outputs][2][len44], len44 = srtIstftLength(srtStftRows(n44)); output pair p is srtResample(44100 -> out_rate) of y44[p] taken as
 *   a signal of len44 frames, all len_out = srtResampleLength(len44, 44100, out_rate) of its frames (len44 at 44100) - bit for bit, up to the sign of a zero.
 *   srtHostRateLength returns len_out.  h_out is float [outputs][2][len_out], or int16 [outputs][len_out][2] with the out flag (srtPcm16Pack's rule, the clipped
 *   counts in h_clipped).  Nothing is pre-shifted or trimmed: the transform's delay is the caller's, as with srtSeparateHostStream.  With both rates 44100 the call
 *   is srtSeparateHostStreamOverlap, launch for launch.
 * How: a piece of srtHostOverlapPieces analyses 44.1 kHz samples [s0, s0 + ns); the source frames their windows reach - [src0, src0 + src_len) - go up into a
 *   staging buffer at in_rate and srtResampleSpans' kernel writes the piece's 44.1 kHz input (a few hundred halo frames per piece go up twice).  Behind the seam
 *   add the piece has finalised samples [fin0, fin1) of every plane; it emits output frames [out0, out1), those whose last weighted tap lies before fin1, from a
 *   carry of the 2 H - 1 samples before fin0 (H = srtResampleHorizon(44100, out_rate)) and its own planes - one launch for all pairs - then packs and downloads.
 *   Staging and carry are grow-only beside the host staging (srtReleaseStaging frees them); the filter of a rate pair is built at the first call that needs it
 *   and kept until srtDestroy.  Timer names: rate_in, rate_out.
 * srtHostRatePieces: the plan, pure host arithmetic, no device.  Returns the piece count and fills pieces[0 .. min(count, max_pieces)) when pieces is not NULL; 0
 *   with srtLastError() text on a bad argument.
 * -1 with srtLastError() text that names srtSeparateHostStreamRate, before any device work and with nothing written: a null argument, unknown flag bits,
 * SRT_HOST_IN_PCM16 with h_in2 != NULL, a rate outside 8000..384000 Hz, n44 < 4096, overlap_rows outside 0..T/2, the Wiener filter on (the text says "Wiener"), a
 * rate pair whose window does not fit LDS (none does with the built-in filter: the check guards a future table); -5 when a stem's weights are not set.
 * Not built: the CLI flows, multi-device ranges, the Wiener stream forms, a caller's table, explicit frames / rows. */
typedef struct srt_host_rate_piece {
    size_t src0, src_len;           /* source frames at in_rate the piece uploads (in_rate 44100: s0, ns) */
    size_t s0, ns;                  /* 44.1 kHz samples the piece analyses */
    size_t fin0, fin1;              /* 44.1 kHz output samples the piece finalises, per plane */
    size_t out0, out1;              /* output frames at out_rate the piece emits (out_rate 44100: fin0, fin1) */
} srt_host_rate_piece;
SRT_API size_t srtHostRateLength(size_t n, int in_rate, int out_rate);   /* frames per output plane; 0 on a bad argument; pure arithmetic */
SRT_API size_t srtHostRatePieces(const srt_config *cfg, size_t n, int in_rate, int out_rate, int overlap_rows,
                                 srt_host_rate_piece *pieces, size_t max_pieces);
SRT_API int    srtSeparateHostStreamRate(srt_engine *e, const void *h_in, const void *h_in2, size_t n, int in_rate, int out_rate,
                                         int overlap_rows, void *h_out, unsigned flags, unsigned long long *h_clipped);

/* ---- one node, several devices: the reference CLI's tile-range fan-out (Executable/main.c:544-673, `processMT`: spawnNthreads workers, each with
 * its own network instance and a contiguous tile range, one shared read-only weight blob) with a GPU where the reference has a CPU thread.
 * One engine per entry of `devices` (an index may repeat: several engines on one GPU), one host thread per engine while a call runs; weights are
 * uploaded once and distributed with one ncclBroadcast per blob over the devices (RCCL, loaded on first use; hipMemcpyPeer when it is absent or
 * SPLEETERRT_NO_RCCL=1); no data-path collective - neighbouring ranges share 3072 output samples, which the call adds on the host when it joins. */
typedef struct srt_span {           /* one rank's share of an n-sample stream; same arithmetic as spleeterrt_amd/stream.py:rank_span */
    size_t tile0, tile1;            /* tiles [tile0, tile1) */
    size_t sample0, nsamples;       /* PCM samples [sample0, sample0 + nsamples): the range + its 3072-sample halo */
    size_t frames, rows;            /* frames that receive a transform / spectrogram rows of the range (srtSeparateEx geometry) */
    size_t out_offset;              /* where the range's overlap-add contribution (rows*1024 + 3072 samples) starts in the output */
} srt_span;
typedef struct srt_multi srt_multi;
SRT_API int  srtDeviceCount(void);                                               /* HIP devices visible to the process (0: none) */
SRT_API int  srtRankSpan(size_t n, int T, int rank, int world, srt_span *out);   /* pure host arithmetic: works without a device */
SRT_API int  srtMultiCreate(const srt_config *cfg, const int *devices /* NULL: 0..ndev-1 */, int ndev, srt_multi **out);  /* cfg->max_tiles: per engine */
SRT_API void srtMultiDestroy(srt_multi *m);
SRT_API int  srtMultiSetCoeffHost(srt_multi *m, int stem, const void *h_coeff);              /* spleeterCoeff, fp32 */
SRT_API int  srtMultiSetCoeffFp16Host(srt_multi *m, int stem, const uint16_t *h_halfs);      /* spleeterQuantizedSubNet */
/* whole host-resident stream, the engine's n_stems sub-networks: h_out [n_stems][2][srtIstftLength(srtStftRows(n))]; flags as srtSeparateHostStreamEx */
SRT_API int  srtMultiSeparateHost(srt_multi *m, const float *h_L, const float *h_R, size_t n, float *h_out, unsigned flags);
/* the offline CLI's flows (srtSeparateCliHost) over the devices: h_out [stems][2][srtIstftLength(srtStftRows(n))] */
SRT_API int  srtMultiSeparateCliHost(srt_multi *m, const float *h_L, const float *h_R, size_t n, int stems, float *h_out);
/* "engines=2 devices=0,1 distinct=2 weights=rccl broadcasts=2" (tests, logs); returns the number of engines */
SRT_API int  srtMultiInfo(const srt_multi *m, char *text, size_t bytes);
/* engine g of the object (borrowed; for srtSetTiming / srtGetTiming* / srtCopyTensor on it), NULL outside [0, engines) */
SRT_API srt_engine *srtMultiEngine(srt_multi *m, int g);
/* Resident throughput of all engines at once, the measurement `bench.py --host native` reports: every worker thread fills `tiles` (<= max_tiles)
 * tiles of synthetic PCM in its device's HBM, runs `warmup` untimed srtSeparate passes, meets the others at a barrier, runs `steps` passes and
 * synchronises its device.  *seconds = first worker released -> last worker done.  seconds_events (may be NULL): the same K passes once more with
 * per-launch HIP events switched on for engine 0 (read them with srtGetTiming(srtMultiEngine(m, 0), ...); timing stays on). */
SRT_API int  srtMultiBenchResident(srt_multi *m, int tiles, int steps, int warmup, double *seconds, double *seconds_events);
/* (with seconds_events != NULL the per-launch timing window of engine 0 stays OPEN after the call so that srtGetTiming / srtGetTimingKernels on
 * srtMultiEngine(m, 0) can read the K event-timed passes; the caller closes it with srtSetTiming(engine, 0)) */

/* ---- sample-rate conversion: the reference program converts every input to 44.1 kHz before separating (Executable/main.c:264-271,
 * JamesDSPOfflineResampling -> libsamplerate's src_simple, the sinc converter of libsamplerate/src_sinc.c:366-512, with the 22 438-point
 * table main.c:133-208 rebuilds at start-up, read with index_inc = 491).  The same arithmetic on the GPU, with the phase of output frame n
 * kept exactly (n * fs_in / fs_out in 64-bit integers) and every frame computed, the last one included.  Planar stereo fp32. */
typedef struct srt_resampler srt_resampler;
/* frames main.c:266 allocates: ceil(n_in * (fs_out / (double)fs_in)); pure arithmetic, no device */
SRT_API size_t srtResampleLength(size_t n_in, int fs_in, int fs_out);
/* current device, like srtCreate.  h_table NULL = built-in filter, else a half filter of table_len floats
 * sampled at index_inc points per input sample (the reference's: 22438, 491).  Rates 8000..384000 Hz.
 * Arguments are checked before any HIP call. */
SRT_API int  srtResamplerCreate(int fs_in, int fs_out, const float *h_table, int table_len, int index_inc,
                                void *stream, srt_resampler **out);
SRT_API int  srtResamplerDestroy(srt_resampler *r);
/* device-resident, asynchronous on the resampler's stream, capturable (no host sync):
 * output frames [out0, out0 + n_out) of the converted stream of the n_in input frames in d_L / d_R
 * (d_R may equal d_L: mono; d_Ro may then equal d_Lo).  A frame's value depends on its index only: any split of a range gives the same bits. */
SRT_API int  srtResample(srt_resampler *r, const float *d_L, const float *d_R, size_t n_in,
                         size_t out0, size_t n_out, float *d_Lo, float *d_Ro);
/* The same frames from a window of the stream (a chunk pipeline holds a span of the signal plus a few hundred frames of history, not the whole input):
 * frames [out0, out0 + n_out) of the converted stream of a signal of n_in frames, of which the device holds two consecutive spans:
 * frames [a0, a0 + a_len) at d_a and [a0 + a_len, a0 + a_len + b_len) at d_b (b_len may be 0; a0 may be negative).
 * `pairs` stereo pairs (1..SRT_MAX_STEMS): pair p's L at d_x + 2p * x_stride, its R at d_x + (2p + 1) * x_stride (x_stride >= x_len).
 * Output pair p's L at d_out + 2p * out_stride, R at + (2p + 1) * out_stride, frame out0 at index 0.
 * Frames outside [0, n_in) are zero, as in srtResample.  One launch computes every pair, and the pairs share each weight load (where `pairs` windows
 * of 64 frames do not fit 64 KiB of LDS: one pair per workgroup, a grid dimension over the pairs).
 * -1 before any launch when a requested frame has a weighted tap on a frame of [0, n_in) that neither span holds; taps 0 .. 2 H - 1 of a frame's window,
 * H = srtResampleHorizon, count as weighted (input frames floor(j * fs_in / fs_out) - H + 1 .. + H).  Also -1: a null resampler or buffer, pairs out of range, a
 * stride below its length, out0 + n_out above 2^44.
 * Asynchronous on the resampler's stream, capturable.
 * Every frame has the bits srtResample gives it. */
SRT_API int  srtResampleSpans(srt_resampler *r, int pairs, const float *d_a, size_t a_stride, long long a0, size_t a_len,
                              const float *d_b, size_t b_stride, size_t b_len, size_t n_in,
                              size_t out0, size_t n_out, float *d_out, size_t out_stride);
/* host buffers, synchronous, the whole stream: h_Lo / h_Ro hold srtResampleLength(n_in, fs_in, fs_out) frames */
SRT_API int  srtResampleHost(srt_resampler *r, const float *h_L, const float *h_R, size_t n_in,
                             float *h_Lo, float *h_Ro);

/* ---- the converter as a stream: fed block by block, it emits every output frame that has become computable.  The converted stream is the one
 * srtResample defines, and the concatenation of what the calls emit equals srtResample on the whole input bit for bit, for any partition into
 * blocks.  Output frame j needs the input up to frame floor(j * fs_in / fs_out) + H, H = srtResampleHorizon (50 input frames for 48 k -> 44.1 k,
 * 46 for 44.1 k -> 48 k with the built-in filter's layout), so after n_in input frames srtResampleComputable(fs_in, fs_out, H, n_in) =
 * ceil((n_in - H) * fs_out / fs_in) frames exist (0 up to n_in = H): host integer arithmetic, no device round trip, capturable.
 * srtResampleHorizon: table_len 0 = the built-in filter's layout (22438, 491); -1 on a bad argument.  Both are pure arithmetic, no device.
 * srtResamplerStreamCreate: current device; `channels` 1..16 share one history ring in HBM; max_block 1..2^20 is the largest n of a call; table as
 * srtResamplerCreate.  Every argument is checked before any HIP call.
 * srtResamplerStreamProcess: d_in holds n frames, interleaved [n][channels] (in_stride 0) or planar with channel c at d_in + c * in_stride; the
 * frames that became computable are written planar, channel c at d_out + c * out_stride, and their count is returned (it is
 * srtResampleComputable(have + n) - srtResampleComputable(have): the caller sizes d_out with that).  One kernel launch, asynchronous on the stream.
 * srtResamplerStreamFlush: the input has ended; emits the frames up to srtResampleLength(frames received) with zeros after the last input frame, as
 * srtResample computes them.  After it only Reset (a new stream from frame 0) and Destroy are accepted. */
typedef struct srt_resampler_stream srt_resampler_stream;
SRT_API int  srtResampleHorizon(int fs_in, int fs_out, int table_len, int index_inc);
SRT_API long long srtResampleComputable(int fs_in, int fs_out, int horizon, long long n_in);
SRT_API int  srtResamplerStreamCreate(int fs_in, int fs_out, int channels, int max_block, const float *h_table, int table_len, int index_inc,
                                      void *stream, srt_resampler_stream **out);
SRT_API int  srtResamplerStreamProcess(srt_resampler_stream *r, const float *d_in, size_t in_stride, int n, float *d_out, size_t out_stride);
SRT_API int  srtResamplerStreamFlush(srt_resampler_stream *r, float *d_out, size_t out_stride);
SRT_API int  srtResamplerStreamReset(srt_resampler_stream *r);
SRT_API int  srtResamplerStreamHorizon(const srt_resampler_stream *r);
SRT_API int  srtResamplerStreamDestroy(srt_resampler_stream *r);

/* ---- live separation with a sliding network window: the real-time surface of Spleeter4Stems.h with a short delay.  The networks run
 * every hops_per_run = K hops (1 <= K <= T) on the window of the newest T frames; frame g takes its mask from the run whose window holds it at row
 * T-1-(h_r-g) with h_r-g in [L, L+K-1], L = lookahead (0 <= L <= T-K frames of future context), and is synthesised D = L + 2K hops after it was
 * analysed.  K = T, L = 0 with the plugin's config is exactly Spleeter4Stems.  Frames near the window's right edge see less future context, so
 * separation quality falls as L approaches 0.
 * srtLiveCreate: current device; cfg honours F, T, n_stems, stem_mode, oob_weight, variant, impl, precision, ratio_mask, batch_invariant; max_tiles
 * must be 1; h_coeff: n_stems spleeterCoeff blobs (copied).  Every argument is checked before any HIP call (-1 with srtLastError() text).  Init does
 * all allocation, graph capture and the pre-warm of the hop path; the Wiener filter is off (srtLiveCreateWiener below turns it on).
 * srtLiveProcess: n samples per channel in, up to n samples written to each of the 2*n_stems planar outputs (stem-major L/R pairs), with the
 * reference's accounting (Spleeter4StemsProcessSamples): one 1024-sample segment per completed hop, a two-segment queue, the queue emitting from the
 * call that completes the first hop and never more than the call's n.  Returns the count written (0..n), negative on a bad argument.  Never
 * allocates or captures; after a device failure (reported once) the stream emits silence with the same accounting.
 * srtLiveLatency: (L + 2K) * 1024 + 1024 samples, the delay for a caller that passes 1024-sample blocks; the first D hops are silence. */
typedef struct srt_live srt_live;
SRT_API int  srtLiveCreate(const srt_config *cfg, int hops_per_run, int lookahead, const void *const *h_coeff, srt_live **out);
SRT_API int  srtLiveProcess(srt_live *s, const float *inL, const float *inR, int n, float *const *out);
SRT_API int  srtLiveLatency(const srt_live *s);
SRT_API void srtLiveDestroy(srt_live *s);
/* The live stream at the host's sample rate.  srtLiveCreateRate: as srtLiveCreate, plus sample_rate 8000..384000 Hz and max_block
 * 1..65536 (the largest slice one call is processed in; any n is accepted).  Both conversions (sample_rate -> 44.1 kHz in front of the hop path,
 * 44.1 kHz -> sample_rate behind it) run on the device with the built-in filter of srtResamplerCreate, as streams (srtResamplerStream* above).
 * On such an instance srtLiveProcess consumes n samples at sample_rate and writes exactly n samples to each plane, every call, and returns n: the
 * output is the separated input delayed by the constant A = srtLiveLatency(s) = srtLiveRateLatency(sample_rate, K, L) samples, bit-identical for
 * every way of cutting the input into calls.  A is the smallest delay that is causal for calls of any size, one sample included:
 * H1 + floor(((D + 2) * 1024 - 1 + H2) * sample_rate / 44100) with D = L + 2K and H1, H2 the horizons of the two converters (srtResampleHorizon)
 * whenever 44100 / gcd is odd (every common rate); (D + 2) * 1024 - 1 at 44100 Hz, where no converter runs.  That is up to one hop more than the
 * 44.1 kHz instance's figure for aligned 1024-sample calls: the price of a delay that does not depend on the chunking.  A call costs one upload,
 * one download and one host wait.  srtLiveRateLatency is pure host arithmetic (-1 on a bad argument). */
SRT_API int  srtLiveCreateRate(const srt_config *cfg, int hops_per_run, int lookahead, int sample_rate, int max_block,
                               const void *const *h_coeff, srt_live **out);
SRT_API int  srtLiveRateLatency(int sample_rate, int hops_per_run, int lookahead);
/* The stem remix and the average mask extension in the hop path.  srtLiveCreateEx is srtLiveCreate / srtLiveCreateRate with options; opts =
 * NULL or all fields zero is srtLiveCreate, sample_rate != 0 with the other fields zero is srtLiveCreateRate, both bit for bit (the same launches).
 * n_out > 0: a call takes and fills 2 * n_out planar planes (pair-major L/R) instead of 2 * n_stems.  At hop h the frame g = h - D is synthesised, for output
 * m, from X(c,k) * h_m(c,k),
 *   h = G[m][n_stems];  for s = 0 .. n_stems-1 (ascending):  h = fmaf(G[m][s], g_s(c,k), h)
 * in fp32, one fused multiply-add per stem (srtSetMix's arithmetic), G = the matrix in force when hop h is processed.  g_s, k < F: the mask value the hop
 * reads with the mix off (after the ratio mask when ratio_mask is set; 1 before the first run is joined).  g_s, k >= F: oob_weight[s], or under
 * SRT_MASK_EXT_AVERAGE e_s(c) = (sum over k < F of g_s(c,k)) / F in srtSetMaskExtension's summation order (exactly 1 before the first join; oob_weight is
 * ignored).  The extension also works with n_out = 0: every stem is written, with e_s(c) above F.  A row that is 1 on stem m reproduces g_s exactly; the
 * row (0, .., 0, 1) is the input delayed by the stream's latency.
 * The number of outputs is fixed at creation (every buffer is sized then; srtLiveProcess still never allocates).  srtLiveSetMix replaces the matrix values
 * (the same n_out; [n_out][n_stems + 1], copied): call it from the thread that calls srtLiveProcess; it does no device work, the matrix travels by value in
 * the next hop's launch.  Frames synthesised later use the new matrix, the kept half of the previous frame the old one: the 50 % overlap-add is the
 * cross-fade between the two.  srtLiveOutputs: the stereo pairs a call writes, n_out while the mix is on, else n_stems; 0 for NULL.
 * Accounting, latency, the silent first D hops and the failure policy (silence, over 2 * srtLiveOutputs planes) are those of srtLiveCreate[Rate].
 * -1 with srtLastError() text, before any HIP call: everything srtLiveCreate / srtLiveCreateRate refuse, n_out outside 0..SRT_MAX_STEMS, n_out > 0 with a
 * null h_gain, an entry that is not finite, an unknown mask_extension; srtLiveSetMix on a null handle, on an instance created with n_out = 0, with a null
 * matrix or a non-finite entry (the old matrix stays in force).  The plugin surface (Spleeter4Stems*) keeps its eight planes and the constant rule. */
typedef struct srt_live_opts {
    int sample_rate;      /* 0: srtLiveCreate's instance (the reference's accounting); else a rate instance, as srtLiveCreateRate */
    int max_block;        /* rate instances only (ignored when sample_rate == 0) */
    int n_out;            /* 0: every stem (off); 1..SRT_MAX_STEMS: outputs of the mix */
    const float *h_gain;  /* [n_out][n_stems + 1], row-major, copied; last column = the unmasked input (srtSetMix's layout) */
    int mask_extension;   /* SRT_MASK_EXT_CONSTANT | SRT_MASK_EXT_AVERAGE */
} srt_live_opts;
SRT_API int srtLiveCreateEx(const srt_config *cfg, int hops_per_run, int lookahead, const srt_live_opts *opts,
                            const void *const *h_coeff, srt_live **out);
SRT_API int srtLiveSetMix(srt_live *s, const float *h_gain);   /* same n_out as at creation; holds from the next hop processed */
SRT_API int srtLiveOutputs(const srt_live *s);                 /* stereo pairs a call writes: n_out while the mix is on, else n_stems; 0 for NULL */
/* The multichannel Wiener filter (srtSetWiener's --mwf) in the live hop path.  srtLiveCreateWiener is srtLiveCreateEx plus `iterations` = n,
 * 0..3, fixed at creation; 0 is srtLiveCreateEx(cfg, K, L, opts, ..): the same launches, the same bits.  With n > 0 the statistics window of a run is its network
 * window: run r, which ends at hop h_r, leaves the tables srtIstftWiener(e, X_r, T, M_r, n, ..) leaves as "wiener_cov", bit for bit - X_r [2][T][2052] the
 * spectrum rows of frames h_r-T+1 .. h_r as the live forward transform stores them, oldest first, zero for frames before 0; M_r [S][2][T][F] the masks the run
 * wrote (floats in every precision) - by the same kernels, chunks and row order.  Frame g, synthesised at hop g + D from the run whose window holds it at row
 * p = T-1-(h_r-g) (the schedule above, unchanged), takes for k < F stem j's spectrum y_j from the filter's chain on (s_L, s_R, M_r[:, :, p, k]) - the soft-mask
 * start, then n EM iterations with run r's tables and a - and for k >= F oob_weight[j] * s, or e_j(c) * s under SRT_MASK_EXT_AVERAGE (the extension follows the
 * mask, not the filter).  With opts->n_out > 0 output m is, per complex component, h = G[m][S] * s; h = fmaf(G[m][j], y_j, h) for j ascending (srtIstftWienerEx's
 * chain) in band and srtLiveCreateEx's gain chain times s above F; srtLiveSetMix works as there, and a one-hot row equals that stem of the instance without a
 * mix bit for bit.  Before the first run is joined the tables are zero and a = 1; only zero spectra are synthesised then, and the chain gives exactly 0.
 * Everything srtLiveCreateEx honours holds (rate instances, the mix, the extension, the engine's precision), as do its accounting, srtLiveLatency, the D silent
 * hops and the failure policy; Init does every allocation, the workspace set-up and the pre-warm of every kernel, srtLiveProcess still never allocates or captures.
 * -1 with srtLastError() text, before any HIP call: everything srtLiveCreateEx refuses, iterations outside 0..3, ratio_mask set with iterations > 0 (both
 * are the post-processing of the masks).  srtLiveWiener: the iterations, 0 while off or for NULL.
 * srtLiveCopyTensor: debug read-back of the run launched last (it waits for both of the instance's streams: not for the audio thread).  *run_hop (may be NULL)
 * receives that run's h_r; while no run has been launched it receives -1, nothing is written and 0 is returned.  "wiener_cov": index = the iteration 1..n,
 * 5 F + 1 floats as srtCopyTensor's (R [F][4], the weight sums [F], a); "wiener_spec": the gathered window [2][T][2052] complex, 2 * T * 2052 * 2 floats;
 * "masks": the stem's [2][T][F].  Returns the float count; -1 for a null handle, name or buffer, an unknown name, a stem outside the stems, an index outside
 * the iterations, a buffer that is too small, "wiener_*" on an instance without the filter. */
SRT_API int srtLiveCreateWiener(const srt_config *cfg, int hops_per_run, int lookahead, const srt_live_opts *opts /* may be NULL */,
                                int iterations, const void *const *h_coeff, srt_live **out);
SRT_API int srtLiveWiener(const srt_live *s);      /* iterations, 0 while off or for NULL */
SRT_API int srtLiveCopyTensor(srt_live *s, const char *name, int stem, int index, float *h_dst, size_t max_floats, long long *run_hop);

/* debug / measurement */
SRT_API int  srtCopyTensor(srt_engine *e, const char *name, int stem, int tile, float *h_dst, size_t max_floats); /* "conv1".."conv6","act1".."act5","up1".."up6";
                                                                                                                   "wiener_cov": tile = 4 * track + iteration (see srtIstftWiener);
                                                                                                                   after srtSeparateBatch: packed tile indices */
SRT_API int  srtSetTiming(srt_engine *e, int enable);                    /* record HIP events around every launch of the next calls */
SRT_API int  srtGetTiming(srt_engine *e, char *names, size_t names_bytes, float *ms, int max_entries); /* returns count; syncs the stream */
/* which kernel ran each of those launches (same order), ';'-separated, named as rocprofv3 names kernels ("srt_dec_wino<4, 16, 1, 0>"):
 * the dispatch depends on batch size and geometry, so tests and bench.py read it from here instead of assuming it.  Returns the count. */
SRT_API int  srtGetTimingKernels(srt_engine *e, char *kernels, size_t kernels_bytes);

#ifdef __cplusplus
}
#endif
#endif
