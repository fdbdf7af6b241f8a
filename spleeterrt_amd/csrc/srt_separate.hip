// srt_separate.hip — the offline transforms, the Wiener filter, srtSeparate and the device-resident CLI flows of the engine (its private declarations: srt_engine.h).
#include "srt_engine.h"

int srtRatioMask(srt_engine* e, float* d_masks, int ntiles)
{
    if (!e || !d_masks || ntiles < 1) return fail(-1, "srtRatioMask: bad argument");
    DeviceScope ds(e->device);
    TimerScope ts(e, "ratio");
    if (srt_launch_ratio_mask(d_masks, e->cfg.n_stems, (size_t)ntiles * 2 * e->cfg.T * e->cfg.F, e->stream)) return fail(-2, "ratio-mask launch failed");
    return 0;
}

SrtDspTables tables_of(const srt_engine* e) { SrtDspTables t; t.preWin = e->preWin; t.postWin = e->postWin; t.twiddle = e->twiddle; return t; }

// the transform behind srtStftEx with the overlap of the magnitude layout as an argument (ov: the engine's srtSetOverlap for srtStftEx, the call's own for srtSeparateWiener)
static int stft_issue(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_spec, float* d_mag, int ov)
{
    if (!e || !d_L || !d_R || !d_spec) return fail(-1, "srtStft: null argument");
    DeviceScope ds(e->device);
    if (rows < 1 || frames > rows) return fail(-1, "srtStft: need 1 <= frames <= rows");
    const int T = e->cfg.T, O = d_mag ? ov : 0;
    const size_t ntiles = overlap_tiles(rows, T, ov);
    if (d_mag && ntiles > (size_t)e->cfg.max_tiles) return fail(-1, ov ? "srtStft: more than max_tiles tiles at this overlap (srtOverlapTiles)" : "srtStft: more than max_tiles * T rows");
    SrtStftParams p; memset(&p, 0, sizeof p);
    p.L = d_L; p.R = d_R; p.nsamples = n;
    p.frames_computed = (int)frames;
    p.rows_total = (int)rows;
    p.spec = (float2*)d_spec; p.spec_ch_stride = rows * SRT_SPEC_LD;
    p.mag = nullptr; p.T = T; p.F = e->cfg.F; p.tab = tables_of(e);
    if (d_mag) {
        // magnitude rows exist for whole tiles: rows..ntiles*T are zero (main.c:507-514); overlapped tiles end at row (ntiles - 1) (T - O) + T
        p.mag = d_mag;
        if ((ntiles - 1) * (T - O) + T > rows) HIPCHK(hipMemsetAsync(d_mag, 0, ntiles * 2 * (size_t)T * e->cfg.F * sizeof(float), e->stream));
    }
    TimerScope ts(e, "stft");
    if (srt_launch_stft(p, e->stream, O, (int)ntiles)) return fail(-2, "stft launch failed");
    return 0;
}

int srtStftEx(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_spec, float* d_mag)
{
    if (!e) return fail(-1, "srtStft: null argument");
    return stft_issue(e, d_L, d_R, n, frames, rows, d_spec, d_mag, e->overlap);
}

int srtStft(srt_engine* e, const float* d_L, const float* d_R, size_t n, float* d_spec, float* d_mag)
{
    if (n < SRT_FFT) return fail(-1, "srtStft: need at least 4096 samples");          // the reference underflows here (stftFix.c:378)
    return srtStftEx(e, d_L, d_R, n, srtStftFrames(n), srtStftRows(n), d_spec, d_mag);
}

// average mask extension: the gain table of the inverse transform that follows on the same stream, from the masks that transform will apply
// (rows <= rows_cap: every caller has checked its tiles against max_tiles)
// (tracks: a packed batch with overlapped tiles - rows = the packed rows, each mapped inside its own track: srt_launch_mask_ext_batch)
int mask_ext_issue(srt_engine* e, const float* masks, int masks16, int nstems, int ntiles, int rows, int ratio, int O, const SrtBatchTrack* tracks, int ntracks)
{
    if (!e->ext || (size_t)rows > e->rows_cap || nstems != e->cfg.n_stems) return fail(-1, "mask extension: no gain table for this call (srtSetMaskExtension allocates it for n_stems x max_tiles * T rows)");
    SrtMaskExtParams m; memset(&m, 0, sizeof m);
    m.masks = masks; m.masks16 = masks16; m.nstems = nstems; m.ntiles = ntiles; m.T = e->cfg.T; m.F = e->cfg.F; m.rows = rows; m.ratio = ratio;
    m.ext = e->ext; m.ext_stem = e->rows_cap * 2;
    TimerScope ts(e, "mask_ext");
    if (tracks ? srt_launch_mask_ext_batch(m, tracks, ntracks, e->stream, O) : srt_launch_mask_ext(m, e->stream, O)) return fail(-2, "mask extension launch failed (the masks must be 16-byte aligned)");
    e->last.ext_rows = rows;
    return 0;
}

// inverse transform of `nstems` stems of one spectrum under their masks (nullptr: all-ones) into [nstems][2][srtIstftLength(rows)]; oob: per stem, the weight of bins >= F
// mix (srtSetMix; only istft_issue sets it): d_out is [mix_out][2][len], output m the chain of e->mix[m] over the stems' gains
// ext_mode: the rule for bins >= F - the engine's own (srtSetMaskExtension) unless the caller names one (the Wiener option calls, whose options hold for the call only)
static int istft_launch(srt_engine* e, const float2* spec, size_t rows, const float* masks, int nstems, const float* oob, bool ratio, bool masks16, float* d_out, bool mix = false, int ext_mode = -1)
{
    DeviceScope ds(e->device);
    const int T = e->cfg.T;
    SrtIstftParams p; memset(&p, 0, sizeof p);
    p.spec = spec; p.spec_ch_stride = rows * SRT_SPEC_LD;
    const int O = masks ? e->overlap : 0;               // (the single-stem callers - CLI flows, Wiener filter - refuse an overlap before they get here)
    p.frames = (int)rows; p.masks = masks; p.nstems = nstems; p.ntiles = (int)(O ? tiles_of(e, rows) : (rows + T - 1) / T);
    p.T = T; p.F = e->cfg.F;
    const bool ext = (ext_mode < 0 ? e->mask_ext : ext_mode) == SRT_MASK_EXT_AVERAGE;      // (its single-stem callers - CLI flows, Wiener filter - refuse the mode before they get here)
    for (int s = 0; s < nstems; ++s) p.oob[s] = ext ? 1.0f : oob[s];     // the mean of an all-ones mask is 1 exactly: no table without masks
    p.ratio = ratio ? 1 : 0; p.masks16 = masks16 ? 1 : 0;
    p.frames_out = nullptr; p.out = d_out; p.out_len = srtIstftLength(rows); p.tab = tables_of(e);
    if (mix) { p.n_out = e->mix_out; memcpy(p.mix, e->mix, sizeof p.mix); }
    if (ext && masks) {
        const int rc = mask_ext_issue(e, masks, p.masks16, nstems, p.ntiles, (int)rows, p.ratio, O);
        if (rc) return rc;
        p.ext = e->ext; p.ext_stem = e->rows_cap * 2;
    }
    TimerScope ts(e, "istft");
    if (srt_launch_istft(p, e->stream, O)) return fail(-2, "istft launch failed");
    return 0;
}
// ONE stem's mask (or none) into a [2][len] destination
static int istft_one(srt_engine* e, const float2* spec, size_t rows, const float* mask_stem, float oob, float* d_dst, int ext_mode = -1) { return istft_launch(e, spec, rows, mask_stem, 1, &oob, false, false, d_dst, false, ext_mode); }
static int istft_issue(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, float* d_out, bool ratio, bool masks16 = false)
{
    if (!e || !d_spec || !d_out) return fail(-1, "srtIstft: null argument");
    if (rows < 1) return fail(-1, "srtIstft: no rows");
    if (d_masks && tiles_of(e, rows) > (size_t)e->cfg.max_tiles) return fail(-1, e->overlap ? "srtIstft: more than max_tiles tiles at this overlap (srtOverlapTiles)" : "srtIstft: rows exceed max_tiles * T");
    return istft_launch(e, (const float2*)d_spec, rows, d_masks, e->cfg.n_stems, e->cfg.oob_weight, ratio, masks16, d_out, e->mix_out > 0);
}
// (the public entry applies the masks as they are given: srtRatioMask is its caller's business)
int srtIstft(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, float* d_out) { return istft_issue(e, d_spec, rows, d_masks, d_out, false); }

// ---- multichannel Wiener filter (srt_wiener.hip)
static size_t wiener_slab_floats(const srt_engine* e) { return (size_t)SRT_WIENER_MAX_CHUNKS * e->cfg.n_stems * 4 * e->cfg.F + (size_t)SRT_WIENER_MAX_CHUNKS * SRT_WIENER_BINBLK; }
static size_t wiener_tab_floats(const srt_engine* e) { return (size_t)SRT_WIENER_MAX_ITERS * e->cfg.n_stems * e->cfg.F * 5 + 4; }

// the statistics slab, the R tables and the S filtered spectra for max_tiles tiles - allocated once (srtSetWiener, or the first srtIstftWiener), never
// inside a capture, kept until srtDestroy (a captured graph holds these addresses)
static int ensure_wiener_ws(srt_engine* e)
{
    if (e->wslab && e->wtab && e->wspec) return 0;
    if (stream_capturing(e)) return fail(-1, "Wiener filter: workspace not allocated (call srtSetWiener before capturing)");
    SrtSetupLock setup;
    if (!e->wslab) HIPCHK(hipMalloc((void**)&e->wslab, wiener_slab_floats(e) * sizeof(float)));
    if (!e->wtab) {
        HIPCHK(hipMalloc((void**)&e->wtab, wiener_tab_floats(e) * sizeof(float)));
        HIPCHK(hipMemset(e->wtab, 0, wiener_tab_floats(e) * sizeof(float)));
    }
    if (!e->wspec) HIPCHK(hipMalloc((void**)&e->wspec, (size_t)e->cfg.n_stems * 2 * e->rows_cap * SRT_SPEC_LD * sizeof(float2)));
    return 0;
}

// statistics passes (one stats + one finalize launch per iteration), the filter, then one inverse transform per stem on its filtered spectrum
// (no masks: all-ones in band; bins >= F get oob_weight as with masks).  The statistics window is exactly the `rows` rows of this call.
// opt (srtIstftWienerEx / srtSeparateWiener): the call's own options, checked by wiener_opts_check - the engine's srtSetOverlap / srtSetMaskExtension /
// srtSetMix state is not read then.  With every option off the launches are the ones of a call without `opt`; with an overlap the statistics run on blended masks
// (srt_wiener_stats_ov_kernel), and with any option the filter writes final spectra (srt_wiener_filter_opt_kernel) of the n_out mixes or of every stem, which the
// inverse transforms without a gain.  d_masks: [S][overlap_tiles(rows, T, overlap)][2][T][F].
struct WienerCall { int overlap, ext, n_out; float mix[SRT_MAX_STEMS][SRT_MAX_STEMS + 1]; };
static int wiener_issue(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, int iters, float* d_out, const WienerCall* opt = nullptr)
{
    const int T = e->cfg.T, S = e->cfg.n_stems, F = e->cfg.F;
    const int O = opt ? opt->overlap : 0;
    const bool plain = !opt || (!O && !opt->ext && !opt->n_out);
    SrtWienerParams w; memset(&w, 0, sizeof w);
    w.spec = (const float2*)d_spec; w.spec_ch_stride = rows * SRT_SPEC_LD; w.rows = (int)rows;
    w.masks = d_masks; w.nstems = S; w.ntiles = (int)overlap_tiles(rows, T, O); w.T = T; w.F = F;
    int nch = (int)((rows + 15) / 16); if (nch > SRT_WIENER_MAX_CHUNKS) nch = SRT_WIENER_MAX_CHUNKS;
    w.rpc = (int)((rows + nch - 1) / nch); w.nchunks = (int)((rows + w.rpc - 1) / w.rpc);
    w.slab = e->wslab; w.slab_max = e->wslab + (size_t)SRT_WIENER_MAX_CHUNKS * S * 4 * F;
    w.rtab = e->wtab; w.wsum = e->wtab + (size_t)SRT_WIENER_MAX_ITERS * S * F * 4; w.scal = w.wsum + (size_t)SRT_WIENER_MAX_ITERS * S * F;
    w.out = e->wspec; w.out_stem = 2 * rows * SRT_SPEC_LD;
    for (int pass = 1; pass <= iters; ++pass) {
        { TimerScope ts(e, "wiener_stats"); if (O ? srt_launch_wiener_stats_ov(w, O, pass, e->stream) : srt_launch_wiener_stats(w, pass, e->stream)) return fail(-2, "Wiener statistics launch failed"); }
        { TimerScope ts(e, "wiener_cov"); if (srt_launch_wiener_finalize(w, pass, e->stream)) return fail(-2, "Wiener finalize launch failed"); }
    }
    const size_t len = srtIstftLength(rows);
    // (an option call names the constant rule for its mask-free inverse transforms: the engine's srtSetMaskExtension mode is not read)
    const int ext_mode = opt ? SRT_MASK_EXT_CONSTANT : -1;
    if (plain) {
        { TimerScope ts(e, "wiener_filter"); if (srt_launch_wiener_filter(w, iters, e->stream)) return fail(-2, "Wiener filter launch failed"); }
        e->last.wiener_last = iters; e->last.wiener_tracks = 0;
        for (int j = 0; j < S; ++j) {
            const int rc = istft_one(e, e->wspec + (size_t)j * w.out_stem, rows, nullptr, e->cfg.oob_weight[j], d_out + (size_t)j * 2 * len, ext_mode);
            if (rc) return rc;
        }
        return 0;
    }
    SrtWienerOpt q; memset(&q, 0, sizeof q);
    q.overlap = O; q.n_out = opt->n_out;
    memcpy(q.oob, e->cfg.oob_weight, sizeof q.oob);
    memcpy(q.mix, opt->mix, sizeof q.mix);
    if (opt->ext) {      // e_j(r, c): the table the inverse transform's own kernel writes from the same (blended) masks, ratio = 0
        const int rc = mask_ext_issue(e, d_masks, 0, S, w.ntiles, (int)rows, 0, O);
        if (rc) return rc;
        q.ext = e->ext; q.ext_stem = e->rows_cap * 2;
    }
    { TimerScope ts(e, "wiener_filter"); if (srt_launch_wiener_filter_opt(w, q, iters, e->stream)) return fail(-2, "Wiener filter launch failed"); }
    e->last.wiener_last = iters; e->last.wiener_tracks = 0;
    for (int m = 0; m < (q.n_out ? q.n_out : S); ++m) {      // the spectra are final: no gain in the inverse
        const int rc = istft_one(e, e->wspec + (size_t)m * w.out_stem, rows, nullptr, 1.0f, d_out + (size_t)m * 2 * len, ext_mode);
        if (rc) return rc;
    }
    return 0;
}

// the checks srtIstftWienerEx and srtSeparateWiener share (`who` names the caller): 0 with *c filled, or -1 with the error text set; no device work
static int wiener_opts_check(const srt_engine* e, const char* who, const srt_wiener_opts* o, size_t rows, WienerCall* c)
{
    const int T = e->cfg.T, S = e->cfg.n_stems;
    if (o->iterations < 1 || o->iterations > SRT_WIENER_MAX_ITERS) return fail(-1, "%s: iterations must be 1..3", who);
    if (o->overlap_rows < 0 || o->overlap_rows > T / 2) return fail(-1, "%s: overlap_rows must be 0 .. T / 2", who);
    if (o->mask_extension != SRT_MASK_EXT_CONSTANT && o->mask_extension != SRT_MASK_EXT_AVERAGE) return fail(-1, "%s: mask_extension must be SRT_MASK_EXT_CONSTANT (0) or SRT_MASK_EXT_AVERAGE (1)", who);
    if (o->n_out < 0 || o->n_out > S) return fail(-1, "%s: n_out must be 0 (every stem) .. n_stems (the filter's spectrum workspace holds n_stems spectra; more outputs are a follow-up)", who);
    if (o->n_out && !o->h_gain) return fail(-1, "%s: null gain matrix with n_out > 0", who);
    for (int i = 0; i < o->n_out * (S + 1); ++i) if (!isfinite(o->h_gain[i])) return fail(-1, "%s: every gain must be finite", who);
    if (e->cfg.ratio_mask) return fail(-1, "%s: the Wiener filter and ratio_mask exclude each other (both are the post-processing of the masks)", who);
    if (rows < 1 || overlap_tiles(rows, T, o->overlap_rows) > (size_t)e->cfg.max_tiles)
        return fail(-1, o->overlap_rows ? "%s: the signal takes more than max_tiles tiles at this overlap (srtOverlapTiles)" : "%s: need 1 <= rows <= max_tiles * T", who);
    memset(c, 0, sizeof *c);
    c->overlap = o->overlap_rows; c->ext = o->mask_extension; c->n_out = o->n_out;
    for (int m = 0; m < o->n_out; ++m) for (int s = 0; s <= S; ++s) c->mix[m][s] = o->h_gain[m * (S + 1) + s];
    return 0;
}

// the workspaces of an option call: the filter's, and with the average extension the engine's gain table (srtSetMaskExtension's, same size, kept until srtDestroy)
static int ensure_wiener_opts_ws(srt_engine* e, const char* who, const WienerCall& c)
{
    const int rc = ensure_wiener_ws(e);
    if (rc) return rc;
    if (c.ext && !e->ext) {
        if (stream_capturing(e)) return fail(-1, "%s: the mask extension's gain table is not allocated yet (srtSetMaskExtension, or one call outside the capture)", who);
        SrtSetupLock setup;
        HIPCHK(hipMalloc((void**)&e->ext, (size_t)e->cfg.n_stems * e->rows_cap * 2 * sizeof(float)));
    }
    return 0;
}

int srtIstftWienerEx(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, const srt_wiener_opts* opts, float* d_out)
{
    if (!e || !d_spec || !d_masks || !opts || !d_out) return fail(-1, "srtIstftWienerEx: null argument");
    DeviceScope ds(e->device);
    WienerCall c;
    int rc = wiener_opts_check(e, "srtIstftWienerEx", opts, rows, &c);
    if (rc) return rc;
    if ((rc = ensure_wiener_opts_ws(e, "srtIstftWienerEx", c))) return rc;
    return wiener_issue(e, d_spec, rows, d_masks, opts->iterations, d_out, &c);
}

// srtSeparate's stages with the call's own options: one STFT in the overlapped layout, one forward over its tiles (fp32 masks in the fp16 mode too, as with
// srtSetWiener), the filter.  Always eager: the graph cache has no key for the options.
int srtSeparateWiener(srt_engine* e, const float* d_L, const float* d_R, size_t n, const srt_wiener_opts* opts, float* d_out)
{
    if (!e || !d_L || !d_R || !opts || !d_out) return fail(-1, "srtSeparateWiener: null argument");
    if (n < SRT_FFT) return fail(-1, "srtSeparateWiener: need at least 4096 samples");
    DeviceScope ds(e->device);
    const size_t rows = srtStftRows(n), frames = srtStftFrames(n);
    WienerCall c;
    int rc = wiener_opts_check(e, "srtSeparateWiener", opts, rows, &c);
    if (rc) return rc;
    for (int s = 0; s < e->cfg.n_stems; ++s) if (!e->have_coeff[s]) return fail(-5, "srtSeparateWiener: weights not set for every stem");
    if ((rc = ensure_wiener_opts_ws(e, "srtSeparateWiener", c))) return rc;
    const SrtSwitches sw = srt_read_switches();
    const size_t ntiles = overlap_tiles(rows, e->cfg.T, c.overlap);
    if ((rc = stft_issue(e, d_L, d_R, n, frames, rows, (float*)e->spec, e->mag, c.overlap))) return rc;
    if ((rc = forward_range(e, sw, e->mag, (int)ntiles, e->masks, 0, e->cfg.n_stems, false))) return rc;
    return wiener_issue(e, (const float*)e->spec, rows, e->masks, opts->iterations, d_out, &c);
}

int srtIstftWiener(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, int iterations, float* d_out)
{
    if (!e || !d_spec || !d_masks || !d_out) return fail(-1, "srtIstftWiener: null argument");
    DeviceScope ds(e->device);
    if (iterations < 1 || iterations > SRT_WIENER_MAX_ITERS) return fail(-1, "srtIstftWiener: iterations must be 1..3");
    if (e->mix_out) return fail(-1, MIX_REFUSED, "srtIstftWiener");
    if (e->overlap) return fail(-1, OVERLAP_REFUSED, "srtIstftWiener");      // its kernels index masks by (row / T, row % T)
    if (e->mask_ext) return fail(-1, MASK_EXT_REFUSED, "srtIstftWiener");    // the filter's own gains above F would have to be defined first
    if (rows < 1 || (rows + e->cfg.T - 1) / e->cfg.T > (size_t)e->cfg.max_tiles) return fail(-1, "srtIstftWiener: need 1 <= rows <= max_tiles * T");
    const int rc = ensure_wiener_ws(e);
    if (rc) return rc;
    return wiener_issue(e, d_spec, rows, d_masks, iterations, d_out);
}

int srtSetWiener(srt_engine* e, int iterations)
{
    if (!e) return fail(-1, "srtSetWiener: null engine");
    if (iterations < 0 || iterations > SRT_WIENER_MAX_ITERS) return fail(-1, "srtSetWiener: iterations must be 0 (off) or 1..3");
    if (iterations && e->cfg.ratio_mask) return fail(-1, "srtSetWiener: the Wiener filter and ratio_mask exclude each other (both are the post-processing of the masks)");
    if (iterations && e->mask_ext) return fail(-1, MASK_EXT_REFUSED, "srtSetWiener");
    if (iterations && e->mix_out) return fail(-1, MIX_REFUSED, "srtSetWiener");
    DeviceScope ds(e->device);
    if (iterations) { const int rc = ensure_wiener_ws(e); if (rc) return rc; }
    e->wiener = iterations;
    return 0;
}

int srt_engine_wiener(const srt_engine* e) { return e->wiener; }

// fp16 mode: the masks between the head and the inverse transform - the engine's own buffer, never seen by a caller - are halves where both kernels take them
// (srt_head_rows_kernel<.., true> / srt_istft_ola3_kernel<.., true>: F <= 1024, no ratio mask, no Wiener filter (fp32 masks), head launches of >= 1024
// workgroups: srt_head_out16_ok; sw.m16 = 0: floats, for A/B runs)
// (nor with the stem remix: there is no half-mask MIX kernel)
bool masks16_wanted(const srt_engine* e, const SrtSwitches& sw) { return e->cfg.precision == SRT_PREC_F16 && e->act16 && !e->cfg.ratio_mask && !e->wiener && !e->mix_out && e->cfg.F <= 1024 && sw.m16; }

static int separate_issue(srt_engine* e, const SrtSwitches& sw, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_out)
{
    const size_t ntiles = tiles_of(e, rows);            // overlapped tiles: the three stages agree on the layout through e->overlap
    int rc = srtStftEx(e, d_L, d_R, n, frames, rows, (float*)e->spec, e->mag);
    if (rc) return rc;
    rc = forward_range(e, sw, e->mag, (int)ntiles, e->masks, 0, e->cfg.n_stems, masks16_wanted(e, sw));
    if (rc) return rc;
    if (e->wiener) return wiener_issue(e, (const float*)e->spec, rows, e->masks, e->wiener, d_out);
    // ratio_mask: normalised across the stems inside the inverse kernel's prologue (srt_ratio_of, srt_dsp.hip) - e->masks keeps the raw sigmoid masks
    return istft_issue(e, (const float*)e->spec, rows, e->masks, d_out, e->cfg.ratio_mask != 0, e->last.masks16);
}

int srtSeparateEx(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_out)
{
    if (!e) return fail(-1, "srtSeparate: null engine");
    const size_t ntiles = tiles_of(e, rows);
    if (rows < 1 || ntiles > (size_t)e->cfg.max_tiles) return fail(-1, e->overlap ? "srtSeparate: the signal takes more than max_tiles tiles at this overlap (srtOverlapTiles)" : "srtSeparate: signal longer than max_tiles * T frames");
    if (e->overlap && e->wiener) return fail(-1, OVERLAP_REFUSED, "srtSeparate with the Wiener filter on");
    const SrtSwitches sw = srt_read_switches();
    if (!e->graph_mode) return separate_issue(e, sw, d_L, d_R, n, frames, rows, d_out);
    DeviceScope ds(e->device);
    GraphKey k;
    const bool valid = graph_prepare(e, d_L && d_R && d_out && frames <= rows, ntiles, 2, sw, &k);
    k.p0 = d_L; k.p1 = d_R; k.p2 = d_out; k.n = n; k.frames = frames; k.rows = rows; k.wiener = e->wiener; k.overlap = e->overlap; k.mask_ext = e->mask_ext;
    k.mix_gen = e->mix_out ? e->mix_gen : 0;
    return run_graphed(e, k, valid, [&]() { return separate_issue(e, sw, d_L, d_R, n, frames, rows, d_out); });
}

int srtSeparate(srt_engine* e, const float* d_L, const float* d_R, size_t n, float* d_out)
{
    if (n < SRT_FFT) return fail(-1, "srtSeparate: need at least 4096 samples");
    return srtSeparateEx(e, d_L, d_R, n, srtStftFrames(n), srtStftRows(n), d_out);
}

// The offline CLI's separation flows, device resident (Executable/main.c:776-798 two outputs, :845-928 three outputs).
// Sub-network 0 is the CLI's net[0] (drum, mode 1), sub-network 1 its net[1] (vocal, mode 0)  (main.c:759-760).
//   2: vocal = istft(mask1 . S);  accompaniment = input - vocal                                  (time-domain residual)
//   3: drum = istft(mask0 . S);  R = S - mask0 . S;  vocal = istft(mask1(|R|) . R);  accompaniment = istft(R) - vocal
// d_out: [stems][2][srtIstftLength(rows)] in the CLI's file order: (Vocal, Accompaniment) or (Drum, Vocal, Accompaniment).
// Explicit geometry as srtSeparateEx (a tile range of a longer file).  residual_now = false leaves the last, time-domain subtraction
// to the caller: the chunked pipeline first adds the previous chunk's overlap to every plane (the accompaniment slot then holds
// the UNsubtracted term: nothing for 2 outputs, istft(R) for 3) and subtracts afterwards (cli_time_residual).
// samples [lo, hi) of the planes (hi = 0: all of them)
int cli_time_residual(srt_engine* e, const float* d_L, const float* d_R, size_t n, int stems, float* d_out, size_t len, size_t lo, size_t hi)
{
    TimerScope ts(e, "residual");
    if (!hi) hi = len;
    const int rc = stems == 2 ? srt_launch_time_residual(d_L, d_R, n, d_out, len, d_out + 2 * len, lo, hi, e->stream)
                              : srt_launch_time_residual(d_out + 4 * len, d_out + 5 * len, len, d_out + 2 * len, len, d_out + 4 * len, lo, hi, e->stream);
    return rc ? fail(-2, "residual launch failed") : 0;
}

int cli_issue(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, int stems, float* d_out, bool residual_now)
{
    const int T = e->cfg.T;
    const size_t ntiles = (rows + T - 1) / T, len = srtIstftLength(rows);
    const size_t HW2 = 2 * (size_t)T * e->cfg.F;
    float* mask0 = e->masks;                                  // stem stride of this batch = ntiles instances
    float* mask1 = e->masks + ntiles * HW2;
    const SrtSwitches sw = srt_read_switches();
    int rc = srtStftEx(e, d_L, d_R, n, frames, rows, (float*)e->spec, e->mag);
    if (rc) return rc;
    if (stems == 2) {
        if ((rc = forward_range(e, sw, e->mag, (int)ntiles, e->masks, 1, 1))) return rc;
        if ((rc = istft_one(e, e->spec, rows, mask1, e->cfg.oob_weight[1], d_out))) return rc;
        return residual_now ? cli_time_residual(e, d_L, d_R, n, stems, d_out, len) : 0;
    }
    if (!e->spec2) HIPCHK(hipMalloc((void**)&e->spec2, (size_t)2 * e->rows_cap * SRT_SPEC_LD * sizeof(float2)));
    if ((rc = forward_range(e, sw, e->mag, (int)ntiles, e->masks, 0, 1))) return rc;
    if ((rc = istft_one(e, e->spec, rows, mask0, e->cfg.oob_weight[0], d_out))) return rc;                 // Drum
    {
        SrtResidualParams r; memset(&r, 0, sizeof r);
        r.spec = e->spec; r.res = e->spec2; r.spec_ch_stride = rows * SRT_SPEC_LD; r.rows = (int)rows; r.T = T; r.F = e->cfg.F;
        r.mask = mask0; r.oob = e->cfg.oob_weight[0]; r.mag = e->mag;
        TimerScope ts(e, "residual");
        if (srt_launch_residual(r, e->stream)) return fail(-2, "residual launch failed");
    }
    if ((rc = istft_one(e, e->spec2, rows, nullptr, 1.0f, d_out + 4 * len))) return rc;                      // accompaniment + vocal
    if ((rc = forward_range(e, sw, e->mag, (int)ntiles, e->masks, 1, 1))) return rc;
    if ((rc = istft_one(e, e->spec2, rows, mask1, e->cfg.oob_weight[1], d_out + 2 * len))) return rc;       // Vocal
    return residual_now ? cli_time_residual(e, d_L, d_R, n, stems, d_out, len) : 0;
}

int cli_check(srt_engine* e, int stems)
{
    if (stems != 2 && stems != 3) return fail(-1, "srtSeparateCli: stems must be 2 or 3");
    if (e->cfg.n_stems < 2) return fail(-1, "srtSeparateCli: the engine needs sub-networks 0 (drum) and 1 (vocal)");
    if (e->cfg.ratio_mask) return fail(-1, "srtSeparateCli: ratio_mask does not apply to the CLI flows (the sub-networks see different inputs)");
    if (e->overlap) return fail(-1, OVERLAP_REFUSED, "srtSeparateCli");       // the residual chain reads masks and writes the second network's magnitudes by tile
    if (e->mix_out) return fail(-1, MIX_REFUSED, "srtSeparateCli");           // the flows have no stem axis to mix over
    if (e->mask_ext) return fail(-1, MASK_EXT_REFUSED, "srtSeparateCli");     // the complex-domain residual chain subtracts oob * spec (srt_residual_kernel)
    if (e->wiener) return fail(-1, "srtSeparateCli: the Wiener filter does not apply to the CLI flows (the sub-networks see different inputs, and its statistics span the whole signal)");
    return 0;
}

int srtSeparateCli(srt_engine* e, const float* d_L, const float* d_R, size_t n, int stems, float* d_out)
{
    if (!e || !d_L || !d_R || !d_out) return fail(-1, "srtSeparateCli: null argument");
    DeviceScope ds(e->device);
    int rc = cli_check(e, stems);
    if (rc) return rc;
    if (n < SRT_FFT) return fail(-1, "srtSeparateCli: need at least 4096 samples");
    const int T = e->cfg.T;
    const size_t rows = srtStftRows(n), frames = srtStftFrames(n), ntiles = (rows + T - 1) / T;
    if (ntiles > (size_t)e->cfg.max_tiles) return fail(-1, "srtSeparateCli: signal longer than max_tiles * T frames (srtSeparateCliHost walks longer files chunk by chunk)");
    return cli_issue(e, d_L, d_R, n, frames, rows, stems, d_out, true);
}
