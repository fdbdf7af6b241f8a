// srt_batch.hip — the packed-batch entry points of the engine: the batch plans, the track tables, srtSeparateBatch / Overlap / Mix / Wiener / WienerEx (its private declarations: srt_engine.h).
#include "srt_engine.h"

// ---- packed batch of independent tracks (srt_dsp.hip: srt_stft_batch_kernel / srt_istft_batch_kernel)
// the plan of checked tracks: track k takes overlap_tiles(rows_k, T, O) packed tiles from tile0[k] on (O = 0: ceil(rows_k / T)); returns their sum
static size_t plan_tiles(const size_t* n, int ntracks, int T, int O, size_t* tile0)
{
    size_t t = 0;
    for (int k = 0; k < ntracks; ++k) {
        if (tile0) tile0[k] = t;
        t += overlap_tiles(srtStftRows(n[k]), T, O);
    }
    return t;
}

int srtBatchPlan(const size_t* n, int ntracks, int T, size_t* tile0, size_t* total_tiles)
{
    if (!n || !total_tiles || ntracks < 1 || T < 1) return fail(-1, "srtBatchPlan: need ntracks >= 1, T >= 1, n and total_tiles");
    for (int k = 0; k < ntracks; ++k) if (n[k] < SRT_FFT) return fail(-1, "srtBatchPlan: every track needs at least 4096 samples");
    *total_tiles = plan_tiles(n, ntracks, T, 0, tile0);
    return 0;
}

// the same with overlapped tiles inside every track (srtSeparateBatchOverlap); O = 0 is srtBatchPlan
int srtBatchPlanOverlap(const size_t* n, int ntracks, int T, int overlap_rows, size_t* tile0, size_t* total_tiles)
{
    if (!n || !total_tiles || ntracks < 1 || T < 1) return fail(-1, "srtBatchPlanOverlap: need ntracks >= 1, T >= 1, n and total_tiles");
    if (!overlap_ok(overlap_rows, T)) return fail(-1, "srtBatchPlanOverlap: the overlap must be 0 .. T / 2 rows");
    for (int k = 0; k < ntracks; ++k) if (n[k] < SRT_FFT) return fail(-1, "srtBatchPlanOverlap: every track needs at least 4096 samples");
    *total_tiles = plan_tiles(n, ntracks, T, overlap_rows, tile0);
    return 0;
}

// the device track table and the pinned upload slots, allocated on the first batch call and kept until srtDestroy
static int ensure_batch(srt_engine* e)
{
    if (e->btab && e->bpin && e->bev[SRT_BATCH_SLOTS - 1]) return 0;
    SrtSetupLock setup;
    const size_t cap = (size_t)e->cfg.max_tiles;
    if (!e->btab) HIPCHK(hipMalloc((void**)&e->btab, cap * sizeof(SrtBatchTrack)));
    if (!e->bpin) HIPCHK(hipHostMalloc((void**)&e->bpin, SRT_BATCH_SLOTS * cap * sizeof(SrtBatchTrack), hipHostMallocDefault));
    for (hipEvent_t& ev : e->bev) if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return 0;
}

// the per-track remix matrices (see srt_engine::bgtab): the device table and its pinned slots, allocated once, by the first srtSeparateBatchMix with n_out > 0
static int ensure_batch_mix(srt_engine* e)
{
    if (e->bgtab && e->bgpin) return 0;
    SrtSetupLock setup;
    const size_t bytes = (size_t)e->cfg.max_tiles * SRT_BATCH_GAIN_FLOATS * sizeof(float);
    if (!e->bgtab) HIPCHK(e->bwmem.alloc(&e->bgtab, bytes));
    if (!e->bgpin) HIPCHK(e->bwmem.alloc(&e->bgpin, SRT_BATCH_SLOTS * bytes, true));
    return 0;
}

// the per-track filter's workspace (see srt_engine::bwmem): sizes follow from the configuration, so it is allocated once, by the first srtSeparateBatchWiener
static size_t batch_wiener_chunk_cap(const srt_engine* e) { return (size_t)e->cfg.max_tiles * e->cfg.T / 16 + e->cfg.max_tiles; }
static size_t batch_wiener_track_floats(const srt_engine* e) { return (size_t)SRT_WIENER_MAX_ITERS * e->cfg.n_stems * e->cfg.F; }      // R: x 4, weight sums: x 1
static int ensure_batch_wiener(srt_engine* e)
{
    if (e->bwtab && e->bwpin && e->bwslab && e->bwtabf && e->wspec) return 0;
    SrtSetupLock setup;
    const size_t cap = (size_t)e->cfg.max_tiles, S = e->cfg.n_stems, F = e->cfg.F;
    if (!e->bwtab) HIPCHK(e->bwmem.alloc(&e->bwtab, cap * sizeof(SrtBatchWiener)));
    if (!e->bwpin) HIPCHK(e->bwmem.alloc(&e->bwpin, SRT_BATCH_SLOTS * cap * sizeof(SrtBatchWiener), true));
    if (!e->bwslab) HIPCHK(e->bwmem.alloc(&e->bwslab, batch_wiener_chunk_cap(e) * (S * 4 * F + SRT_WIENER_BINBLK) * sizeof(float)));
    if (!e->bwtabf) {
        const size_t bytes = (cap * batch_wiener_track_floats(e) * 5 + cap) * sizeof(float);
        HIPCHK(e->bwmem.alloc(&e->bwtabf, bytes));
        HIPCHK(hipMemset(e->bwtabf, 0, bytes));
    }
    if (!e->wspec) HIPCHK(hipMalloc((void**)&e->wspec, S * 2 * e->rows_cap * SRT_SPEC_LD * sizeof(float2)));      // (ensure_wiener_ws's size rule: max_tiles tiles)
    return 0;
}

// the track arrays of a batch call (`who` names the entry point): what every entry point checks before it looks at options
static int batch_tracks_check(const char* who, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out)
{
    if (ntracks < 1 || !d_L || !d_R || !n || !d_out) return fail(-1, "%s: need ntracks >= 1 and the four track arrays", who);
    char what[160];
    for (int k = 0; k < ntracks; ++k) {
        if (!d_L[k] || !d_R[k] || !d_out[k]) { snprintf(what, sizeof what, "%s: null pointer in track %d", who, k); return fail(-1, "%s", what); }
        if (n[k] < SRT_FFT) { snprintf(what, sizeof what, "%s: track %d has fewer than 4096 samples", who, k); return fail(-1, "%s", what); }
    }
    return 0;
}

static const char* const BATCH_OVERLAP_RANGE = "%s: the overlap must be 0 .. T / 2 rows";
static const char* const BATCH_MIX_REFUSED = "%s: not available with the engine's stem remix on (srtSetMix): srtSeparateBatchMix takes the mix per track, or srtSetMix(e, 0, NULL) first";
static const char* const BATCH_WIENER_REFUSED = "%s: not available with the Wiener filter on (its kernels index masks by back-to-back tiles): srtSetWiener(e, 0) first";

// What the batch entry points share once their checks have passed, up to and including the forward: the plan of o.overlap against max_tiles, the track table(s)
// and their upload from a pinned slot, the batched STFT and the network over the packed tiles.  o.wiener: the filter's second table.  o.n_out > 0: the tracks'
// matrices [n_out][n_stems + 1] at h_gain + k * gain_stride (0: one for all) go up beside the track table (per track, so beside the record: o.mix stays unused).
struct BatchCall { size_t total; SrtBatchGrid g; size_t ch_stride; int wchunks; };
static int batch_forward(srt_engine* e, const char* who, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out,
                         const SepOpts& o, const float* h_gain, size_t gain_stride, BatchCall* bc)
{
    const SrtSwitches sw = srt_read_switches();
    const int T = e->cfg.T, F = e->cfg.F, S = e->cfg.n_stems, O = o.overlap, wiener = o.wiener;
    const int n_out = o.n_out, gw = n_out * (S + 1);                           // gw: floats of one track's matrix
    const size_t total = plan_tiles(n, ntracks, T, O, nullptr);
    if (total > (size_t)e->cfg.max_tiles) {
        char what[160];
        snprintf(what, sizeof what, O ? "%s: the tracks take %zu overlapped tiles, more than max_tiles (srtBatchPlanOverlap counts them; split the list into calls that fit)"
                                      : "%s: the tracks take %zu tiles, more than max_tiles (split the list into calls that fit, as stream.pack_tracks does)", who, total);
        return fail(-1, "%s", what);
    }
    if (wiener && total * T / 16 > 65535) return fail(-1, "%s: more than 65535 blocks of 16 packed rows (the filter's grid)", who);
    for (int s = 0; s < S; ++s) if (!e->have_coeff[s]) return fail(-5, "%s: weights not set for every stem", who);
    if (stream_capturing(e)) return fail(-1, "%s: not capturable (the track table is uploaded per call): call it outside stream capture", who);
    int rc = ensure_batch(e);
    if (rc) return rc;
    if (wiener && (rc = ensure_batch_wiener(e))) return rc;
    if (n_out && (rc = ensure_batch_mix(e))) return rc;
    if (wiener && o.mask_ext == SRT_MASK_EXT_AVERAGE && (rc = ensure_mask_ext_table(e, who))) return rc;      // (without the filter the table is srtSetMaskExtension's)
    // the table goes up in stream order from a pinned slot; the slot's previous copy (SRT_BATCH_SLOTS calls ago) must have left it first
    const int slot = e->bslot;
    if (e->bused[slot]) HIPCHK(hipEventSynchronize(e->bev[slot]));
    SrtBatchTrack* h = e->bpin + (size_t)slot * e->cfg.max_tiles;
    size_t tile0 = 0;
    for (int k = 0; k < ntracks; ++k) {
        SrtBatchTrack& t = h[k];
        t.L = d_L[k]; t.R = d_R[k]; t.n = n[k];
        t.frames = (int)srtStftFrames(n[k]); t.rows = (int)srtStftRows(n[k]);
        t.tile0 = (int)tile0; t.ntiles = (int)overlap_tiles((size_t)t.rows, T, O); tile0 += t.ntiles;      // (O = 0: ceil(rows / T))
        t.out = d_out[k]; t.out_len = srtIstftLength(t.rows);
    }
    // (the inverse grid has one workgroup column per output of a remix, as srt_launch_istft's ncol; the STFT grid does not depend on the count)
    if (srt_batch_geometry(h, ntracks, T, F, n_out ? n_out : S, &bc->g)) return fail(-1, "%s: batch geometry out of range", who);
    bc->wchunks = 0;
    SrtBatchWiener* hw = wiener ? e->bwpin + (size_t)slot * e->cfg.max_tiles : nullptr;
    if (wiener) {
        bc->wchunks = srt_batch_wiener_geometry(h, hw, ntracks);
        if (bc->wchunks < 1 || (size_t)bc->wchunks > batch_wiener_chunk_cap(e)) return fail(-1, "%s: batch geometry out of range", who);
    }
    HIPCHK(hipMemcpyAsync(e->btab, h, (size_t)ntracks * sizeof(SrtBatchTrack), hipMemcpyHostToDevice, e->stream));
    if (wiener) HIPCHK(hipMemcpyAsync(e->bwtab, hw, (size_t)ntracks * sizeof(SrtBatchWiener), hipMemcpyHostToDevice, e->stream));
    if (n_out) {                                               // the tracks' matrices, packed [ntracks][n_out][S + 1], from the same slot of the ring
        float* hg = e->bgpin + (size_t)slot * e->cfg.max_tiles * SRT_BATCH_GAIN_FLOATS;
        for (int k = 0; k < ntracks; ++k) memcpy(hg + (size_t)k * gw, h_gain + k * gain_stride, (size_t)gw * sizeof(float));
        HIPCHK(hipMemcpyAsync(e->bgtab, hg, (size_t)ntracks * gw * sizeof(float), hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(hipEventRecord(e->bev[slot], e->stream));
    e->bused[slot] = true; e->bslot = (slot + 1) % SRT_BATCH_SLOTS;
    bc->total = total;
    bc->ch_stride = total * T * SRT_SPEC_LD;                   // the packed spectrum: [2][total * T][SRT_SPEC_LD]
    {
        SrtStftParams p; memset(&p, 0, sizeof p);
        p.spec = e->spec; p.spec_ch_stride = bc->ch_stride; p.mag = e->mag;
        p.rows_total = (int)(total * T); p.T = T; p.F = F; p.tab = tables_of(e);
        TimerScope ts(e, "stft_batch");
        if (srt_launch_stft_batch(p, e->btab, ntracks, bc->g, e->stream, O)) return fail(-2, "batched stft launch failed");
    }
    // the network over all packed tiles; the fp16 mode's half masks under the same rule as separate_issue (never with the filter, which reads fp32 masks, nor
    // with a remix: the MIX kernels read float masks, as under srtSetMix)
    return forward_range(e, sw, e->mag, (int)total, e->masks, 0, S, masks16_wanted(e, sw, o));
}

// Every batch entry point behind its checks: the shared front, then ONE batched inverse - of the masked spectrum (the gain table of o.mask_ext first: the engine's
// srtSetMaskExtension, except in srtSeparateBatchWienerEx, which takes the rule from its arguments; o.n_out > 0: n_out pairs per track, each the chain of the track's own matrix row in the device gain table), or
// with o.wiener of the per-stem spectra the filter wrote: o.wiener x (statistics + finalize) and the filter over the packed rows with every track's own window, a
// and tables (srt_wiener.hip); with o.overlap, the average extension or o.n_out under the filter the option kernels run and the spectra are final
static int batch_separate(srt_engine* e, const char* who, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out,
                          const SepOpts& o, const float* h_gain, size_t gain_stride)
{
    DeviceScope ds(e->device);
    BatchCall bc;
    int rc = batch_forward(e, who, ntracks, d_L, d_R, n, d_out, o, h_gain, gain_stride, &bc);
    if (rc) return rc;
    const int T = e->cfg.T, F = e->cfg.F, S = e->cfg.n_stems, O = o.overlap;
    SrtIstftParams q; memset(&q, 0, sizeof q);
    q.spec_ch_stride = bc.ch_stride; q.frames = (int)(bc.total * T); q.nstems = S; q.ntiles = (int)bc.total; q.T = T; q.F = F;
    for (int s = 0; s < SRT_MAX_STEMS; ++s) q.oob[s] = e->cfg.oob_weight[s];
    q.tab = tables_of(e);
    if (o.wiener) {
        const size_t cap = (size_t)e->cfg.max_tiles, tf = batch_wiener_track_floats(e);
        SrtWienerParams w; memset(&w, 0, sizeof w);
        w.spec = e->spec; w.spec_ch_stride = bc.ch_stride; w.rows = q.frames;
        w.masks = e->masks; w.nstems = S; w.ntiles = (int)bc.total; w.T = T; w.F = F;
        w.nchunks = bc.wchunks;
        w.slab = e->bwslab; w.slab_max = e->bwslab + batch_wiener_chunk_cap(e) * S * 4 * F;
        w.rtab = e->bwtabf; w.wsum = e->bwtabf + cap * tf * 4; w.scal = w.wsum + cap * tf;
        w.out = e->wspec; w.out_stem = 2 * bc.ch_stride;
        // plain: srtSeparateBatchWiener's four launches as always.  With an option (srtSeparateBatchWienerEx) the statistics run on blended masks
        // when O > 0, and the filter writes FINAL spectra of the n_out mixes or of every stem, which the batched inverse transforms without a gain
        const bool average = o.mask_ext == SRT_MASK_EXT_AVERAGE, plain = !O && !average && !o.n_out;
        for (int pass = 1; pass <= o.wiener; ++pass) {
            { TimerScope ts(e, "wiener_stats_batch"); if (O ? srt_launch_wiener_stats_batch_ov(w, e->btab, e->bwtab, ntracks, O, pass, e->stream) : srt_launch_wiener_stats_batch(w, e->btab, e->bwtab, ntracks, pass, e->stream)) return fail(-2, "batched Wiener statistics launch failed"); }
            { TimerScope ts(e, "wiener_cov_batch"); if (srt_launch_wiener_finalize_batch(w, e->bwtab, ntracks, pass, e->stream)) return fail(-2, "batched Wiener finalize launch failed"); }
        }
        if (plain) {
            TimerScope ts(e, "wiener_filter_batch");
            if (srt_launch_wiener_filter_batch(w, e->btab, e->bwtab, ntracks, o.wiener, e->stream)) return fail(-2, "batched Wiener filter launch failed");
        } else {
            SrtBatchWienerOpt b; memset(&b, 0, sizeof b);
            b.overlap = O; b.n_out = o.n_out; b.gains = o.n_out ? e->bgtab : nullptr;
            memcpy(b.oob, e->cfg.oob_weight, sizeof b.oob);
            if (average) {      // e_j(r, c) over the packed rows from the tracks' own (blended) masks, ratio = 0: the table wiener_issue takes, per track
                if ((rc = mask_ext_issue(e, e->masks, 0, S, q.ntiles, q.frames, 0, O, O ? e->btab : nullptr, ntracks))) return rc;
                b.ext = e->ext; b.ext_stem = e->rows_cap * 2;
            }
            TimerScope ts(e, "wiener_filter_batch");
            if (srt_launch_wiener_filter_batch_opt(w, b, e->btab, e->bwtab, ntracks, o.wiener, e->stream)) return fail(-2, "batched Wiener filter launch failed");
            q.nstems = o.n_out ? o.n_out : S;                  // the spectra to invert (bc.g has as many workgroup columns)
            for (int s = 0; s < SRT_MAX_STEMS; ++s) q.oob[s] = 1.0f;
        }
        e->last.wiener_last = o.wiener; e->last.wiener_tracks = ntracks;
        q.spec = e->wspec;
        TimerScope ts(e, "istft_batch");
        return srt_launch_istft_batch_spec(q, w.out_stem, e->btab, ntracks, bc.g, e->stream) ? fail(-2, "batched istft launch failed") : 0;
    }
    q.spec = e->spec; q.masks = e->masks; q.masks16 = e->last.masks16 ? 1 : 0;
    q.ratio = e->cfg.ratio_mask ? 1 : 0;                       // normalised in the inverse kernel's prologue, as separate_issue does
    if (o.mask_ext == SRT_MASK_EXT_AVERAGE) {                  // row-local: one table over the packed rows, each track reads its own (tile0 * T onwards)
        // (with an overlap a packed row's tile and blend partner depend on the track it lies in: the batch form of the table kernel)
        if ((rc = mask_ext_issue(e, q.masks, q.masks16, S, q.ntiles, q.frames, q.ratio, O, O ? e->btab : nullptr, ntracks))) return rc;
        q.ext = e->ext; q.ext_stem = e->rows_cap * 2;
    }
    q.n_out = o.n_out;
    TimerScope ts(e, "istft_batch");
    if (o.n_out ? srt_launch_istft_batch_mix(q, e->btab, e->bgtab, ntracks, bc.g, e->stream, O) : srt_launch_istft_batch(q, e->btab, ntracks, bc.g, e->stream, O)) return fail(-2, "batched istft launch failed");
    return 0;
}

int srtSeparateBatch(srt_engine* e, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out)
{
    static const char* const who = "srtSeparateBatch";
    if (!e) return fail(-1, "srtSeparateBatch: null engine");
    if (const int rc = batch_tracks_check(who, ntracks, d_L, d_R, n, d_out)) return rc;
    const SepOpts eng = engine_opts(e);
    if (eng.overlap) return fail(-1, OVERLAP_REFUSED, who);    // srtBatchPlan has no overlap argument: srtSeparateBatchOverlap
    if (eng.n_out) return fail(-1, BATCH_MIX_REFUSED, who);
    if (eng.wiener) return fail(-1, "srtSeparateBatch: the Wiener filter's statistics would have to be per track (not supported): srtSetWiener(e, 0), or srtSeparate per track");
    SepOpts o; o.mask_ext = eng.mask_ext;
    return batch_separate(e, who, ntracks, d_L, d_R, n, d_out, o, nullptr, 0);
}

// srtSeparateBatch with overlapped tiles inside every track: overlap_rows holds for this call, the engine's own srtSetOverlap is neither read nor changed
int srtSeparateBatchOverlap(srt_engine* e, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out, int overlap_rows)
{
    static const char* const who = "srtSeparateBatchOverlap";
    if (!e) return fail(-1, "srtSeparateBatchOverlap: null engine");
    if (overlap_rows < 0) return fail(-1, "srtSeparateBatchOverlap: the overlap must be 0 .. T / 2 rows");
    if (const int rc = batch_tracks_check(who, ntracks, d_L, d_R, n, d_out)) return rc;
    if (!overlap_ok(overlap_rows, e->cfg.T)) return fail(-1, BATCH_OVERLAP_RANGE, who);
    const SepOpts eng = engine_opts(e);
    if (eng.n_out) return fail(-1, BATCH_MIX_REFUSED, who);
    if (eng.wiener) return fail(-1, BATCH_WIENER_REFUSED, who);
    SepOpts o; o.overlap = overlap_rows; o.mask_ext = eng.mask_ext;
    return batch_separate(e, who, ntracks, d_L, d_R, n, d_out, o, nullptr, 0);
}

// srtSeparateBatchOverlap with a stem remix per track: n_out outputs per track instead of n_stems, track k's matrix [n_out][n_stems + 1] at
// h_gain + k * gain_stride (0: one matrix for all).  overlap_rows, n_out and the matrices hold for this call; the engine's srtSetOverlap / srtSetMix are neither
// read nor changed.  n_out = 0: srtSeparateBatchOverlap
int srtSeparateBatchMix(srt_engine* e, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out, int overlap_rows,
                        int n_out, const float* h_gain, size_t gain_stride)
{
    static const char* const who = "srtSeparateBatchMix";
    if (!e) return fail(-1, "srtSeparateBatchMix: null engine");
    if (overlap_rows < 0) return fail(-1, "srtSeparateBatchMix: the overlap must be 0 .. T / 2 rows");
    if (n_out < 0 || n_out > SRT_MAX_STEMS) return fail(-1, "srtSeparateBatchMix: n_out must be 0 (no remix) .. SRT_MAX_STEMS");
    if (const int rc = batch_tracks_check(who, ntracks, d_L, d_R, n, d_out)) return rc;
    if (!overlap_ok(overlap_rows, e->cfg.T)) return fail(-1, BATCH_OVERLAP_RANGE, who);
    const int gw = n_out * (e->cfg.n_stems + 1);
    if (!n_out) gain_stride = 0;
    else {
        if (!h_gain) return fail(-1, "%s: null gain matrices", who);
        if (gain_stride && gain_stride < (size_t)gw) return fail(-1, "%s: gain_stride must be 0 (one matrix for every track) or at least n_out * (n_stems + 1)", who);
        for (int k = 0; k < (gain_stride ? ntracks : 1); ++k)
            if (!gain_finite(h_gain + k * gain_stride, gw)) { char what[160]; snprintf(what, sizeof what, "%s: a gain of track %d is not finite", who, k); return fail(-1, "%s", what); }
    }
    const SepOpts eng = engine_opts(e);
    if (eng.wiener) return fail(-1, BATCH_WIENER_REFUSED, who);
    SepOpts o; o.overlap = overlap_rows; o.mask_ext = eng.mask_ext; o.n_out = n_out;
    return batch_separate(e, who, ntracks, d_L, d_R, n, d_out, o, h_gain, gain_stride);
}

// srtSeparateBatch with the Wiener filter per track: fp32 masks, every other option off
int srtSeparateBatchWiener(srt_engine* e, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out, int iterations)
{
    static const char* const who = "srtSeparateBatchWiener";
    if (!e) return fail(-1, "srtSeparateBatchWiener: null engine");
    if (iterations < 1 || iterations > SRT_WIENER_MAX_ITERS) return fail(-1, "srtSeparateBatchWiener: iterations must be 1..3");
    if (e->cfg.ratio_mask) return fail(-1, "srtSeparateBatchWiener: the Wiener filter and ratio_mask exclude each other (both are the post-processing of the masks)");
    const SepOpts eng = engine_opts(e);
    if (eng.mask_ext) return fail(-1, MASK_EXT_REFUSED, who);
    if (const int rc = batch_tracks_check(who, ntracks, d_L, d_R, n, d_out)) return rc;
    if (eng.overlap) return fail(-1, OVERLAP_REFUSED, who);
    if (eng.n_out) return fail(-1, MIX_REFUSED, who);
    SepOpts o; o.wiener = iterations;
    return batch_separate(e, who, ntracks, d_L, d_R, n, d_out, o, nullptr, 0);
}

// srtSeparateBatchWiener with the options of srtSeparateWiener per call: overlapped tiles inside every track, the rule for bins >= F and a stem
// remix per track, all from the arguments - the engine's srtSetWiener / srtSetOverlap / srtSetMaskExtension / srtSetMix state is neither read nor changed
int srtSeparateBatchWienerEx(srt_engine* e, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out, const srt_batch_wiener_opts* opts)
{
    static const char* const who = "srtSeparateBatchWienerEx";
    if (!e) return fail(-1, "srtSeparateBatchWienerEx: null engine");
    if (!opts) return fail(-1, "srtSeparateBatchWienerEx: null opts");
    if (const int rc = batch_tracks_check(who, ntracks, d_L, d_R, n, d_out)) return rc;
    const int S = e->cfg.n_stems, n_out = opts->n_out, gw = n_out * (S + 1);
    if (opts->iterations < 1 || opts->iterations > SRT_WIENER_MAX_ITERS) return fail(-1, "%s: iterations must be 1..3", who);
    if (!overlap_ok(opts->overlap_rows, e->cfg.T)) return fail(-1, BATCH_OVERLAP_RANGE, who);
    if (!mask_ext_ok(opts->mask_extension)) return fail(-1, "%s: mask_extension must be SRT_MASK_EXT_CONSTANT (0) or SRT_MASK_EXT_AVERAGE (1)", who);
    if (n_out < 0 || n_out > S) return fail(-1, "%s: n_out must be 0 (every stem) .. n_stems (the filter's spectrum workspace holds n_stems spectra)", who);
    size_t gain_stride = opts->gain_stride;
    if (!n_out) gain_stride = 0;
    else {
        if (!opts->h_gain) return fail(-1, "%s: null gain matrices with n_out > 0", who);
        if (gain_stride && gain_stride < (size_t)gw) return fail(-1, "%s: gain_stride must be 0 (one matrix for every track) or at least n_out * (n_stems + 1)", who);
        for (int k = 0; k < (gain_stride ? ntracks : 1); ++k)
            if (!gain_finite(opts->h_gain + k * gain_stride, gw)) { char what[160]; snprintf(what, sizeof what, "%s: a gain of track %d is not finite", who, k); return fail(-1, "%s", what); }
    }
    if (e->cfg.ratio_mask) return fail(-1, "%s: the Wiener filter and ratio_mask exclude each other (both are the post-processing of the masks)", who);
    SepOpts o; o.wiener = opts->iterations; o.overlap = opts->overlap_rows; o.mask_ext = opts->mask_extension; o.n_out = n_out;
    return batch_separate(e, who, ntracks, d_L, d_R, n, d_out, o, n_out ? opts->h_gain : nullptr, gain_stride);
}
