// srt_batch.hip — the packed-batch entry points of the engine: the batch plans, the track tables, srtSeparateBatch / Overlap / Wiener (its private declarations: srt_engine.h).
#include "srt_engine.h"

// ---- packed batch of independent tracks (srt_dsp.hip: srt_stft_batch_kernel / srt_istft_batch_kernel)
int srtBatchPlan(const size_t* n, int ntracks, int T, size_t* tile0, size_t* total_tiles)
{
    if (!n || !total_tiles || ntracks < 1 || T < 1) return fail(-1, "srtBatchPlan: need ntracks >= 1, T >= 1, n and total_tiles");
    for (int k = 0; k < ntracks; ++k) if (n[k] < SRT_FFT) return fail(-1, "srtBatchPlan: every track needs at least 4096 samples");
    size_t t = 0;
    for (int k = 0; k < ntracks; ++k) {
        if (tile0) tile0[k] = t;
        t += (srtStftRows(n[k]) + T - 1) / T;
    }
    *total_tiles = t;
    return 0;
}

// the same with overlapped tiles inside every track (srtSeparateBatchOverlap): track k takes overlap_tiles(rows_k, T, O) packed tiles; O = 0 is srtBatchPlan
int srtBatchPlanOverlap(const size_t* n, int ntracks, int T, int overlap_rows, size_t* tile0, size_t* total_tiles)
{
    if (!n || !total_tiles || ntracks < 1 || T < 1) return fail(-1, "srtBatchPlanOverlap: need ntracks >= 1, T >= 1, n and total_tiles");
    if (overlap_rows < 0 || overlap_rows > T / 2) return fail(-1, "srtBatchPlanOverlap: the overlap must be 0 .. T / 2 rows");
    for (int k = 0; k < ntracks; ++k) if (n[k] < SRT_FFT) return fail(-1, "srtBatchPlanOverlap: every track needs at least 4096 samples");
    size_t t = 0;
    for (int k = 0; k < ntracks; ++k) {
        if (tile0) tile0[k] = t;
        t += overlap_tiles(srtStftRows(n[k]), T, overlap_rows);
    }
    *total_tiles = t;
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

// What the batch entry points share, up to and including the forward: the argument checks (`who` names the entry point; wiener = the iterations of
// srtSeparateBatchWiener, 0 for the others), the track table(s) and their upload from a pinned slot, the batched STFT and the network over the packed tiles.
// overlap: -1 for the entry points that have no overlap argument (they refuse while the engine's own setting is on); >= 0: srtSeparateBatchOverlap's argument, which
// holds for the call whatever the engine's setting says (0: the back-to-back plan and kernels)
// mx: srtSeparateBatchMix's own arguments (null for the other entry points, which refuse while the engine's srtSetMix is on); n_out = 0: no remix in this call
struct BatchCall { size_t total; SrtBatchGrid g; size_t ch_stride; int wchunks; };
struct BatchMix { int n_out; const float* h_gain; size_t stride; };
static int batch_forward(srt_engine* e, const char* who, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out,
                         int wiener, int overlap, BatchCall* bc, const BatchMix* mx = nullptr)
{
    if (ntracks < 1 || !d_L || !d_R || !n || !d_out) return fail(-1, "%s: need ntracks >= 1 and the four track arrays", who);
    const SrtSwitches sw = srt_read_switches();
    char what[160];
    for (int k = 0; k < ntracks; ++k) {
        if (!d_L[k] || !d_R[k] || !d_out[k]) { snprintf(what, sizeof what, "%s: null pointer in track %d", who, k); return fail(-1, "%s", what); }
        if (n[k] < SRT_FFT) { snprintf(what, sizeof what, "%s: track %d has fewer than 4096 samples", who, k); return fail(-1, "%s", what); }
    }
    const int T = e->cfg.T, F = e->cfg.F, S = e->cfg.n_stems;
    if (overlap < 0 && e->overlap) return fail(-1, OVERLAP_REFUSED, who);     // srtBatchPlan has no overlap argument: srtSeparateBatchOverlap
    if (overlap > T / 2) return fail(-1, "%s: the overlap must be 0 .. T / 2 rows", who);
    const int O = overlap > 0 ? overlap : 0;
    if (!mx && e->mix_out) return wiener ? fail(-1, MIX_REFUSED, who)
                                         : fail(-1, "%s: not available with the engine's stem remix on (srtSetMix): srtSeparateBatchMix takes the mix per track, or srtSetMix(e, 0, NULL) first", who);
    const int n_out = mx ? mx->n_out : 0, gw = n_out * (S + 1);                // gw: floats of one track's matrix
    if (n_out) {
        if (!mx->h_gain) return fail(-1, "%s: null gain matrices", who);
        if (mx->stride && mx->stride < (size_t)gw) return fail(-1, "%s: gain_stride must be 0 (one matrix for every track) or at least n_out * (n_stems + 1)", who);
        for (int k = 0; k < (mx->stride ? ntracks : 1); ++k)
            for (int i = 0; i < gw; ++i) if (!isfinite(mx->h_gain[k * mx->stride + i])) { snprintf(what, sizeof what, "%s: a gain of track %d is not finite", who, k); return fail(-1, "%s", what); }
    }
    if (overlap >= 0 && e->wiener) return fail(-1, "%s: not available with the Wiener filter on (its kernels index masks by back-to-back tiles): srtSetWiener(e, 0) first", who);
    if (!wiener && e->wiener) return fail(-1, "srtSeparateBatch: the Wiener filter's statistics would have to be per track (not supported): srtSetWiener(e, 0), or srtSeparate per track");
    size_t total = 0;
    if (O ? srtBatchPlanOverlap(n, ntracks, T, O, nullptr, &total) : srtBatchPlan(n, ntracks, T, nullptr, &total)) return -1;
    if (total > (size_t)e->cfg.max_tiles) {
        if (O) snprintf(what, sizeof what, "%s: the tracks take %zu overlapped tiles, more than max_tiles (srtBatchPlanOverlap counts them; split the list into calls that fit)", who, total);
        else snprintf(what, sizeof what, "%s: the tracks take %zu tiles, more than max_tiles (split the list into calls that fit, as stream.pack_tracks does)", who, total);
        return fail(-1, "%s", what);
    }
    if (wiener && total * T / 16 > 65535) return fail(-1, "%s: more than 65535 blocks of 16 packed rows (the filter's grid)", who);
    for (int s = 0; s < S; ++s) if (!e->have_coeff[s]) return fail(-5, "%s: weights not set for every stem", who);
    if (stream_capturing(e)) return fail(-1, "%s: not capturable (the track table is uploaded per call): call it outside stream capture", who);
    int rc = ensure_batch(e);
    if (rc) return rc;
    if (wiener && (rc = ensure_batch_wiener(e))) return rc;
    if (n_out && (rc = ensure_batch_mix(e))) return rc;
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
        for (int k = 0; k < ntracks; ++k) memcpy(hg + (size_t)k * gw, mx->h_gain + k * mx->stride, (size_t)gw * sizeof(float));
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
    // the network over all packed tiles; the fp16 mode's half masks under the same rule as separate_issue (never with the filter, which reads fp32 masks)
    // (nor with a remix: the MIX kernels read float masks, as under srtSetMix)
    return forward_range(e, sw, e->mag, (int)total, e->masks, 0, S, !wiener && !n_out && masks16_wanted(e, sw));
}

// srtSeparateBatch (overlap = -1) and srtSeparateBatchOverlap (overlap >= 0): the shared front, the gain table of the average mask extension, one batched inverse
// mx with n_out > 0 (srtSeparateBatchMix): the inverse writes n_out pairs per track, each the chain of the track's own matrix row (the device gain table)
static int batch_separate(srt_engine* e, const char* who, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out, int overlap,
                          const BatchMix* mx = nullptr)
{
    DeviceScope ds(e->device);
    BatchCall bc;
    int rc = batch_forward(e, who, ntracks, d_L, d_R, n, d_out, 0, overlap, &bc, mx);
    if (rc) return rc;
    const int T = e->cfg.T, F = e->cfg.F, S = e->cfg.n_stems, O = overlap > 0 ? overlap : 0;
    SrtIstftParams q; memset(&q, 0, sizeof q);
    q.spec = e->spec; q.spec_ch_stride = bc.ch_stride; q.frames = (int)(bc.total * T);
    q.masks = e->masks; q.masks16 = e->last.masks16 ? 1 : 0; q.nstems = S; q.ntiles = (int)bc.total; q.T = T; q.F = F;
    for (int s = 0; s < SRT_MAX_STEMS; ++s) q.oob[s] = e->cfg.oob_weight[s];
    q.ratio = e->cfg.ratio_mask ? 1 : 0;                       // normalised in the inverse kernel's prologue, as separate_issue does
    q.tab = tables_of(e);
    if (e->mask_ext == SRT_MASK_EXT_AVERAGE) {                 // row-local: one table over the packed rows, each track reads its own (tile0 * T onwards)
        // (with an overlap a packed row's tile and blend partner depend on the track it lies in: the batch form of the table kernel)
        if ((rc = mask_ext_issue(e, q.masks, q.masks16, S, q.ntiles, q.frames, q.ratio, O, O ? e->btab : nullptr, ntracks))) return rc;
        q.ext = e->ext; q.ext_stem = e->rows_cap * 2;
    }
    TimerScope ts(e, "istft_batch");
    if (mx && mx->n_out) {
        q.n_out = mx->n_out;
        if (srt_launch_istft_batch_mix(q, e->btab, e->bgtab, ntracks, bc.g, e->stream, O)) return fail(-2, "batched istft launch failed");
    } else if (srt_launch_istft_batch(q, e->btab, ntracks, bc.g, e->stream, O)) return fail(-2, "batched istft launch failed");
    return 0;
}

int srtSeparateBatch(srt_engine* e, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out)
{
    if (!e) return fail(-1, "srtSeparateBatch: null engine");
    return batch_separate(e, "srtSeparateBatch", ntracks, d_L, d_R, n, d_out, -1);
}

// srtSeparateBatch with overlapped tiles inside every track: overlap_rows holds for this call, the engine's own srtSetOverlap is neither read nor changed
int srtSeparateBatchOverlap(srt_engine* e, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out, int overlap_rows)
{
    if (!e) return fail(-1, "srtSeparateBatchOverlap: null engine");
    if (overlap_rows < 0) return fail(-1, "srtSeparateBatchOverlap: the overlap must be 0 .. T / 2 rows");
    return batch_separate(e, "srtSeparateBatchOverlap", ntracks, d_L, d_R, n, d_out, overlap_rows);
}

// srtSeparateBatchOverlap with a stem remix per track: n_out outputs per track instead of n_stems, track k's matrix [n_out][n_stems + 1] at
// h_gain + k * gain_stride (0: one matrix for all).  overlap_rows, n_out and the matrices hold for this call; the engine's srtSetOverlap / srtSetMix are neither
// read nor changed.  n_out = 0: srtSeparateBatchOverlap
int srtSeparateBatchMix(srt_engine* e, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out, int overlap_rows,
                        int n_out, const float* h_gain, size_t gain_stride)
{
    if (!e) return fail(-1, "srtSeparateBatchMix: null engine");
    if (overlap_rows < 0) return fail(-1, "srtSeparateBatchMix: the overlap must be 0 .. T / 2 rows");
    if (n_out < 0 || n_out > SRT_MAX_STEMS) return fail(-1, "srtSeparateBatchMix: n_out must be 0 (no remix) .. SRT_MAX_STEMS");
    const BatchMix mx = { n_out, h_gain, n_out ? gain_stride : 0 };
    return batch_separate(e, "srtSeparateBatchMix", ntracks, d_L, d_R, n, d_out, overlap_rows, &mx);
}

// srtSeparateBatch with the Wiener filter per track: the shared front (fp32 masks), `iterations` x (statistics + finalize) and the filter over the packed rows
// with every track's own window, a and tables (srt_wiener.hip), then ONE batched inverse of the per-stem filtered spectra
int srtSeparateBatchWiener(srt_engine* e, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out, int iterations)
{
    static const char* const who = "srtSeparateBatchWiener";
    if (!e) return fail(-1, "srtSeparateBatchWiener: null engine");
    DeviceScope ds(e->device);
    if (iterations < 1 || iterations > SRT_WIENER_MAX_ITERS) return fail(-1, "srtSeparateBatchWiener: iterations must be 1..3");
    if (e->cfg.ratio_mask) return fail(-1, "srtSeparateBatchWiener: the Wiener filter and ratio_mask exclude each other (both are the post-processing of the masks)");
    if (e->mask_ext) return fail(-1, MASK_EXT_REFUSED, who);
    BatchCall bc;
    const int rc = batch_forward(e, who, ntracks, d_L, d_R, n, d_out, iterations, -1, &bc);
    if (rc) return rc;
    const int T = e->cfg.T, F = e->cfg.F, S = e->cfg.n_stems;
    const size_t cap = (size_t)e->cfg.max_tiles, tf = batch_wiener_track_floats(e);
    SrtWienerParams w; memset(&w, 0, sizeof w);
    w.spec = e->spec; w.spec_ch_stride = bc.ch_stride; w.rows = (int)(bc.total * T);
    w.masks = e->masks; w.nstems = S; w.ntiles = (int)bc.total; w.T = T; w.F = F;
    w.nchunks = bc.wchunks;
    w.slab = e->bwslab; w.slab_max = e->bwslab + batch_wiener_chunk_cap(e) * S * 4 * F;
    w.rtab = e->bwtabf; w.wsum = e->bwtabf + cap * tf * 4; w.scal = w.wsum + cap * tf;
    w.out = e->wspec; w.out_stem = 2 * bc.ch_stride;
    for (int pass = 1; pass <= iterations; ++pass) {
        { TimerScope ts(e, "wiener_stats_batch"); if (srt_launch_wiener_stats_batch(w, e->btab, e->bwtab, ntracks, pass, e->stream)) return fail(-2, "batched Wiener statistics launch failed"); }
        { TimerScope ts(e, "wiener_cov_batch"); if (srt_launch_wiener_finalize_batch(w, e->bwtab, ntracks, pass, e->stream)) return fail(-2, "batched Wiener finalize launch failed"); }
    }
    { TimerScope ts(e, "wiener_filter_batch"); if (srt_launch_wiener_filter_batch(w, e->btab, e->bwtab, ntracks, iterations, e->stream)) return fail(-2, "batched Wiener filter launch failed"); }
    e->last.wiener_last = iterations; e->last.wiener_tracks = ntracks;
    SrtIstftParams q; memset(&q, 0, sizeof q);
    q.spec = e->wspec; q.spec_ch_stride = bc.ch_stride; q.frames = (int)(bc.total * T);
    q.nstems = S; q.ntiles = (int)bc.total; q.T = T; q.F = F;
    for (int s = 0; s < SRT_MAX_STEMS; ++s) q.oob[s] = e->cfg.oob_weight[s];
    q.tab = tables_of(e);
    TimerScope ts(e, "istft_batch");
    if (srt_launch_istft_batch_spec(q, w.out_stem, e->btab, ntracks, bc.g, e->stream)) return fail(-2, "batched istft launch failed");
    return 0;
}
