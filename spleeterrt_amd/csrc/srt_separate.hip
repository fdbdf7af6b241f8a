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

// the transform behind srtStftEx; of the call's options only o.overlap matters: the tile layout of the magnitudes
// tiles: the tile count when the caller's plan gives it (a piece of srtSeparateHostStreamOverlap), 0: the signal's own, overlap_tiles(rows)
static int stft_issue(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_spec, float* d_mag, const SepOpts& o, size_t tiles = 0)
{
    if (!e || !d_L || !d_R || !d_spec) return fail(-1, "srtStft: null argument");
    DeviceScope ds(e->device);
    if (rows < 1 || frames > rows) return fail(-1, "srtStft: need 1 <= frames <= rows");
    const int T = e->cfg.T, O = d_mag ? o.overlap : 0;
    const size_t ntiles = tiles ? tiles : overlap_tiles(rows, T, o.overlap);
    if (d_mag && ntiles > (size_t)e->cfg.max_tiles) return fail(-1, o.overlap ? "srtStft: more than max_tiles tiles at this overlap (srtOverlapTiles)" : "srtStft: more than max_tiles * T rows");
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

int srtStftEx(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_spec, float* d_mag) { return e ? stft_issue(e, d_L, d_R, n, frames, rows, d_spec, d_mag, engine_opts(e)) : fail(-1, "srtStft: null argument"); }

int srtStft(srt_engine* e, const float* d_L, const float* d_R, size_t n, float* d_spec, float* d_mag)
{
    if (n < SRT_FFT) return fail(-1, "srtStft: need at least 4096 samples");          // the reference underflows here (stftFix.c:378)
    return srtStftEx(e, d_L, d_R, n, srtStftFrames(n), srtStftRows(n), d_spec, d_mag);
}

// average mask extension: the gain table of the inverse transform that follows on the same stream, from the masks that transform will apply
// (rows <= rows_cap: every caller has checked its tiles against max_tiles)
// (tracks: a packed batch with overlapped tiles - rows = the packed rows, each mapped inside its own track: srt_launch_mask_ext_batch)
// (seam: a piece of srtSeparateHostStreamOverlap - the mask seam carry its first O rows blend with, as in the inverse transform)
int mask_ext_issue(srt_engine* e, const float* masks, int masks16, int nstems, int ntiles, int rows, int ratio, int O, const SrtBatchTrack* tracks, int ntracks, const float* seam)
{
    if (!e->ext || (size_t)rows > e->rows_cap || nstems != e->cfg.n_stems) return fail(-1, "mask extension: no gain table for this call (srtSetMaskExtension allocates it for n_stems x max_tiles * T rows)");
    SrtMaskExtParams m; memset(&m, 0, sizeof m);
    m.masks = masks; m.masks16 = masks16; m.nstems = nstems; m.ntiles = ntiles; m.T = e->cfg.T; m.F = e->cfg.F; m.rows = rows; m.ratio = ratio;
    m.ext = e->ext; m.ext_stem = e->rows_cap * 2;
    TimerScope ts(e, "mask_ext");
    if (tracks ? srt_launch_mask_ext_batch(m, tracks, ntracks, e->stream, O) : srt_launch_mask_ext(m, e->stream, O, seam)) return fail(-2, "mask extension launch failed (the masks must be 16-byte aligned)");
    e->last.ext_rows = rows;
    return 0;
}

// inverse transform of `nstems` stems of one spectrum under their masks (nullptr: all-ones) into [nstems][2][srtIstftLength(rows)]; oob: per stem, the weight of bins >= F
// o: the overlap of the masks' tiles, the rule for bins >= F, and with o.n_out > 0 the remix - d_out is then [n_out][2][len], output m the chain of o.mix[m] over the
// stems' gains.  The single-stem callers (CLI flows, Wiener filter) pass SepOpts{}.
// pc: the signal is a piece of a longer stream (separate_piece) - `rows` are the rows it owns, the first of pc->stft_rows spectrum rows, under pc->tiles mask tiles
// (not overlap_tiles(rows): the piece's last tile reaches into the next piece's rows), and pc->seam the carry its first O rows blend with
static int istft_launch(srt_engine* e, const float2* spec, size_t rows, const float* masks, int nstems, const float* oob, bool ratio, bool masks16, float* d_out, const SepOpts& o,
                        const HostOvPiece* pc = nullptr)
{
    DeviceScope ds(e->device);
    const int T = e->cfg.T;
    SrtIstftParams p; memset(&p, 0, sizeof p);
    p.spec = spec; p.spec_ch_stride = (pc ? pc->stft_rows : rows) * SRT_SPEC_LD;
    const int O = masks ? o.overlap : 0;
    p.frames = (int)rows; p.masks = masks; p.nstems = nstems; p.ntiles = pc ? (int)pc->tiles : (int)overlap_tiles(rows, T, O);      // (O = 0: ceil(rows / T))
    p.T = T; p.F = e->cfg.F;
    const bool ext = o.mask_ext == SRT_MASK_EXT_AVERAGE;
    for (int s = 0; s < nstems; ++s) p.oob[s] = ext ? 1.0f : oob[s];     // the mean of an all-ones mask is 1 exactly: no table without masks
    p.ratio = ratio ? 1 : 0; p.masks16 = masks16 ? 1 : 0;
    p.frames_out = nullptr; p.out = d_out; p.out_len = srtIstftLength(rows); p.tab = tables_of(e);
    if (o.n_out) { p.n_out = o.n_out; memcpy(p.mix, o.mix, sizeof p.mix); }
    if (ext && masks) {
        const int rc = mask_ext_issue(e, masks, p.masks16, nstems, p.ntiles, (int)rows, p.ratio, O, nullptr, 0, pc ? pc->seam : nullptr);
        if (rc) return rc;
        p.ext = e->ext; p.ext_stem = e->rows_cap * 2;
    }
    TimerScope ts(e, "istft");
    if (srt_launch_istft(p, e->stream, O, pc ? pc->seam : nullptr)) return fail(-2, "istft launch failed");
    return 0;
}
// ONE stem's mask (or none) into a [2][len] destination, every option off
static int istft_one(srt_engine* e, const float2* spec, size_t rows, const float* mask_stem, float oob, float* d_dst) { return istft_launch(e, spec, rows, mask_stem, 1, &oob, false, false, d_dst, SepOpts{}); }
static int istft_issue(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, float* d_out, bool ratio, bool masks16, const SepOpts& o)
{
    if (!d_spec || !d_out) return fail(-1, "srtIstft: null argument");
    if (rows < 1) return fail(-1, "srtIstft: no rows");
    if (d_masks && overlap_tiles(rows, e->cfg.T, o.overlap) > (size_t)e->cfg.max_tiles) return fail(-1, o.overlap ? "srtIstft: more than max_tiles tiles at this overlap (srtOverlapTiles)" : "srtIstft: rows exceed max_tiles * T");
    return istft_launch(e, (const float2*)d_spec, rows, d_masks, e->cfg.n_stems, e->cfg.oob_weight, ratio, masks16, d_out, o);
}
// (the public entry applies the masks as they are given: srtRatioMask is its caller's business)
int srtIstft(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, float* d_out) { return e ? istft_issue(e, d_spec, rows, d_masks, d_out, false, false, engine_opts(e)) : fail(-1, "srtIstft: null argument"); }

// ---- multichannel Wiener filter (srt_wiener.hip)
static size_t wiener_slab_floats(const srt_engine* e) { return (size_t)SRT_WIENER_MAX_CHUNKS * e->cfg.n_stems * 4 * e->cfg.F + (size_t)SRT_WIENER_MAX_CHUNKS * SRT_WIENER_BINBLK; }
static size_t wiener_tab_floats(const srt_engine* e) { return (size_t)SRT_WIENER_MAX_ITERS * e->cfg.n_stems * e->cfg.F * 5 + 4; }

// the statistics slab, the R tables and the S filtered spectra for max_tiles tiles - allocated once (srtSetWiener, or the first srtIstftWiener), never
// inside a capture, kept until srtDestroy (a captured graph holds these addresses)
int ensure_wiener_ws(srt_engine* e)
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

// the part of the launch arguments that depends on the engine and on the signal's row count alone: the row chunks of the statistics pass (at most
// SRT_WIENER_MAX_CHUNKS, of at least 16 rows) and the workspaces.  The caller adds the spectrum, the masks and their tile count.
SrtWienerParams wiener_geometry(const srt_engine* e, size_t rows)
{
    const int S = e->cfg.n_stems, F = e->cfg.F;
    SrtWienerParams w; memset(&w, 0, sizeof w);
    w.rows = (int)rows; w.nstems = S; w.T = e->cfg.T; w.F = F;
    int nch = (int)((rows + 15) / 16); if (nch > SRT_WIENER_MAX_CHUNKS) nch = SRT_WIENER_MAX_CHUNKS;
    w.rpc = (int)((rows + nch - 1) / nch); w.nchunks = (int)((rows + w.rpc - 1) / w.rpc);
    w.slab = e->wslab; w.slab_max = e->wslab + (size_t)SRT_WIENER_MAX_CHUNKS * S * 4 * F;
    w.rtab = e->wtab; w.wsum = e->wtab + (size_t)SRT_WIENER_MAX_ITERS * S * F * 4; w.scal = w.wsum + (size_t)SRT_WIENER_MAX_ITERS * S * F;
    w.out = e->wspec; w.out_stem = 2 * rows * SRT_SPEC_LD;
    return w;
}

// the filter over w's rows (its spectrum, masks and tile count; the R tables and a are final) into the engine's spectrum workspace, then one inverse transform per
// output: the second half of wiener_issue, and what srtSeparateHostWiener / srtSeparateHostWienerOverlap run per piece
// seam (a later piece under an overlap): w.rows are the rows the piece owns and `seam` the mask carry its first O rows blend with - in the gain table and in the filter
static int wiener_render(srt_engine* e, const SrtWienerParams& w, float* d_out, const SepOpts& o, const float* seam = nullptr)
{
    const int S = e->cfg.n_stems, O = o.overlap, iters = o.wiener;
    const size_t rows = (size_t)w.rows;
    const bool ext = o.mask_ext == SRT_MASK_EXT_AVERAGE, plain = !O && !ext && !o.n_out;
    SrtWienerOpt q; memset(&q, 0, sizeof q);
    q.overlap = O; q.n_out = o.n_out;
    memcpy(q.oob, e->cfg.oob_weight, sizeof q.oob);
    memcpy(q.mix, o.mix, sizeof q.mix);
    if (ext) {      // e_j(r, c): the table the inverse transform's own kernel writes from the same (blended) masks, ratio = 0
        const int rc = mask_ext_issue(e, w.masks, 0, S, w.ntiles, (int)rows, 0, O, nullptr, 0, seam);
        if (rc) return rc;
        q.ext = e->ext; q.ext_stem = e->rows_cap * 2;
    }
    { TimerScope ts(e, "wiener_filter"); if (plain ? srt_launch_wiener_filter(w, iters, e->stream) : srt_launch_wiener_filter_opt(w, q, iters, e->stream, seam)) return fail(-2, "Wiener filter launch failed"); }
    e->last.wiener_last = iters; e->last.wiener_tracks = 0;
    const size_t len = srtIstftLength(rows);
    for (int m = 0; m < (o.n_out ? o.n_out : S); ++m) {      // plain: stem m under its oob_weight; with an option the spectra are final: no gain in the inverse
        const int rc = istft_one(e, e->wspec + (size_t)m * w.out_stem, rows, nullptr, plain ? e->cfg.oob_weight[m] : 1.0f, d_out + (size_t)m * 2 * len);
        if (rc) return rc;
    }
    return 0;
}

// statistics passes (one stats + one finalize launch per iteration), the filter, then one inverse transform per stem on its filtered spectrum
// (no masks: all-ones in band; bins >= F get oob_weight as with masks).  The statistics window is exactly the `rows` rows of this call.
// o: o.wiener iterations under the call's other options (off on the engine's own path, whose setters keep them apart from the filter).  With every
// option off the filter writes per-stem spectra and the inverse applies oob_weight; with an overlap the statistics run on blended masks
// (srt_wiener_stats_ov_kernel), and with any option the filter writes final spectra (srt_wiener_filter_opt_kernel) of the n_out mixes or of every stem, which the
// inverse transforms without a gain.  d_masks: [S][overlap_tiles(rows, T, overlap)][2][T][F].
static int wiener_issue(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, float* d_out, const SepOpts& o)
{
    const int O = o.overlap, iters = o.wiener;
    SrtWienerParams w = wiener_geometry(e, rows);
    w.spec = (const float2*)d_spec; w.spec_ch_stride = rows * SRT_SPEC_LD;
    w.masks = d_masks; w.ntiles = (int)overlap_tiles(rows, e->cfg.T, O);
    for (int pass = 1; pass <= iters; ++pass) {
        { TimerScope ts(e, "wiener_stats"); if (O ? srt_launch_wiener_stats_ov(w, O, pass, e->stream) : srt_launch_wiener_stats(w, pass, e->stream)) return fail(-2, "Wiener statistics launch failed"); }
        { TimerScope ts(e, "wiener_cov"); if (srt_launch_wiener_finalize(w, pass, e->stream)) return fail(-2, "Wiener finalize launch failed"); }
    }
    return wiener_render(e, w, d_out, o);
}

// the checks srtIstftWienerEx and srtSeparateWiener share (`who` names the caller): 0 with the call's record in *c, or -1 with the error text set; no device work
// any_rows (srtSeparateHostWiener, which holds one piece of max_tiles tiles at a time): no limit on the signal's tiles
static int wiener_opts_check(const srt_engine* e, const char* who, const srt_wiener_opts* o, size_t rows, SepOpts* c, bool any_rows = false)
{
    const int T = e->cfg.T, S = e->cfg.n_stems;
    if (o->iterations < 1 || o->iterations > SRT_WIENER_MAX_ITERS) return fail(-1, "%s: iterations must be 1..3", who);
    if (!overlap_ok(o->overlap_rows, T)) return fail(-1, "%s: overlap_rows must be 0 .. T / 2", who);
    if (!mask_ext_ok(o->mask_extension)) return fail(-1, "%s: mask_extension must be SRT_MASK_EXT_CONSTANT (0) or SRT_MASK_EXT_AVERAGE (1)", who);
    if (o->n_out < 0 || o->n_out > S) return fail(-1, "%s: n_out must be 0 (every stem) .. n_stems (the filter's spectrum workspace holds n_stems spectra; more outputs are a follow-up)", who);
    if (o->n_out && !o->h_gain) return fail(-1, "%s: null gain matrix with n_out > 0", who);
    if (!gain_finite(o->h_gain, o->n_out * (S + 1))) return fail(-1, "%s: every gain must be finite", who);
    if (e->cfg.ratio_mask) return fail(-1, "%s: the Wiener filter and ratio_mask exclude each other (both are the post-processing of the masks)", who);
    if (rows < 1 || (!any_rows && overlap_tiles(rows, T, o->overlap_rows) > (size_t)e->cfg.max_tiles))
        return fail(-1, o->overlap_rows ? "%s: the signal takes more than max_tiles tiles at this overlap (srtOverlapTiles)" : "%s: need 1 <= rows <= max_tiles * T", who);
    *c = SepOpts{};
    c->wiener = o->iterations; c->overlap = o->overlap_rows; c->mask_ext = o->mask_extension; c->n_out = o->n_out;
    for (int m = 0; m < o->n_out; ++m) for (int s = 0; s <= S; ++s) c->mix[m][s] = o->h_gain[m * (S + 1) + s];
    return 0;
}

// the workspaces of an option call: the filter's, and with the average extension the engine's gain table (srtSetMaskExtension's, same size, kept until srtDestroy)
// (the gain table's piece on its own: srtSeparateBatchWienerEx has workspaces of its own but shares the table)
// Calls on one engine are single-threaded by contract (the first test of e->ext is outside the lock, as everywhere); the table is tested again under the lock so that
// a caller who breaks that rule cannot allocate it twice.  From batch_forward the capture branch is never taken: a batch call has refused a capture before it gets here.
int ensure_mask_ext_table(srt_engine* e, const char* who)
{
    if (e->ext) return 0;
    if (stream_capturing(e)) return fail(-1, "%s: the mask extension's gain table is not allocated yet (srtSetMaskExtension, or one call outside the capture)", who);
    SrtSetupLock setup;
    if (!e->ext) HIPCHK(hipMalloc((void**)&e->ext, (size_t)e->cfg.n_stems * e->rows_cap * 2 * sizeof(float)));
    return 0;
}
static int ensure_wiener_opts_ws(srt_engine* e, const char* who, const SepOpts& c)
{
    const int rc = ensure_wiener_ws(e);
    if (rc) return rc;
    return c.mask_ext ? ensure_mask_ext_table(e, who) : 0;
}

int srtIstftWienerEx(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, const srt_wiener_opts* opts, float* d_out)
{
    if (!e || !d_spec || !d_masks || !opts || !d_out) return fail(-1, "srtIstftWienerEx: null argument");
    DeviceScope ds(e->device);
    SepOpts o;
    int rc = wiener_opts_check(e, "srtIstftWienerEx", opts, rows, &o);
    if (rc) return rc;
    if ((rc = ensure_wiener_opts_ws(e, "srtIstftWienerEx", o))) return rc;
    return wiener_issue(e, d_spec, rows, d_masks, d_out, o);
}

int srtIstftWiener(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, int iterations, float* d_out)
{
    if (!e || !d_spec || !d_masks || !d_out) return fail(-1, "srtIstftWiener: null argument");
    DeviceScope ds(e->device);
    if (iterations < 1 || iterations > SRT_WIENER_MAX_ITERS) return fail(-1, "srtIstftWiener: iterations must be 1..3");
    SepOpts o = engine_opts(e);
    if (o.n_out) return fail(-1, MIX_REFUSED, "srtIstftWiener");
    if (o.overlap) return fail(-1, OVERLAP_REFUSED, "srtIstftWiener");      // its kernels index masks by (row / T, row % T)
    if (o.mask_ext) return fail(-1, MASK_EXT_REFUSED, "srtIstftWiener");    // the filter's own gains above F would have to be defined first
    if (rows < 1 || (rows + e->cfg.T - 1) / e->cfg.T > (size_t)e->cfg.max_tiles) return fail(-1, "srtIstftWiener: need 1 <= rows <= max_tiles * T");
    const int rc = ensure_wiener_ws(e);
    if (rc) return rc;
    o.wiener = iterations;                                                  // whatever srtSetWiener says
    return wiener_issue(e, d_spec, rows, d_masks, d_out, o);
}

// ---- srtSeparateHostWiener's stages: srt_host.hip walks the stream piece by piece and owns the copies, the store and the events; what a piece
// computes is issued here, beside the single-signal path it has to equal.  A piece is rows [row0, row0 + rows) of the signal, its spectrum and masks in the store.
// srtSeparateHostWienerOverlap (ov = true) runs the same stages on the pieces of srtHostOverlapPieces: `rows` are then the rows a piece owns, the first
// of the stft_rows its tiles cover, and its first O rows blend with the carry of the piece before it.
int host_wiener_check(const srt_engine* e, const srt_wiener_opts* opts, size_t n, SepOpts* o, bool ov)
{
    const char* const who = ov ? "srtSeparateHostWienerOverlap" : "srtSeparateHostWiener";
    if (!ov && opts->overlap_rows > 0) return fail(-1, "%s: overlap_rows must be 0: srtSeparateHostWienerOverlap takes an overlap for a stream of any length", who);
    if (n < SRT_FFT) return fail(-1, "%s: need at least 4096 samples", who);
    const size_t rows = srtStftRows(n);
    if (rows > (size_t)0x7fffffff - 4) return fail(-1, "%s: more than 2^31 rows", who);
    int rc = wiener_opts_check(e, who, opts, rows, o, true);
    if (rc) return rc;
    for (int s = 0; s < e->cfg.n_stems; ++s) if (!e->have_coeff[s]) return fail(-5, "%s: weights not set for every stem", who);
    return 0;
}

int host_wiener_ws(srt_engine* e, const SepOpts& o, const char* who) { return ensure_wiener_opts_ws(e, who, o); }

// sweep A: the piece's PCM -> its spectrum and fp32 masks in the store (not the engine's own mask buffer, so the fp16 mode keeps floats as everywhere the filter runs)
// O > 0: the transform covers the piece's stft_rows rows in the overlapped layout of its own tiles, and unless the piece is the stream's last, rows [S, T) of its last
// tile go into its carry slot for the next piece (pc.seam_out)
int host_wiener_analyse(srt_engine* e, const SrtSwitches& sw, const float* d_L, const float* d_R, size_t n, size_t frames, const HostWienerPiece& pc, int O)
{
    SepOpts so{}; so.overlap = O;
    int rc = stft_issue(e, d_L, d_R, n, frames, pc.stft_rows, (float*)pc.spec, e->mag, so, O ? (size_t)pc.ntiles : 0);
    if (rc) return rc;
    if ((rc = forward_range(e, sw, e->mag, pc.ntiles, pc.masks, 0, e->cfg.n_stems)) || !pc.seam_out) return rc;
    TimerScope ts(e, "mask_seam");
    return srt_launch_mask_seam_save(pc.masks, e->cfg.n_stems, pc.ntiles, e->cfg.T, e->cfg.F, O, pc.seam_out, e->stream) ? fail(-2, "mask seam save launch failed") : 0;
}

// w: wiener_geometry of the whole signal; the piece goes into a copy of it
static SrtWienerParams piece_params(const SrtWienerParams& w, const HostWienerPiece& pc)
{
    SrtWienerParams p = w;
    p.spec = pc.spec; p.spec_ch_stride = pc.stft_rows * SRT_SPEC_LD; p.masks = pc.masks; p.ntiles = pc.ntiles;
    return p;
}

// the piece's share of statistics pass `pass` (chunks that straddle a piece boundary continue in the slab: srt_wiener_stats_seg_kernel)
// (O > 0: on the blended masks of the piece's overlapped tiles, srt_wiener_stats_seg_ov_kernel)
int host_wiener_stats(srt_engine* e, const SrtWienerParams& w, const HostWienerPiece& pc, int pass, int O)
{
    TimerScope ts(e, "wiener_stats");
    const SrtWienerParams p = piece_params(w, pc);
    return (O ? srt_launch_wiener_stats_seg_ov(p, O, pc.seam, pc.row0, pc.rows, pass, e->stream) : srt_launch_wiener_stats_seg(p, pc.row0, pc.rows, pass, e->stream))
               ? fail(-2, "Wiener statistics launch failed") : 0;
}

int host_wiener_finalize(srt_engine* e, const SrtWienerParams& w, int pass)
{
    TimerScope ts(e, "wiener_cov");
    return srt_launch_wiener_finalize(w, pass, e->stream) ? fail(-2, "Wiener finalize launch failed") : 0;
}

// sweep B: the filter is row-local once the tables exist, so the piece is rendered as a signal of its own rows: wiener_issue's second half
int host_wiener_render(srt_engine* e, const SrtWienerParams& w, const SepOpts& o, const HostWienerPiece& pc, float* d_out)
{
    SrtWienerParams p = piece_params(w, pc);
    p.rows = (int)pc.rows; p.out_stem = 2 * pc.rows * SRT_SPEC_LD;
    return wiener_render(e, p, d_out, o, pc.seam);
}

// fp16 mode: the masks between the head and the inverse transform - the engine's own buffer, never seen by a caller - are halves where both kernels take them
// (srt_head_rows_kernel<.., true> / srt_istft_ola3_kernel<.., true>: F <= 1024, no ratio mask, no Wiener filter (fp32 masks), head launches of >= 1024
// workgroups: srt_head_out16_ok; sw.m16 = 0: floats, for A/B runs)
// (nor with the stem remix: there is no half-mask MIX kernel)
bool masks16_wanted(const srt_engine* e, const SrtSwitches& sw, const SepOpts& o) { return e->cfg.precision == SRT_PREC_F16 && e->act16 && !e->cfg.ratio_mask && !o.wiener && !o.n_out && e->cfg.F <= 1024 && sw.m16; }

// the three stages of one separation under the call's record: the STFT, the forward over the tiles of o.overlap, then the filter (o.wiener) or the masked inverse
static int separate_issue(srt_engine* e, const SrtSwitches& sw, const SepOpts& o, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_out)
{
    const size_t ntiles = overlap_tiles(rows, e->cfg.T, o.overlap);
    int rc = stft_issue(e, d_L, d_R, n, frames, rows, (float*)e->spec, e->mag, o);
    if (rc) return rc;
    rc = forward_range(e, sw, e->mag, (int)ntiles, e->masks, 0, e->cfg.n_stems, masks16_wanted(e, sw, o));
    if (rc) return rc;
    if (o.wiener) return wiener_issue(e, (const float*)e->spec, rows, e->masks, d_out, o);
    // ratio_mask: normalised across the stems inside the inverse kernel's prologue (srt_ratio_of, srt_dsp.hip) - e->masks keeps the raw sigmoid masks
    return istft_issue(e, (const float*)e->spec, rows, e->masks, d_out, e->cfg.ratio_mask != 0, e->last.masks16, o);
}

// One piece of srtSeparateHostStreamOverlap (srt_host.hip walks the plan and owns the copies): separate_issue's stages on the piece's geometry.
// The STFT runs over pc.stft_rows rows into pc.tiles overlapped tiles, the forward over those tiles (float masks in every mode: the carry holds floats), the
// inverse over the pc.own_rows rows the piece owns with pc.seam for its first O rows; then, unless the piece is the stream's last, rows [S, T) of its last tile
// go into d_seam for the next piece (the stream is in order: the inverse has read the old carry by then).  o.overlap > 0, o.wiener = 0.
int separate_piece(srt_engine* e, const SrtSwitches& sw, const SepOpts& o, const float* d_L, const float* d_R, size_t n, size_t frames, const HostOvPiece& pc, float* d_seam, float* d_out)
{
    int rc = stft_issue(e, d_L, d_R, n, frames, pc.stft_rows, (float*)e->spec, e->mag, o, pc.tiles);
    if (rc) return rc;
    if ((rc = forward_range(e, sw, e->mag, (int)pc.tiles, e->masks, 0, e->cfg.n_stems))) return rc;
    if ((rc = istft_launch(e, e->spec, pc.own_rows, e->masks, e->cfg.n_stems, e->cfg.oob_weight, e->cfg.ratio_mask != 0, false, d_out, o, &pc))) return rc;
    if (!d_seam) return 0;
    TimerScope ts(e, "mask_seam");
    return srt_launch_mask_seam_save(e->masks, e->cfg.n_stems, (int)pc.tiles, e->cfg.T, e->cfg.F, o.overlap, d_seam, e->stream) ? fail(-2, "mask seam save launch failed") : 0;
}

// srtSeparate with the call's own options (fp32 masks in the fp16 mode too, as with srtSetWiener).  Always eager: the graph cache has no key for an option call.
int srtSeparateWiener(srt_engine* e, const float* d_L, const float* d_R, size_t n, const srt_wiener_opts* opts, float* d_out)
{
    if (!e || !d_L || !d_R || !opts || !d_out) return fail(-1, "srtSeparateWiener: null argument");
    if (n < SRT_FFT) return fail(-1, "srtSeparateWiener: need at least 4096 samples");
    DeviceScope ds(e->device);
    const size_t rows = srtStftRows(n);
    SepOpts o;
    int rc = wiener_opts_check(e, "srtSeparateWiener", opts, rows, &o);
    if (rc) return rc;
    for (int s = 0; s < e->cfg.n_stems; ++s) if (!e->have_coeff[s]) return fail(-5, "srtSeparateWiener: weights not set for every stem");
    if ((rc = ensure_wiener_opts_ws(e, "srtSeparateWiener", o))) return rc;
    return separate_issue(e, srt_read_switches(), o, d_L, d_R, n, srtStftFrames(n), rows, d_out);
}

// srtSeparateEx under the engine's record, already resolved (host_stream resolves once for all its chunks): its checks, then the stages, eager or through the graph cache
int separate_run(srt_engine* e, const SepOpts& o, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_out)
{
    const size_t ntiles = overlap_tiles(rows, e->cfg.T, o.overlap);
    if (rows < 1 || ntiles > (size_t)e->cfg.max_tiles) return fail(-1, o.overlap ? "srtSeparate: the signal takes more than max_tiles tiles at this overlap (srtOverlapTiles)" : "srtSeparate: signal longer than max_tiles * T frames");
    if (o.overlap && o.wiener) return fail(-1, OVERLAP_REFUSED, "srtSeparate with the Wiener filter on");
    const SrtSwitches sw = srt_read_switches();
    if (!e->graph_mode) return separate_issue(e, sw, o, d_L, d_R, n, frames, rows, d_out);
    DeviceScope ds(e->device);
    GraphKey k;
    const bool valid = graph_prepare(e, d_L && d_R && d_out && frames <= rows, ntiles, 2, sw, &k);
    k.p0 = d_L; k.p1 = d_R; k.p2 = d_out; k.n = n; k.frames = frames; k.rows = rows;
    graph_key_opts(&k, o);
    return run_graphed(e, k, valid, [&]() { return separate_issue(e, sw, o, d_L, d_R, n, frames, rows, d_out); });
}

int srtSeparateEx(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_out) { return e ? separate_run(e, engine_opts(e), d_L, d_R, n, frames, rows, d_out) : fail(-1, "srtSeparate: null engine"); }

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
    int rc = stft_issue(e, d_L, d_R, n, frames, rows, (float*)e->spec, e->mag, SepOpts{});      // (every option off: cli_check has refused the engine's)
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
    const SepOpts o = engine_opts(e);
    if (o.overlap) return fail(-1, OVERLAP_REFUSED, "srtSeparateCli");        // the residual chain reads masks and writes the second network's magnitudes by tile
    if (o.n_out) return fail(-1, MIX_REFUSED, "srtSeparateCli");              // the flows have no stem axis to mix over
    if (o.mask_ext) return fail(-1, MASK_EXT_REFUSED, "srtSeparateCli");      // the complex-domain residual chain subtracts oob * spec (srt_residual_kernel)
    if (o.wiener) return fail(-1, "srtSeparateCli: the Wiener filter does not apply to the CLI flows (the sub-networks see different inputs, and its statistics span the whole signal)");
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
