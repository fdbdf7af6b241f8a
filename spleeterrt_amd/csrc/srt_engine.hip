// srt_engine.hip — engine object, HBM layout and the device-resident C ABI (include/spleeterrt_amd.h).
//
// HBM layout (all fp32, instance = (stem, tile), CHW planar, row = time, contiguous = frequency):
//   coeff[stem]           raw spleeterCoeff blob (Executable/spleeter.h:5-31), biases / BN read in place
//   wpack[stem][layer]    GEMM-ready weights [Cin][25][CP]
//   raw[i]  i=0..5        encoder conv+bias outputs   [stem][tile][Cout][H>>i+1][W>>i+1]: the skip tensors AND the next encoder
//                         layer's input (its BN + activation is applied by the consumer while staging; nothing is stored twice)
//   up[i]   i=0..5        decoder outputs (new channels only; the concat is done by pointer)
//   spec / mag / masks / frames / pcm for the DSP stages
//
// This unit: error text, set-up lock and kernel note, the option setters, create / destroy, coefficients, the graph cache's preamble and the network forward.
// The other entry points are in srt_separate.hip, srt_host.hip, srt_batch.hip and srt_taps.hip; what the five units share is declared in srt_engine.h.
#include "srt_engine.h"
#include <mutex>

static std::recursive_mutex g_setup_mutex;
SrtSetupLock::SrtSetupLock() { g_setup_mutex.lock(); }
SrtSetupLock::~SrtSetupLock() { g_setup_mutex.unlock(); }

static thread_local char g_err[512] = "";
static thread_local hipError_t g_hip_noted = hipSuccess;               // HIP error behind the last failed launch (srt_launch_status)
void srt_note_hip_error(hipError_t e) { g_hip_noted = e; }
int srt_set_error(int code, const char* fmt, const char* detail)      // shared with the drop-in layers (srt_compat.hip, srt_stream.hip)
{
    const int n = snprintf(g_err, sizeof g_err, fmt, detail);
    if (g_hip_noted != hipSuccess && n > 0 && (size_t)n < sizeof g_err - 8)
        snprintf(g_err + n, sizeof g_err - n, " [HIP: %s]", hipGetErrorString(g_hip_noted));
    g_hip_noted = hipSuccess;
    return code;
}

// first kernel the calling thread launched since the last reset (SRT_LAUNCH, srt_internal.h)
static thread_local const void* g_kfn = nullptr;
static thread_local const char* g_ktext = nullptr;
void srt_kernel_note(const void* fn, const char* text) { if (!g_kfn) { g_kfn = fn; g_ktext = text; } }
void srt_kernel_note_reset() { g_kfn = nullptr; g_ktext = nullptr; }

TimerScope::TimerScope(srt_engine* e_, const char* name) : e(e_), idx(0), on(e_->timing && e_->tlog.size() < SRT_TIMING_MAX) {
    if (!on) return;
    TimingEntry t; t.name = name; t.kfn = nullptr; t.ktext = nullptr;
    srt_kernel_note_reset();
    if (hipEventCreate(&t.a) != hipSuccess) { on = false; return; }
    if (hipEventCreate(&t.b) != hipSuccess) { hipEventDestroy(t.a); on = false; return; }
    hipEventRecord(t.a, e->stream);
    e->tlog.push_back(t); idx = e->tlog.size() - 1;
}
TimerScope::~TimerScope() { if (on) { hipEventRecord(e->tlog[idx].b, e->stream); e->tlog[idx].kfn = g_kfn; e->tlog[idx].ktext = g_ktext; } }

static Layout make_layout()
{
    Layout lo; size_t o = 0;
    for (int i = 0; i < 6; ++i) {
        LayerOff& L = lo.down[i]; L.cin = ENC_CH[i][0]; L.cout = ENC_CH[i][1]; L.cp = (L.cout + 31) / 32 * 32;
        L.w = o; o += (size_t)25 * L.cin * L.cout; L.b = o; o += L.cout; L.bn = o; if (i < 5) o += 2 * (size_t)L.cout;
    }
    for (int i = 0; i < 6; ++i) {
        LayerOff& L = lo.up[i]; L.cin = DEC_CH[i][0]; L.cout = DEC_CH[i][1]; L.cp = (L.cout + 31) / 32 * 32;
        L.w = o; o += (size_t)25 * L.cin * L.cout; L.b = o; o += L.cout; L.bn = o; o += 2 * (size_t)L.cout;
    }
    lo.head_w = o; o += 32; lo.head_b = o; o += 2; lo.total = o;
    return lo;
}

const char* srtLastError(void) { return g_err; }
size_t srtCoeffBytes(void) { return (size_t)SRT_COEFF_FLOATS * 4; }
size_t srtStftRows(size_t n) { return (n + SRT_HOP - 1) / SRT_HOP; }
size_t srtStftFrames(size_t n) { return n < SRT_FFT ? 0 : (n - SRT_FFT + SRT_HOP / 4) / SRT_HOP + 1; }   // stftFix.c:378 + tail frame
size_t srtIstftLength(size_t rows) { return rows * SRT_HOP + (SRT_FFT - SRT_HOP); }

size_t srtOverlapTiles(size_t rows, int T, int overlap_rows)
{
    if (T < 1 || !overlap_ok(overlap_rows, T)) { fail(-1, "srtOverlapTiles: need T >= 1 and 0 <= overlap <= T / 2"); return 0; }
    return overlap_tiles(rows, T, overlap_rows);
}

int srtSetOverlap(srt_engine* e, int overlap_rows)
{
    if (!e) return fail(-1, "srtSetOverlap: null engine");
    if (!overlap_ok(overlap_rows, e->cfg.T)) return fail(-1, "srtSetOverlap: the overlap must be 0 (off) .. T / 2 rows");
    e->overlap = overlap_rows;
    return 0;
}
int srt_engine_overlap(const srt_engine* e) { return e->overlap; }

int srtSetMix(srt_engine* e, int n_out, const float* h_gain)
{
    if (!e) return fail(-1, "srtSetMix: null engine");
    if (n_out < 0 || n_out > SRT_MAX_STEMS) return fail(-1, "srtSetMix: n_out must be 0 (off) .. SRT_MAX_STEMS");
    if (n_out && !h_gain) return fail(-1, "srtSetMix: null gain matrix");
    const int S = e->cfg.n_stems;
    if (!gain_finite(h_gain, n_out * (S + 1))) return fail(-1, "srtSetMix: every gain must be finite");
    if (n_out && e->wiener) return fail(-1, "srtSetMix: the stem remix is not available with the Wiener filter on (the mix of filtered spectra is a follow-up, DESIGN.md 16): srtSetWiener(e, 0) first");
    memset(e->mix, 0, sizeof e->mix);
    for (int m = 0; m < n_out; ++m) for (int s = 0; s <= S; ++s) e->mix[m][s] = h_gain[m * (S + 1) + s];
    e->mix_out = n_out;
    if (n_out) { if (!++e->mix_gen) ++e->mix_gen; }
    return 0;
}
int srtMixOutputs(const srt_engine* e) { return e ? e->mix_out : 0; }
int srt_engine_mix(const srt_engine* e) { return e->mix_out; }

int srtSetMaskExtension(srt_engine* e, int mode)
{
    if (!e) return fail(-1, "srtSetMaskExtension: null engine");
    if (!mask_ext_ok(mode)) return fail(-1, "srtSetMaskExtension: the mode must be SRT_MASK_EXT_CONSTANT (0) or SRT_MASK_EXT_AVERAGE (1)");
    if (mode && e->wiener) return fail(-1, "srtSetMaskExtension: not available with the Wiener filter on (its gains above F are a follow-up, DESIGN.md 15): srtSetWiener(e, 0) first");
    DeviceScope ds(e->device);
    if (mode && !e->ext) {                               // the gain table, once: never inside a capture, kept until srtDestroy (a captured graph holds its address)
        if (stream_capturing(e)) return fail(-1, "srtSetMaskExtension: the gain table is not allocated yet (switch the mode on before capturing)");
        SrtSetupLock setup;
        HIPCHK(hipMalloc((void**)&e->ext, (size_t)e->cfg.n_stems * e->rows_cap * 2 * sizeof(float)));
    }
    e->mask_ext = mode;
    return 0;
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

int srtSetDitherSeed(srt_engine* e, uint64_t seed)
{
    if (!e) return fail(-1, "srtSetDitherSeed: null engine");
    e->dither_seed = seed;
    return 0;
}

// The engine's own options as a call's record: with the setters and accessors above, the only reader of these fields.  (The setters keep the filter apart from
// the extension and the mix, so a record with wiener > 0 has both off.)
SepOpts engine_opts(const srt_engine* e)
{
    SepOpts o;
    o.overlap = e->overlap; o.mask_ext = e->mask_ext; o.wiener = e->wiener; o.n_out = e->mix_out; o.mix_gen = e->mix_gen;
    o.dither_seed = e->dither_seed;
    memcpy(o.mix, e->mix, sizeof o.mix);
    return o;
}

// the option fields of a graph key (GraphKey, srt_engine.h): a sequence captured under one record is never replayed under another; the generation counts only while the mix is on
void graph_key_opts(GraphKey* k, const SepOpts& o) { k->wiener = o.wiener; k->overlap = o.overlap; k->mask_ext = o.mask_ext; k->mix_gen = o.n_out ? o.mix_gen : 0; }

static void free_staging(srt_engine* e)
{
    HostStaging& h = e->hs;
    for (int b = 0; b < 2; ++b) {
        if (h.d_in[b]) hipFree(h.d_in[b]);
        if (h.d_out[b]) hipFree(h.d_out[b]);
        if (h.d_inq[b]) hipFree(h.d_inq[b]);
        if (h.d_outq[b]) hipFree(h.d_outq[b]);
        if (h.d_rin[b]) hipFree(h.d_rin[b]);
        if (h.d_rout[b]) hipFree(h.d_rout[b]);
        if (h.ev_in[b]) hipEventDestroy(h.ev_in[b]);
        if (h.ev_cmp[b]) hipEventDestroy(h.ev_cmp[b]);
        if (h.ev_out[b]) hipEventDestroy(h.ev_out[b]);
    }
    if (h.d_carry) hipFree(h.d_carry);
    if (h.d_clip) hipFree(h.d_clip);
    if (h.d_wstore) hipFree(h.d_wstore);
    if (h.d_mseam) hipFree(h.d_mseam);
    if (h.d_rcarry) hipFree(h.d_rcarry);
    if (h.s_in) hipStreamDestroy(h.s_in);
    if (h.s_out) hipStreamDestroy(h.s_out);
    memset(&h, 0, sizeof h);
}

static void free_graphs(srt_engine* e)
{
    for (GraphSlot& g : e->gslots) {
        if (g.exec) hipGraphExecDestroy(g.exec);
        if (g.graph) hipGraphDestroy(g.graph);
        memset(&g, 0, sizeof g);
    }
}

static void free_all(srt_engine* e)
{
    free_graphs(e);
    free_staging(e);
    for (int i = 0; i < 6; ++i) {
        void* layer[] = { e->wpack16_down[i], e->wpack16_up[i], e->wino_u[i], e->wino_e[i], e->act32[i], e->wpack_down[i], e->wpack_up[i], e->raw[i], e->up[i], i < 5 ? e->act16buf[i] : nullptr };
        for (void* m : layer) if (m) hipFree(m);
    }
    void* misc[] = { e->coeff_all, e->ws, e->wpack2_d1, e->wpack2_u5, e->wpack16cs_u5, e->preWin, e->postWin, e->twiddle, e->spec, e->spec2, e->mag, e->masks, e->wslab, e->wtab, e->wspec, e->btab, e->ext };
    for (void* m : misc) if (m) hipFree(m);
    if (e->bpin) hipHostFree(e->bpin);
    for (hipEvent_t ev : e->bev) if (ev) hipEventDestroy(ev);
    for (auto& t : e->tlog) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
    for (auto& rf : e->rate_filters) srt_rs_filter_free(&rf.f);
    e->rate_filters.clear();
}

int srt_check_config(const srt_config* cfg, const char* who)
{
    if (cfg->F < 64 || cfg->F > 2048 || cfg->F % 64 || cfg->T < 64 || cfg->T % 64)
        return srt_set_error(-1, "%s: F and T must be multiples of 64 (F <= 2048)", who);     // spleeter.c:113-119 floor-divides by 64
    if (cfg->n_stems < 1 || cfg->n_stems > SRT_MAX_STEMS || cfg->max_tiles < 1) return srt_set_error(-1, "%s: bad n_stems / max_tiles", who);
    return 0;
}

int srtCreate(const srt_config* cfg, void* stream, srt_engine** out)
{
    if (!cfg || !out) return fail(-1, "srtCreate: null argument");
    SrtSetupLock setup;
    if (const int rc = srt_check_config(cfg, "srtCreate")) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(-3, "srtCreate: no HIP device (this library has no CPU path)");
    srt_engine* e = new srt_engine();
    if (hipGetDevice(&e->device) != hipSuccess) { delete e; return fail(-3, "srtCreate: no current HIP device"); }
    e->cfg = *cfg;
    { const char* bi = getenv("SPLEETERRT_BATCH_INVARIANT"); if (bi && bi[0] == '1') e->cfg.batch_invariant = 1; }
    e->stream = (hipStream_t)stream; e->lo = make_layout(); e->last.ntiles = cfg->max_tiles;
    if (e->lo.total != SRT_COEFF_FLOATS) { delete e; return fail(-4, "internal: weight layout size mismatch"); }
    const size_t S = cfg->n_stems, NT = cfg->max_tiles, HW = (size_t)cfg->T * cfg->F;
#define EALLOC(ptr, nfloats) do { if (hipMalloc((void**)&(ptr), (nfloats) * sizeof(float)) != hipSuccess) { free_all(e); delete e; return fail(-2, "srtCreate: hipMalloc failed"); } } while (0)
    EALLOC(e->coeff_all, S * SRT_COEFF_STRIDE);
    if (cfg->precision != SRT_PREC_F32) {
        for (int i = 0; i < 6; ++i) {
            const LayerOff& D = e->lo.down[i]; const LayerOff& U = e->lo.up[i];
            e->wpack16_down_stem[i] = D.cin % 16 ? 0 : (size_t)(D.cin / 16) * 400 * D.cp;      // halves
            e->wpack16_up_stem[i] = U.cin % 16 ? 0 : (size_t)(U.cin / 16) * 400 * U.cp;
            if (e->wpack16_down_stem[i] && hipMalloc((void**)&e->wpack16_down[i], S * e->wpack16_down_stem[i] * 2) != hipSuccess) { free_all(e); delete e; return fail(-2, "srtCreate: hipMalloc failed"); }
            if (e->wpack16_up_stem[i] && hipMalloc((void**)&e->wpack16_up[i], S * e->wpack16_up_stem[i] * 2) != hipSuccess) { free_all(e); delete e; return fail(-2, "srtCreate: hipMalloc failed"); }
        }
    }
    EALLOC(e->wpack2_d1, (size_t)2 * 25 * 128);
    EALLOC(e->wpack2_u5, S * 64 * 15 * 32);
    // The Winograd-form layers only ever run on launches above 16 instances (forward_range: `few`) or under batch_invariant: an engine that can never
    // hold that many (every drop-in tile-API / plugin instance: 1 tile x 1-4 stems) does not allocate their transformed weights and input copies.
    const bool wino_possible = S * NT > 16 || e->cfg.batch_invariant || srt_wino_force();
    for (int i = 0; i < 6; ++i) {
        e->wpack_down_stem[i] = (size_t)e->lo.down[i].cin * 25 * e->lo.down[i].cp;
        e->wpack_up_stem[i] = (size_t)e->lo.up[i].cin * 25 * e->lo.up[i].cp;
        EALLOC(e->wpack_down[i], S * e->wpack_down_stem[i]);
        EALLOC(e->wpack_up[i], S * e->wpack_up_stem[i]);
        // Winograd form of the decoder layers named by srt_wino_mask() (fp32 MFMA path): [Cin/4][Cout/16][4][16][52] per stem
        const LayerOff& U = e->lo.up[i];
        if (wino_possible && cfg->impl == SRT_IMPL_MFMA && cfg->precision == SRT_PREC_F32 && ((srt_wino_mask() >> i) & 1) && U.cout % 16 == 0 && U.cin % 4 == 0) {
            e->wino_u_stem[i] = (size_t)U.cin * U.cout * 52;
            EALLOC(e->wino_u[i], S * e->wino_u_stem[i]);
        }
        const LayerOff& Dn = e->lo.down[i];
        if (wino_possible && cfg->impl == SRT_IMPL_MFMA && cfg->precision == SRT_PREC_F32 && i >= 1 && srt_enc_wino_covers(Dn.cin, Dn.cout, cfg->T >> i, cfg->F >> i)) {
            e->wino_e_stem[i] = (size_t)Dn.cin * Dn.cout * 52;
            EALLOC(e->wino_e[i], S * e->wino_e_stem[i]);
            EALLOC(e->act32[i - 1], S * NT * ((size_t)ENC_CH[i - 1][1] * (HW >> (2 * i))));        // act(BN(raw_{i-1})): this layer's input
        }
    }
    // fp16 activation storage: every layer between down1 and up6 must run on the fp16-MFMA kernels, which stage aligned
    // 4-pixel row segments at every level (up1's input is F/64 wide): F % 256 == 0.  Other geometries keep fp32 tensors.
    e->act16 = cfg->precision == SRT_PREC_F16 && cfg->impl == SRT_IMPL_MFMA && cfg->F % 256 == 0;
    if (e->act16 && hipMalloc((void**)&e->wpack16cs_u5, S * SRT_W16CS_U5 * 2) != hipSuccess) { free_all(e); delete e; return fail(-2, "srtCreate: hipMalloc failed"); }
    for (int i = 0; i < 6; ++i) {
        e->raw_tile[i] = (size_t)ENC_CH[i][1] * (HW >> (2 * (i + 1)));
        EALLOC(e->raw[i], (S * NT * e->raw_tile[i] + (e->act16 ? 1 : 0)) / (e->act16 ? 2 : 1));
        if (e->act16 && i < 5) EALLOC(e->act16buf[i], (S * NT * e->raw_tile[i] + 1) / 2);
        e->up_tile[i] = (size_t)DEC_CH[i][1] * (HW >> (2 * (5 - i)));
        EALLOC(e->up[i], (S * NT * e->up_tile[i] + (e->act16 && i < 5 ? 1 : 0)) / (e->act16 && i < 5 ? 2 : 1));      // up6's output (the head's input) stays fp32
    }
    e->rows_cap = NT * cfg->T;
    EALLOC(e->preWin, SRT_FFT); EALLOC(e->postWin, SRT_FFT); EALLOC(e->twiddle, 2 * SRT_FFT);
    EALLOC(e->spec, 2 * 2 * e->rows_cap * SRT_SPEC_LD);
    EALLOC(e->mag, NT * 2 * HW);
    EALLOC(e->masks, S * NT * 2 * HW);
#undef EALLOC
    // tables: same formulas and float rounding as InitSTFT (stftFix.c:302-313)
    std::vector<float> pre(SRT_FFT), post(SRT_FFT), tw(2 * SRT_FFT), sig(1026);
    const double w0 = 6.283185307179586476925286766559 / SRT_FFT;
    const float postScale = (float)SRT_FFT * ((1.0f / 2.0f) / (3.0f / 8.0f));
    for (int i = 0; i < SRT_FFT; ++i) {
        const float hs = (float)((1.0 / SRT_FFT) * (0.5 * (1.0 - cos(w0 * (i + 0.5)))));
        pre[i] = hs * (2.0f / 4.0f);
        post[i] = hs * postScale * 0.5f;
        tw[2 * i] = (float)cos(w0 * i); tw[2 * i + 1] = (float)(-sin(w0 * i));
    }
    // logistic LUT of the Executable flavour (spleeter.c:29): 1025 samples on [-7,7] + trailing 1.0, regenerated in closed form
    for (int i = 0; i < 1025; ++i) sig[i] = (float)(1.0 / (1.0 + exp(7.0 - 0.013671875 * i)));
    sig[1025] = 1.0f;
    if (hipMemcpy(e->preWin, pre.data(), SRT_FFT * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->postWin, post.data(), SRT_FFT * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->twiddle, tw.data(), 2 * SRT_FFT * 4, hipMemcpyHostToDevice) != hipSuccess ||
        srt_set_sigmoid_table(sig.data()) != 0) { free_all(e); delete e; return fail(-2, "srtCreate: table upload failed"); }
    *out = e;
    return 0;
}

void srtDestroy(srt_engine* e)
{
    if (!e) return;
    DeviceScope ds(e->device);
    hipStreamSynchronize(e->stream);
    free_all(e);
    delete e;
}

// SRT_PREC_F16X2 promises fp32-level parity, which holds only while every weight that goes through the fp16 pack is an fp16 value: refuse a blob that
// is not (the caller picks SRT_PREC_F32, or SRT_PREC_F16 with its 2e-2 tolerance class, knowingly) instead of silently rounding it.
static int check_f16x2_weights(srt_engine* e, int stem)
{
    unsigned* d_count = nullptr; unsigned bad = 0; size_t total = 0;
    HIPCHK(hipMalloc((void**)&d_count, sizeof(unsigned)));
    hipError_t er = hipMemsetAsync(d_count, 0, sizeof(unsigned), e->stream);
    const float* c = e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE;
    for (int i = 0; i < 6 && er == hipSuccess; ++i) {
        const LayerOff& D = e->lo.down[i]; const LayerOff& U = e->lo.up[i];
        if (e->wpack16_down[i]) { total += (size_t)25 * D.cin * D.cout; if (srt_launch_count_not_fp16(c + D.w, (size_t)25 * D.cin * D.cout, d_count, e->stream)) er = hipErrorLaunchFailure; }
        if (e->wpack16_up[i]) { total += (size_t)25 * U.cin * U.cout; if (srt_launch_count_not_fp16(c + U.w, (size_t)25 * U.cin * U.cout, d_count, e->stream)) er = hipErrorLaunchFailure; }
    }
    if (er == hipSuccess) er = hipMemcpyAsync(&bad, d_count, sizeof(unsigned), hipMemcpyDeviceToHost, e->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    hipFree(d_count);
    HIPCHK(er);
    if (bad) {
        e->have_coeff[stem] = false;
        char what[96];
        snprintf(what, sizeof what, "sub-network %d: %u of %zu are not and would be rounded", stem, bad, total);
        return fail(-5, "srtSetCoeff: SRT_PREC_F16X2 needs fp16-representable conv weights (%s); use SRT_PREC_F32, or SRT_PREC_F16 for the fp16 tolerance class", what);
    }
    return 0;
}

static int pack_stem(srt_engine* e, int stem)
{
    if (e->cfg.precision == SRT_PREC_F16X2 && e->cfg.impl == SRT_IMPL_MFMA) { const int rc = check_f16x2_weights(e, stem); if (rc) return rc; }
    for (int i = 0; i < 6; ++i) {
        const LayerOff& D = e->lo.down[i]; const LayerOff& U = e->lo.up[i];
        const float* c = e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE;
        if (srt_launch_pack_enc(c + D.w, e->wpack_down[i] + stem * e->wpack_down_stem[i], D.cin, D.cout, D.cp, e->stream)) return fail(-2, "pack launch failed");
        if (srt_launch_pack_dec(c + U.w, e->wpack_up[i] + stem * e->wpack_up_stem[i], U.cin, U.cout, U.cp, e->stream)) return fail(-2, "pack launch failed");
        if (e->wpack16_down[i] && srt_launch_pack16(c + D.w, e->wpack16_down[i] + stem * e->wpack16_down_stem[i], D.cin, D.cout, D.cp, 0, e->stream)) return fail(-2, "pack launch failed");
        if (e->wpack16_up[i] && srt_launch_pack16(c + U.w, e->wpack16_up[i] + stem * e->wpack16_up_stem[i], U.cin, U.cout, U.cp, 1, e->stream)) return fail(-2, "pack launch failed");
        if (e->wino_u[i] && srt_launch_pack_wino(c + U.w, e->wino_u[i] + stem * e->wino_u_stem[i], U.cin, U.cout, e->stream)) return fail(-2, "pack launch failed");
        if (e->wino_e[i] && srt_launch_pack_wino_enc(c + D.w, e->wino_e[i] + stem * e->wino_e_stem[i], D.cin, D.cout, e->stream)) return fail(-2, "pack launch failed");
    }
    if (srt_launch_pack_classstack(e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE + e->lo.up[4].w, e->wpack2_u5 + (size_t)stem * 64 * 15 * 32, 64, 16, e->stream))
        return fail(-2, "pack launch failed");
    if (e->wpack16cs_u5 && srt_launch_pack16_classstack(e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE + e->lo.up[4].w, e->wpack16cs_u5 + (size_t)stem * SRT_W16CS_U5, 64, 16, e->stream))
        return fail(-2, "pack launch failed");
    e->have_coeff[stem] = true;
    return 0;
}

int srtSetCoeffHost(srt_engine* e, int stem, const void* h)
{
    if (!e || !h || stem < 0 || stem >= e->cfg.n_stems) return fail(-1, "srtSetCoeffHost: bad argument");
    SrtSetupLock setup;
    DeviceScope ds(e->device);
    HIPCHK(hipMemcpyAsync(e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE, h, srtCoeffBytes(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return pack_stem(e, stem);
}
int srtSetCoeffDevice(srt_engine* e, int stem, const void* d)
{
    if (!e || !d || stem < 0 || stem >= e->cfg.n_stems) return fail(-1, "srtSetCoeffDevice: bad argument");
    SrtSetupLock setup;
    DeviceScope ds(e->device);
    HIPCHK(hipMemcpyAsync(e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE, d, srtCoeffBytes(), hipMemcpyDeviceToDevice, e->stream));
    return pack_stem(e, stem);
}
// read the fp32 blob of a sub-network back (what srtSetCoeff* stored: for the fp16 container, the expanded values)
int srtGetCoeffHost(srt_engine* e, int stem, void* h)
{
    if (!e || !h || stem < 0 || stem >= e->cfg.n_stems) return fail(-1, "srtGetCoeffHost: bad argument");
    SrtSetupLock setup;
    DeviceScope ds(e->device);
    HIPCHK(hipMemcpyAsync(h, e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE, srtCoeffBytes(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}
int srtSetCoeffFp16Host(srt_engine* e, int stem, const uint16_t* h)
{
    if (!e || !h || stem < 0 || stem >= e->cfg.n_stems) return fail(-1, "srtSetCoeffFp16Host: bad argument");
    SrtSetupLock setup;
    DeviceScope ds(e->device);
    uint16_t* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, (size_t)SRT_COEFF_FLOATS * 2));
    hipError_t er = hipMemcpyAsync(d, h, (size_t)SRT_COEFF_FLOATS * 2, hipMemcpyHostToDevice, e->stream);
    if (er == hipSuccess) { srt_fp16_expand(d, e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE, SRT_COEFF_FLOATS, e->stream); er = hipStreamSynchronize(e->stream); }
    hipFree(d);
    HIPCHK(er);
    return pack_stem(e, stem);
}


// Small batches (the real-time plugin: 1 tile x 4 stems; BASELINE configs[1]: 1 x 2) leave most CUs idle in the deep layers:
// the launchers get a workspace so they can cut those layers' K loops into slices (srt_nn2.hip, split-K).
static void ensure_ws(srt_engine* e, size_t instances)
{
    if (e->ws || instances > 16 || e->cfg.batch_invariant || e->cfg.impl != SRT_IMPL_MFMA || e->cfg.precision != SRT_PREC_F32) return;
    const size_t want = (size_t)16 << 20;                  // 64 MiB: 8 slices of the largest split layer at 8 instances
    if (hipMalloc((void**)&e->ws, want * sizeof(float)) == hipSuccess) e->ws_floats = want;
    else { e->ws = nullptr; (void)hipGetLastError(); }
}

SrtSwitches srt_read_switches()
{
    SrtSwitches sw;
#define SRT_SW_READ(field, name, dflt, rule) { const char* v = getenv(name); sw.field = SRT_SW_##rule == SRT_SW_FLAG ? !(v && v[0] == '0') : (SRT_SW_##rule == SRT_SW_INT_NONEMPTY ? v && v[0] : v != nullptr) ? atoi(v) : dflt; }
    SRT_SWITCH_TABLE(SRT_SW_READ)
#undef SRT_SW_READ
    return sw;
}

bool stream_capturing(const srt_engine* e) { hipStreamCaptureStatus cap = hipStreamCaptureStatusNone; if (e->stream) (void)hipStreamIsCapturing(e->stream, &cap); return cap != hipStreamCaptureStatusNone; }

// Graph-mode preamble of srtForward / srtSeparateEx: completes `valid` with the weights, allocates the split-K workspace (never inside a capture) and
// starts the key - zeroed, the call kind and the switches; the caller adds its arguments.  Returns `valid`.
bool graph_prepare(srt_engine* e, bool valid, size_t ntiles, int kind, const SrtSwitches& sw, GraphKey* k)
{
    for (int s = 0; s < e->cfg.n_stems; ++s) valid = valid && e->have_coeff[s];
    if (valid && !stream_capturing(e)) ensure_ws(e, (size_t)e->cfg.n_stems * ntiles);
    memset(k, 0, sizeof *k);
    k->kind = kind; k->sw = sw;
    return valid;
}

// One forward_range call: its stem range and tiles and the kernel-choice flags that follow from the launch size.
struct ForwardPlan {
    int ntiles, s0, ns;
    // few: at most 16 instances keep the direct kernels and (small: when the workspace exists) cut the deep layers' K loops into slices; larger launches run up1..up5 and
    // down3..down6 in Winograd form.  batch_invariant: never few (ws stays null) - the Winograd-form layers wherever the geometry fits, the same bits for a tile in any batch.
    bool few, small;
    // c8: fp16 storage, launches above 16 instances - the tensors between down2 and up5 are channel-interleaved by eight, the layers run on the DMA-fed kernels of srt_nn5.hip;
    // c8_l1: ... and down1's two outputs (raw1: up6's skip input, act1: down2's input) where down1 runs on its streamed kernels.  (sw.c8 / sw.c8l1 = 0: planar, for A/B runs)
    bool c8, c8_l1;
    unsigned elu_mask;          // all stems go in one launch per layer; the activation pair is per stem (spleeter.c:130-139) and travels as a bit mask
    const float* cbase;         // the first stem's coefficient blob
};

// what the two layer kinds set alike: channels, batch, the stems' weights, the split-K workspace of small launches
static SrtConvParams layer_params(const srt_engine* e, const ForwardPlan& f, const LayerOff& L, float* wpack, size_t wpack_stem, int act)
{
    SrtConvParams p; memset(&p, 0, sizeof p);
    p.Cin = L.cin; p.Cout = L.cout; p.ntiles = f.ntiles; p.nstems = f.ns;
    p.wraw = f.cbase + L.w; p.bias = f.cbase + L.b; p.coeff_stem = SRT_COEFF_STRIDE;
    p.wpack = wpack + (size_t)f.s0 * wpack_stem; p.wpack_stem = wpack_stem; p.CP = L.cp;
    p.act = act; p.elu_mask = f.elu_mask; p.variant = e->cfg.variant;
    if (f.small) { p.ws = e->ws; p.ws_floats = e->ws_floats; }
    return p;
}

static SrtConvParams encoder_params(const srt_engine* e, const ForwardPlan& f, int i, const float* d_mag)
{
    const LayerOff& L = e->lo.down[i];
    const int nt = f.ntiles;
    SrtConvParams p = layer_params(e, f, L, e->wpack_down[i], e->wpack_down_stem[i], SRT_ACT_LEAKY);
    p.H = e->cfg.T >> i; p.W = e->cfg.F >> i; p.CA = L.cin;
    if (i == 0) { p.srcA = d_mag; p.srcA_stem = 0; p.srcA_tile = 2 * (size_t)e->cfg.T * e->cfg.F; }     // every stem reads the same magnitudes
    else {
        // the previous layer's conv + bias; its batch-norm + activation (spleeter.c:188) is applied by this layer while staging
        const LayerOff& P = e->lo.down[i - 1];
        p.srcA_stem = (size_t)nt * e->raw_tile[i - 1]; p.srcA_tile = e->raw_tile[i - 1];
        if (e->act16) {            // fp16 storage: the producer wrote act(bn(raw)) as a second fp16 tensor (see srt_enc_f16)
            p.srcA = stem_at(e, e->act16buf[i - 1], e->raw_tile[i - 1], nt, f.s0);
            p.in16 = 1;
        } else {
            p.srcA = stem_at(e, e->raw[i - 1], e->raw_tile[i - 1], nt, f.s0);
            p.inShift = f.cbase + P.bn; p.inScale = f.cbase + P.bn + P.cout;
        }
    }
    p.srcB = p.srcA;
    p.outRaw = stem_at(e, e->raw[i], e->raw_tile[i], nt, f.s0);
    p.out16 = e->act16;
    if (e->act16 && i < 5) {
        p.outAct = stem_at(e, e->act16buf[i], e->raw_tile[i], nt, f.s0);
        p.bnShift = f.cbase + L.bn; p.bnScale = f.cbase + L.bn + L.cout;
    }
    p.out_stem = (size_t)nt * e->raw_tile[i]; p.out_tile = e->raw_tile[i];
    if (i == 0) p.c8out = f.c8_l1;
    return p;
}

static SrtConvParams decoder_params(const srt_engine* e, const ForwardPlan& f, int i)
{
    const LayerOff& L = e->lo.up[i];
    const int nt = f.ntiles, sk = 5 - i;                                        // skip tensor = raw[5-i]; up1 consumes conv6 alone
    SrtConvParams p = layer_params(e, f, L, e->wpack_up[i], e->wpack_up_stem[i], SRT_ACT_RELU);
    p.H = e->cfg.T >> (6 - i); p.W = e->cfg.F >> (6 - i);
    p.srcA = stem_at(e, e->raw[sk], e->raw_tile[sk], nt, f.s0); p.srcA_stem = (size_t)nt * e->raw_tile[sk]; p.srcA_tile = e->raw_tile[sk];
    if (i == 0) { p.CA = L.cin; p.srcB = p.srcA; p.srcB_stem = p.srcA_stem; p.srcB_tile = p.srcA_tile; }
    else {
        p.CA = L.cin / 2;
        p.srcB = stem_at(e, e->up[i - 1], e->up_tile[i - 1], nt, f.s0); p.srcB_stem = (size_t)nt * e->up_tile[i - 1]; p.srcB_tile = e->up_tile[i - 1];
    }
    p.in16 = e->act16; p.out16 = e->act16 && i < 5;
    p.c8srcB = f.c8 && i == 5;                                                  // up6 reads up5's C8 output
    p.c8srcA = f.c8_l1 && i == 5;                                               // ... and down1's raw tensor, its skip input, where that is C8 too
    p.bnShift = f.cbase + L.bn; p.bnScale = f.cbase + L.bn + L.cout;
    p.outAct = stem_at(e, e->up[i], e->up_tile[i], nt, f.s0, i == 5);           // up6's output (the head's input) stays fp32
    p.out_stem = (size_t)nt * e->up_tile[i]; p.out_tile = e->up_tile[i];
    if (i == 4) { p.wpack2 = e->wpack2_u5 + (size_t)f.s0 * 64 * 15 * 32; p.wpack2_stem = 64 * 15 * 32; p.CP2 = 32; }
    return p;
}

// Encoder layer i (spleeter.c:182-238) on the first kernel of the chain that covers it (launchers return 1 = not covered).
// act_ready: act32[i-1] holds act(BN(raw_{i-1})) of this batch - carried from layer to layer.
static int launch_encoder_layer(srt_engine* e, const SrtSwitches& sw, const ForwardPlan& f, int i, SrtConvParams p, bool& act_ready)
{
    const LayerOff& L = e->lo.down[i];
    const int nt = f.ntiles;
    // down1's own forms come first: on the fp16 MFMA, every stem of the call (up to six) in ONE launch (fp16 mode, C8 outputs: srt_down1_f16_kernel;
    // sw.d1f16 = 0: the fp32-MFMA streamed kernels below, for A/B runs and the parity test)
    if (i == 0 && f.c8_l1 && e->cfg.precision == SRT_PREC_F16 && p.nstems <= 6 && !f.small && sw.d1f16) {
        p.stack = p.nstems;
        TimerScope tg(e, "down1");
        const int rg = srt_launch_down1_f16(p, e->stream);
        if (rg == 0) return 0;
        if (rg != 1) return fail(-2, "encoder launch failed");
        p.stack = 0;
    }
    if (i == 0 && e->cfg.impl == SRT_IMPL_MFMA) {
        // stem-stacked M: all stems of the group share the input.  More than four sub-networks (BASELINE configs[4]: five): the streamed down1 kernel stacks at
        // most 4 x 16 rows, so the first whole groups of four go out here, each as its own stacked launch; the remainder (1..4 stems) follows the common chain
        while (p.nstems > 4) {
            SrtConvParams q = p;
            q.nstems = 4; q.stack = 4; q.CP2 = 64; q.wpack2 = e->wpack2_d1; q.wpack2_stem = 0;
            if (srt_launch_pack_stemstack(q.wraw, SRT_COEFF_STRIDE, 4, e->wpack2_d1, L.cin, L.cout, q.CP2, e->stream)) return fail(-2, "pack launch failed");
            { TimerScope tg(e, "down1"); const int rg = srt_launch_enc2(q, sw, e->stream);
              if (rg == 1) return fail(-4, "internal: stem-stacked down1 group not covered by its launcher");
              if (rg) return fail(-2, "encoder launch failed"); }
            p.nstems -= 4; p.elu_mask >>= 4;
            p.wpack += 4 * p.wpack_stem;                                 // (the per-stem packs advance with the group too - the remainder launch's fallbacks read them)
            p.wraw += 4 * (size_t)SRT_COEFF_STRIDE; p.bias += 4 * (size_t)SRT_COEFF_STRIDE;
            if (p.bnShift) { p.bnShift += 4 * (size_t)SRT_COEFF_STRIDE; p.bnScale += 4 * (size_t)SRT_COEFF_STRIDE; }
            p.outRaw = eoff(e, p.outRaw, 4 * p.out_stem);
            if (p.outAct) p.outAct = eoff(e, p.outAct, 4 * p.out_stem);
        }
        p.stack = p.nstems; p.CP2 = (p.nstems * 16 + 63) / 64 * 64; p.wpack2 = e->wpack2_d1; p.wpack2_stem = 0;
        if (srt_launch_pack_stemstack(p.wraw, SRT_COEFF_STRIDE, p.nstems, e->wpack2_d1, L.cin, L.cout, p.CP2, e->stream)) return fail(-2, "pack launch failed");
    }
    // Winograd form (down3..down6 of launches above 16 instances): reads the act(BN(raw)) copy of its input, writes raw + its own copy when
    // the next layer runs here too.  The first such layer's input copy is written by the direct layer in front (producer_copy); only when that layer
    // ran on a kernel without the second output does a batched bn+act pass over its raw tensor make the copy here.
    const bool ewino = !f.few && e->wino_e[i] && !e->act16;
    if (ewino) {
        float* copy = stem_at(e, e->act32[i - 1], e->raw_tile[i - 1], nt, f.s0, true);
        if (!act_ready) {
            const LayerOff& P = e->lo.down[i - 1];
            TimerScope ta(e, "actcopy");
            if (srt_launch_bn_act_batch(stem_at(e, e->raw[i - 1], e->raw_tile[i - 1], nt, f.s0, true), copy, f.cbase + P.bn + P.cout, f.cbase + P.bn, SRT_COEFF_STRIDE,
                                        f.ns, nt, P.cout, e->raw_tile[i - 1] / P.cout, SRT_ACT_LEAKY, f.elu_mask, e->cfg.variant, e->stream)) return fail(-2, "bn-act launch failed");
        }
        p.srcA = copy; p.srcB = p.srcA;
        p.inScale = p.inShift = nullptr;
    }
    act_ready = ewino && i + 1 < 6 && e->wino_e[i + 1] != nullptr;          // this layer writes the next one's input copy
    // a direct layer in front of the first Winograd-form one writes that copy itself (srt_enc_mfma2, second fp32 output): one more store per
    // element instead of a pass that reads the tensor back.  Only the plain MFMA kernel does that (not the split-K one of small batches).
    const bool next_wino = !f.few && i > 0 && i + 1 < 6 && e->wino_e[i + 1] && e->act32[i] && !e->act16;
    const bool producer_copy = !ewino && next_wino && e->cfg.impl == SRT_IMPL_MFMA && !f.small && srt_enc_producer_copy();
    if (act_ready || producer_copy) {
        p.outAct = stem_at(e, e->act32[i], e->raw_tile[i], nt, f.s0, true);
        p.bnShift = f.cbase + L.bn; p.bnScale = f.cbase + L.bn + L.cout;
    }
    TimerScope ts(e, ("down" + std::to_string(i + 1)).c_str());
    int rc = 1;
    if (ewino) {
        rc = srt_launch_enc_wino(p, e->wino_e[i] + (size_t)f.s0 * e->wino_e_stem[i], e->wino_e_stem[i], e->stream);
        if (rc == 1) return fail(-4, "internal: Winograd encoder layer not covered by its launcher");
    }
    if (rc == 1 && e->cfg.impl == SRT_IMPL_MFMA && e->wpack16_down[i]) {
        p.wpack16 = e->wpack16_down[i] + (size_t)f.s0 * e->wpack16_down_stem[i]; p.wpack16_stem = e->wpack16_down_stem[i];
        p.nsplit = e->cfg.precision == SRT_PREC_F16X2 ? 2 : 1;
        if (f.c8 && (i >= 2 || f.c8_l1)) {                                  // C8 in, C8 out (srt_nn5.hip); down2 when down1 wrote its act copy C8
            rc = srt_launch_enc_c8(p, sw, e->stream);
            if (rc == 1) return fail(-4, "internal: C8 activation layout but no C8 kernel for an encoder layer");
        } else {
            p.c8out = f.c8 && i == 1;                                       // down2: planar input (down1's act copy), C8 outputs
#ifdef SRT_TUNING
            // timing experiment (wrong results): down2 on the C8 kernel as if its input were C8 - what moving down1's act copy to C8 would buy
            static const bool d2c8 = []() { const char* v = getenv("SRT_TUNE_D2C8"); return v && v[0] == '1'; }();
            if (d2c8 && p.c8out) rc = srt_launch_enc_c8(p, sw, e->stream); else
#endif
            rc = srt_launch_enc_f16(p, e->stream);
        }
    }
    if (e->act16 && i > 0 && rc == 1) return fail(-4, "internal: fp16 activation storage but no fp16 kernel for an encoder layer");
    if (rc == 1 && e->cfg.impl == SRT_IMPL_MFMA) { rc = srt_launch_enc2(p, sw, e->stream); if (rc == 0 && producer_copy) act_ready = true; }
    if (rc < 0) return fail(-2, "encoder launch failed");
    if (rc == 1 && srt_launch_enc(p, e->cfg.impl, e->stream)) return fail(-2, "encoder launch failed");
    return 0;
}

// Decoder layer i (spleeter.c:239-294), the same protocol.  up6 runs together with the head where that form is covered: head_done.
static int launch_decoder_layer(srt_engine* e, const SrtSwitches& sw, const ForwardPlan& f, int i, SrtConvParams p, const SrtHeadParams& head, bool& head_done)
{
    TimerScope ts(e, ("up" + std::to_string(i + 1)).c_str());
    int rc = 1;
    if (e->cfg.impl == SRT_IMPL_MFMA && e->wpack16_up[i]) {
        p.wpack16 = e->wpack16_up[i] + (size_t)f.s0 * e->wpack16_up_stem[i]; p.wpack16_stem = e->wpack16_up_stem[i];
        p.nsplit = e->cfg.precision == SRT_PREC_F16X2 ? 2 : 1;
        if (f.c8 && i < 5) {                                                // C8 in, C8 out (up5: class-stacked weights)
            p.wpack16cs = e->wpack16cs_u5 + (size_t)f.s0 * SRT_W16CS_U5; p.wpack16cs_stem = SRT_W16CS_U5;
            rc = srt_launch_dec_c8(p, sw, e->stream);
            if (rc == 1) return fail(-4, "internal: C8 activation layout but no C8 kernel for a decoder layer");
        } else rc = srt_launch_dec_f16(p, e->stream);
    }
    if (i == 5) {                                                           // up6 + head in one pass where covered (srt_up6_head_kernel); the plane is then not stored
        const unsigned bits = ((1u << f.ns) - 1u) << f.s0;
        e->last.up6_fused &= ~bits;
        if (e->cfg.impl == SRT_IMPL_MFMA && !e->graph_mode) {               // (graphs are for launches far below this form's threshold; lifting the gate changes what they record)
            rc = srt_launch_up6_head(p, head, sw, e->stream);
            if (rc == 0) { head_done = true; e->last.up6_fused |= bits; e->last.up6_params = p; e->last.up6_s0 = f.s0; }
        }
    }
    if (e->act16 && i < 5 && rc == 1) return fail(-4, "internal: fp16 activation storage but no fp16 kernel for a decoder layer");
    if (rc == 1 && e->wino_u[i] && (!f.few || srt_wino_force())) {
        SrtSwitches swd = sw;
        if (swd.wino_ac && (e->graph_mode || stream_capturing(e))) swd.wino_ac = 0;      // (as for up6 + head above: what a graph records stays what it was)
        rc = srt_launch_dec_wino(p, e->wino_u[i] + (size_t)f.s0 * e->wino_u_stem[i], e->wino_u_stem[i], swd, e->stream);
    }
    if (rc == 1 && e->cfg.impl == SRT_IMPL_MFMA) rc = srt_launch_dec2(p, e->stream);
    if (rc < 0) return fail(-2, "decoder launch failed");
    if (rc == 1 && srt_launch_dec(p, e->cfg.impl, e->stream)) return fail(-2, "decoder launch failed");
    return 0;
}

// Sub-networks [s0, s0+ns) on ntiles tiles.  Buffers keep their all-stem layout (stem stride = ntiles instances), so a
// later call for other stems of the same batch lands beside this one's results.  masks16_req: the masks may leave as halves
// (honoured only for the engine's own mask buffer and where the head kernel takes it; e->last.masks16 says what happened).
int forward_range(srt_engine* e, const SrtSwitches& sw, const float* d_mag, int ntiles, float* d_masks, int s0, int ns, bool masks16_req)
{
    if (!e || !d_mag || !d_masks) return fail(-1, "srtForward: null argument");
    DeviceScope ds(e->device);
    if (ntiles < 1 || ntiles > e->cfg.max_tiles) return fail(-1, "srtForward: ntiles exceeds max_tiles");
    const int S = e->cfg.n_stems, T = e->cfg.T, F = e->cfg.F;
    if (s0 < 0 || ns < 1 || s0 + ns > S) return fail(-1, "srtForward: stem range outside the engine's sub-networks");
    for (int s = s0; s < s0 + ns; ++s) if (!e->have_coeff[s]) return fail(-5, "srtForward: weights not set for every stem");
    const size_t HW = (size_t)T * F;
    if (!stream_capturing(e)) ensure_ws(e, (size_t)ns * ntiles);                // (no allocation inside a capture: callers pre-allocate)
    ForwardPlan f;
    f.ntiles = ntiles; f.s0 = s0; f.ns = ns; f.elu_mask = 0;
    f.few = (size_t)ns * ntiles <= 16 && !e->cfg.batch_invariant;
    f.small = f.few && e->ws;
    f.c8 = e->act16 && !f.few && sw.c8;
    f.c8_l1 = f.c8 && sw.c8l1 && e->cfg.impl == SRT_IMPL_MFMA && srt_down1_c8_ok(T, F, ntiles, (size_t)ntiles * e->raw_tile[0], sw);
    for (int s = 0; s < ns; ++s) if (e->cfg.stem_mode[s0 + s]) f.elu_mask |= 1u << s;
    f.cbase = e->coeff_all + (size_t)s0 * SRT_COEFF_STRIDE;
    e->last.ntiles = ntiles; e->last.c8 = f.c8; e->last.c8_l1 = f.c8_l1; e->last.masks16 = false;
    bool act_ready = false;
    for (int i = 0; i < 6; ++i)
        if (const int rc = launch_encoder_layer(e, sw, f, i, encoder_params(e, f, i, d_mag), act_ready)) return rc;
    SrtHeadParams head; memset(&head, 0, sizeof head);                         // head (spleeter.c:295-300)
    head.H = T; head.W = F; head.ntiles = ntiles; head.nstems = ns;
    head.src = stem_at(e, e->up[5], e->up_tile[5], ntiles, s0, true); head.src_stem = (size_t)ntiles * e->up_tile[5]; head.src_tile = e->up_tile[5];
    head.w = f.cbase + e->lo.head_w; head.bias = f.cbase + e->lo.head_b; head.coeff_stem = SRT_COEFF_STRIDE;
    head.out = stem_at(e, d_masks, 2 * HW, ntiles, s0, true); head.out_stem = (size_t)ntiles * 2 * HW; head.out_tile = 2 * HW;
    head.variant = e->cfg.variant;
    head.out16 = masks16_req && d_masks == e->masks && srt_head_out16_ok(head);
    e->last.masks16 = head.out16 != 0;
    bool head_done = false;
    for (int i = 0; i < 6; ++i)
        if (const int rc = launch_decoder_layer(e, sw, f, i, decoder_params(e, f, i), head, head_done)) return rc;
    if (!head_done) {
        TimerScope ts(e, "up7");
        if (srt_launch_head(head, e->stream)) return fail(-2, "head launch failed");
    }
    return 0;
}

int srtForward(srt_engine* e, const float* d_mag, int ntiles, float* d_masks)
{
    if (!e) return fail(-1, "srtForward: null argument");
    const SrtSwitches sw = srt_read_switches();
    if (!e->graph_mode) return forward_range(e, sw, d_mag, ntiles, d_masks, 0, e->cfg.n_stems);
    DeviceScope ds(e->device);
    GraphKey k;
    const bool valid = graph_prepare(e, d_mag && d_masks && ntiles >= 1 && ntiles <= e->cfg.max_tiles, ntiles, 1, sw, &k);
    k.p0 = d_mag; k.p2 = d_masks; k.ntiles = ntiles; k.ns = e->cfg.n_stems;
    return run_graphed(e, k, valid, [&]() { return forward_range(e, sw, d_mag, ntiles, d_masks, 0, e->cfg.n_stems); });
}

int srtPrepareForward(srt_engine* e, const float* d_mag, int ntiles, float* d_masks)
{
    if (!e) return fail(-1, "srtPrepareForward: null argument");
    SrtSetupLock setup;
    DeviceScope ds(e->device);
    const int rc = srtForward(e, d_mag, ntiles, d_masks);     // allocates the workspace, captures + instantiates (graph mode), runs once
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int srtReleaseStaging(srt_engine* e)
{
    if (!e) return fail(-1, "srtReleaseStaging: null argument");
    DeviceScope ds(e->device);
    if (e->hs.ready) { hipStreamSynchronize(e->hs.s_in); hipStreamSynchronize(e->hs.s_out); }
    HIPCHK(hipStreamSynchronize(e->stream));
    free_staging(e);
    return 0;
}

int srtForwardStems(srt_engine* e, const float* d_mag, int ntiles, float* d_masks, int stem0, int nstems)
{
    if (!e) return fail(-1, "srtForward: null argument");
    return forward_range(e, srt_read_switches(), d_mag, ntiles, d_masks, stem0, nstems);
}

int srtSetGraphMode(srt_engine* e, int enable)
{
    if (!e) return fail(-1, "null engine");
    DeviceScope ds(e->device);
    if (!enable) { hipStreamSynchronize(e->stream); free_graphs(e); }
    e->graph_mode = enable != 0;
    return 0;
}

const float* srt_engine_coeff_device(const srt_engine* e, int stem) { return e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE; }
int srt_engine_device(const srt_engine* e) { return e->device; }
void* srt_engine_stream(const srt_engine* e) { return (void*)e->stream; }
