// srt_engine.hip — engine object, HBM layout and the device-resident C ABI (include/spleeterrt_amd.h).
//
// HBM layout (all fp32, instance = (stem, tile), CHW planar, row = time, contiguous = frequency):
//   coeff[stem]           raw spleeterCoeff blob (Executable/spleeter.h:5-31), biases / BN read in place
//   wpack[stem][layer]    GEMM-ready weights [Cin][25][CP]
//   raw[i]  i=0..5        encoder conv+bias outputs   [stem][tile][Cout][H>>i+1][W>>i+1]: the skip tensors AND the next encoder
//                         layer's input (its BN + activation is applied by the consumer while staging; nothing is stored twice)
//   up[i]   i=0..5        decoder outputs (new channels only; the concat is done by pointer)
//   spec / mag / masks / frames / pcm for the DSP stages
#include "srt_internal.h"
#include "../../include/spleeterrt_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <cxxabi.h>
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
static int fail(int code, const char* fmt, const char* detail = "") { return srt_set_error(code, fmt, detail); }

// first kernel the calling thread launched since the last reset (SRT_LAUNCH, srt_internal.h)
static thread_local const void* g_kfn = nullptr;
static thread_local const char* g_ktext = nullptr;
void srt_kernel_note(const void* fn, const char* text) { if (!g_kfn) { g_kfn = fn; g_ktext = text; } }
void srt_kernel_note_reset() { g_kfn = nullptr; g_ktext = nullptr; }
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(-2, "HIP error: %s", hipGetErrorString(_e)); } while (0)

static const int ENC_CH[6][2] = { {2, 16}, {16, 32}, {32, 64}, {64, 128}, {128, 256}, {256, 512} };
static const int DEC_CH[6][2] = { {512, 256}, {512, 128}, {256, 64}, {128, 32}, {64, 16}, {32, 1} };

struct LayerOff { size_t w, b, bn; int cin, cout, cp; };
#define SRT_W16CS_U5 ((size_t)(64 / 16) * 15 * 2 * 32 * 8)    // halves per stem of up5's class-stacked fp16 weights
struct Layout { LayerOff down[6], up[6]; size_t head_w, head_b, total; };

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

struct TimingEntry { std::string name; hipEvent_t a, b; const void* kfn; const char* ktext; };
#define SRT_TIMING_MAX 65536        // launches recorded per srtSetTiming(1) window; later launches run untimed

// Persistent staging of srtSeparateHostStream / srtSeparateCliHost: device double buffers, copy streams and events are
// created on first use, grown when a call needs more, and freed with the engine (not allocated per call).
struct HostStaging {
    float* d_in[2]; float* d_out[2]; float* d_carry;
    size_t in_cap, out_cap, carry_cap;                 // floats
    hipStream_t s_in, s_out;
    hipEvent_t ev_in[2], ev_cmp[2], ev_out[2];
    bool ready;
    // 16-bit PCM forms (SRT_HOST_IN_PCM16 / SRT_HOST_OUT_PCM16, srt_pcm.hip): allocated only when a call asks for them
    int16_t* d_in16[2]; int16_t* d_out16[2];
    size_t in16_cap, out16_cap;                        // stereo frames (4 bytes)
    unsigned long long* d_clip;                        // [SRT_MAX_STEMS] clipped-sample counters, then the pack's workgroup counts
};

// What the last forward left behind, for the calls that come after it (srtCopyTensor's taps, the inverse transform of srtSeparate).  forward_range and
// wiener_issue write it; a graph replay runs no host code, so the slot keeps the record its capture left and run_graphed puts it back.
struct ForwardRecord {
    int ntiles;                        // instance stride of the activation buffers = tiles of that forward
    bool c8, c8_l1, masks16;           // raw2..6 / act2..5 / up1..4 are channel-interleaved by eight (srt_nn5.hip); conv1 / act1 too; the engine's OWN mask buffer holds halves
    unsigned up6_fused; int up6_s0; SrtConvParams up6_params;     // bit s: stem s ran up6 + head in one pass (no up6 plane stored) - srtCopyTensor("up6") re-launches up6 alone from that launch's stem range and parameters
    int wiener_last;                   // iterations of the last filtered call: the R tables srtCopyTensor("wiener_cov") can return
    int wiener_tracks;                 // ... which was a batch of this many tracks (srtSeparateBatchWiener: the per-track tables); 0: a single-signal call
    int ext_rows;                      // rows of the gain table the last inverse transform with the average mask extension filled (srtCopyTensor("mask_ext")); 0: none
};

// hipGraph replay of the launch sequences a low-latency caller repeats with the same arguments (srtSetGraphMode): the real-time
// plugin runs srtForward on the same two mask buffers for ever, the tile API on one pair of buffers.  A sequence is captured
// the first time its argument tuple is seen and replayed afterwards: one host call instead of ~25 launches on the audio thread.
// `sw`: the run-time switches of the call (SrtSwitches, srt_internal.h) - all of them decide what a forward records, so a flipped switch captures a new
// graph instead of replaying the old form.  Keys are zeroed before they are filled and compared with memcmp.
#define SRT_BATCH_SLOTS 4
// `overlap`: the rows consecutive network tiles share (srtSetOverlap) - a sequence captured at one overlap is never replayed at another.
// `mask_ext`: the rule for bins >= F (srtSetMaskExtension), for the same reason.
// `mix_gen`: the generation of the stem remix matrix (srtSetMix bumps it; 0 while the mix is off) - a changed matrix never replays a graph captured with the old one
// (the matrix travels by value in the captured launch).
struct GraphKey { int kind; const void* p0; const void* p1; void* p2; size_t n, frames, rows; int ntiles, s0, ns, wiener; SrtSwitches sw; int overlap, mask_ext; unsigned mix_gen; };
// left: e->last as the capture left it (an eager call in between may have changed it)
struct GraphSlot { GraphKey key; hipGraph_t graph; hipGraphExec_t exec; unsigned long used; ForwardRecord left; };
#define SRT_GRAPH_SLOTS 4

// Every entry point that allocates or launches runs on the device the engine was created on, whatever the caller's
// current device is (a host thread that switched devices after srtCreate must not mix device-A streams with device-B memory).
struct DeviceScope {
    int prev; bool sw;
    explicit DeviceScope(int dev) : prev(-1), sw(false) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) sw = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() { if (sw) hipSetDevice(prev); }
};

struct srt_engine {
    srt_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    HostStaging hs{};
    Layout lo{};
    float* coeff_all = nullptr;                        // [n_stems][SRT_COEFF_STRIDE]
    float* wpack_down[6] = {}; float* wpack_up[6] = {};  // per layer: [n_stems][Cin*25*CP]
    size_t wpack_down_stem[6] = {}, wpack_up_stem[6] = {};
    uint16_t* wpack16_down[6] = {}; uint16_t* wpack16_up[6] = {};  // fp16-MFMA packs [n_stems][Cin/16][25][2][CP][8] (precision != F32 only)
    size_t wpack16_down_stem[6] = {}, wpack16_up_stem[6] = {};
    float* wpack2_d1 = nullptr;                        // down1 stem-stacked [2][25][CP2], repacked per launch group (tiny)
    float* wpack2_u5 = nullptr;                        // up5 class-stacked [n_stems][64][15][32]
    float* wino_u[6] = {}; size_t wino_u_stem[6] = {};   // Winograd-transformed decoder weights (srt_nn4.hip), layers in srt_wino_mask() only
    float* wino_e[6] = {}; size_t wino_e_stem[6] = {};   // the same for the encoder layers that can run in Winograd form (down3..down6)
    float* act32[6] = {};                              // fp32 act(BN(raw_i)) copies, i = 2..4: the inputs of those layers (written by their producers)
    bool   have_coeff[SRT_MAX_STEMS] = {};
    float* raw[6] = {}; float* up[6] = {};
    size_t raw_tile[6] = {}, up_tile[6] = {};          // elements per instance
    float* act16buf[5] = {};                           // fp16-storage mode only: act(bn(raw_i)) as halves, written by the producer
    bool act16 = false;                                // raw[0..5] and up[0..4] hold IEEE halves (precision F16 on a supported geometry)
    uint16_t* wpack16cs_u5 = nullptr;                  // act16 only: up5's class-stacked fp16 weights [n_stems][4][15][2][32][8] (srt_nn5.hip)
    ForwardRecord last{};                              // what the last forward left (ntiles starts at max_tiles: srtCreate)
    float* ws = nullptr; size_t ws_floats = 0;         // split-K partial sums of small-batch launches (allocated on the first one)
    int graph_mode = 0; unsigned long gclock = 0; GraphSlot gslots[SRT_GRAPH_SLOTS] = {};
    // DSP
    float *preWin = nullptr, *postWin = nullptr; float2* twiddle = nullptr;
    float2* spec = nullptr; float2* spec2 = nullptr; float* mag = nullptr; float* masks = nullptr;   // spec2: residual spectrum of the CLI chain (on first use)
    size_t rows_cap = 0;
    // multichannel Wiener filter (srt_wiener.hip, srtSetWiener): allocated for max_tiles when it is switched on (or by the first srtIstftWiener)
    int wiener = 0;                                    // EM iterations applied by srtSeparate / srtSeparateEx, 0: off
    // overlapped network tiles (srtSetOverlap): rows two consecutive tiles of one signal share, 0: back-to-back tiles (the reference's cut)
    int overlap = 0;
    float* wslab = nullptr;                            // statistics partials + block maxima
    float* wtab = nullptr;                             // R tables, weight sums, a
    float2* wspec = nullptr;                           // filtered spectra [n_stems][2][rows][SRT_SPEC_LD]
    // average mask extension (srtSetMaskExtension): the gain table [n_stems][rows_cap][2], allocated when the mode is first switched on
    int mask_ext = SRT_MASK_EXT_CONSTANT;
    float* ext = nullptr;
    // stem remix (srtSetMix): mix_out > 0 - the inverse transform of srtIstft / srtSeparate / the host stream writes mix_out pairs, each the chain
    // of mix[m] over the stems' gains; mix_gen counts the calls that switched it on (the graph key)
    int mix_out = 0; unsigned mix_gen = 0;
    float mix[SRT_MAX_STEMS][SRT_MAX_STEMS + 1] = {};
    // packed batches of tracks (srtSeparateBatch): the device track table (max_tiles rows: every track takes at least one tile) and a ring of pinned
    // host slots it is uploaded from, each reused only after the copy from it issued SRT_BATCH_SLOTS calls earlier has completed (bev)
    SrtBatchTrack* btab = nullptr; SrtBatchTrack* bpin = nullptr;
    hipEvent_t bev[SRT_BATCH_SLOTS] = {}; bool bused[SRT_BATCH_SLOTS] = {}; int bslot = 0;
    // ... with the Wiener filter per track (srtSeparateBatchWiener): the second table (device + the same ring of pinned slots), the statistics slab of
    // max_tiles * T / 16 + max_tiles chunks with its block maxima, and the per-track tables [max_tiles] x (R [3][S][F][4], weight sums [3][S][F]) + a [max_tiles].
    // Allocated by the first such call and owned by bwmem; separate from wslab / wtab, whose addresses a captured single-signal graph may hold (wspec, written
    // and read inside one call, is shared).
    SrtMem bwmem;
    SrtBatchWiener* bwtab = nullptr; SrtBatchWiener* bwpin = nullptr;
    float* bwslab = nullptr; float* bwtabf = nullptr;
    // timing
    bool timing = false; std::vector<TimingEntry> tlog;
};

const char* srtLastError(void) { return g_err; }
size_t srtCoeffBytes(void) { return (size_t)SRT_COEFF_FLOATS * 4; }
size_t srtStftRows(size_t n) { return (n + SRT_HOP - 1) / SRT_HOP; }
size_t srtStftFrames(size_t n) { return n < SRT_FFT ? 0 : (n - SRT_FFT + SRT_HOP / 4) / SRT_HOP + 1; }   // stftFix.c:378 + tail frame
size_t srtIstftLength(size_t rows) { return rows * SRT_HOP + (SRT_FFT - SRT_HOP); }

// Overlapped network tiles, the one rule (mirrored by spleeterrt_amd/stream.py:overlap_tiles): stride S = T - O, tile j covers rows [jS, jS + T); one tile up
// to T rows, else ceil((rows - O) / S) - every tile then owns a row no earlier tile covers, and the tiles cover all rows.  O = 0: ceil(rows / T).
static size_t overlap_tiles(size_t rows, int T, int O) { return rows == 0 ? 0 : rows <= (size_t)T ? 1 : (rows - O + (T - O) - 1) / (T - O); }
size_t srtOverlapTiles(size_t rows, int T, int overlap_rows)
{
    if (T < 1 || overlap_rows < 0 || overlap_rows > T / 2) { fail(-1, "srtOverlapTiles: need T >= 1 and 0 <= overlap <= T / 2"); return 0; }
    return overlap_tiles(rows, T, overlap_rows);
}
static size_t tiles_of(const srt_engine* e, size_t rows) { return overlap_tiles(rows, e->cfg.T, e->overlap); }     // network tiles of a signal of `rows` rows
static const char* const OVERLAP_REFUSED = "%s: not available with overlapped tiles (srtSetOverlap > 0; DESIGN.md 13 lists it as a follow-up): srtSetOverlap(e, 0) first";

int srtSetOverlap(srt_engine* e, int overlap_rows)
{
    if (!e) return fail(-1, "srtSetOverlap: null engine");
    if (overlap_rows < 0 || overlap_rows > e->cfg.T / 2) return fail(-1, "srtSetOverlap: the overlap must be 0 (off) .. T / 2 rows");
    e->overlap = overlap_rows;
    return 0;
}
int srt_engine_overlap(const srt_engine* e) { return e->overlap; }

static const char* const MIX_REFUSED = "%s: not available with the stem remix on (srtSetMix; DESIGN.md 16 lists it as a follow-up): srtSetMix(e, 0, NULL) first";
int srtSetMix(srt_engine* e, int n_out, const float* h_gain)
{
    if (!e) return fail(-1, "srtSetMix: null engine");
    if (n_out < 0 || n_out > SRT_MAX_STEMS) return fail(-1, "srtSetMix: n_out must be 0 (off) .. SRT_MAX_STEMS");
    if (n_out && !h_gain) return fail(-1, "srtSetMix: null gain matrix");
    const int S = e->cfg.n_stems;
    for (int i = 0; i < n_out * (S + 1); ++i) if (!isfinite(h_gain[i])) return fail(-1, "srtSetMix: every gain must be finite");
    if (n_out && e->wiener) return fail(-1, "srtSetMix: the stem remix is not available with the Wiener filter on (the mix of filtered spectra is a follow-up, DESIGN.md 16): srtSetWiener(e, 0) first");
    memset(e->mix, 0, sizeof e->mix);
    for (int m = 0; m < n_out; ++m) for (int s = 0; s <= S; ++s) e->mix[m][s] = h_gain[m * (S + 1) + s];
    e->mix_out = n_out;
    if (n_out) { if (!++e->mix_gen) ++e->mix_gen; }
    return 0;
}
int srtMixOutputs(const srt_engine* e) { return e ? e->mix_out : 0; }
int srt_engine_mix(const srt_engine* e) { return e->mix_out; }

static const char* const MASK_EXT_REFUSED = "%s: not available with the average mask extension (srtSetMaskExtension; DESIGN.md 15 lists it as a follow-up): srtSetMaskExtension(e, SRT_MASK_EXT_CONSTANT) first";
static bool stream_capturing(const srt_engine* e);

int srtSetMaskExtension(srt_engine* e, int mode)
{
    if (!e) return fail(-1, "srtSetMaskExtension: null engine");
    if (mode != SRT_MASK_EXT_CONSTANT && mode != SRT_MASK_EXT_AVERAGE) return fail(-1, "srtSetMaskExtension: the mode must be SRT_MASK_EXT_CONSTANT (0) or SRT_MASK_EXT_AVERAGE (1)");
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

// element offset into an activation tensor whose elements are halves (act16) or floats
static inline float* eoff(const srt_engine* e, float* base, size_t elems) { return (float*)((char*)base + elems * (e->act16 ? 2 : 4)); }

struct TimerScope {
    srt_engine* e; size_t idx; bool on;
    TimerScope(srt_engine* e_, const char* name) : e(e_), idx(0), on(e_->timing && e_->tlog.size() < SRT_TIMING_MAX) {
        if (!on) return;
        TimingEntry t; t.name = name; t.kfn = nullptr; t.ktext = nullptr;
        srt_kernel_note_reset();
        if (hipEventCreate(&t.a) != hipSuccess) { on = false; return; }
        if (hipEventCreate(&t.b) != hipSuccess) { hipEventDestroy(t.a); on = false; return; }
        hipEventRecord(t.a, e->stream);
        e->tlog.push_back(t); idx = e->tlog.size() - 1;
    }
    ~TimerScope() { if (on) { hipEventRecord(e->tlog[idx].b, e->stream); e->tlog[idx].kfn = g_kfn; e->tlog[idx].ktext = g_ktext; } }
};

static void free_staging(srt_engine* e)
{
    HostStaging& h = e->hs;
    for (int b = 0; b < 2; ++b) {
        if (h.d_in[b]) hipFree(h.d_in[b]);
        if (h.d_out[b]) hipFree(h.d_out[b]);
        if (h.d_in16[b]) hipFree(h.d_in16[b]);
        if (h.d_out16[b]) hipFree(h.d_out16[b]);
        if (h.ev_in[b]) hipEventDestroy(h.ev_in[b]);
        if (h.ev_cmp[b]) hipEventDestroy(h.ev_cmp[b]);
        if (h.ev_out[b]) hipEventDestroy(h.ev_out[b]);
    }
    if (h.d_carry) hipFree(h.d_carry);
    if (h.d_clip) hipFree(h.d_clip);
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

// Run `issue` (a function that only enqueues work on e->stream) through the graph cache when graph mode is on.  `valid` says
// whether the arguments passed the entry point's checks: an invalid call is issued eagerly (it fails with its own error code and
// nothing is captured).  Graph mode is switched off for good only when the capture / instantiate API itself fails - a user error
// such as missing weights leaves it on.  If the caller's stream is already capturing (the caller builds its own graph), the
// launches simply join that capture.
template <class F>
static int run_graphed(srt_engine* e, const GraphKey& key, bool valid, F&& issue)
{
    if (!e->graph_mode || e->timing || !e->stream || !valid) return issue();      // the legacy null stream cannot be captured
    for (GraphSlot& g : e->gslots)
        if (g.exec && !memcmp(&g.key, &key, sizeof key)) {
            g.used = ++e->gclock;
            HIPCHK(hipGraphLaunch(g.exec, e->stream));
            const int tables = e->last.wiener_last, wtracks = e->last.wiener_tracks, ext_rows = e->last.ext_rows;
            e->last = g.left;
            if (!key.wiener) { e->last.wiener_last = tables; e->last.wiener_tracks = wtracks; }      // a sequence without the filter leaves the R tables of an earlier call as they are
            if (!key.mask_ext) e->last.ext_rows = ext_rows;                 // ... and one without the mask extension the gain table
            return 0;
        }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(e->stream, &cap) != hipSuccess) { (void)hipGetLastError(); return issue(); }
    if (cap != hipStreamCaptureStatusNone) return issue();                 // inside the caller's capture: do not nest one
    if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); e->graph_mode = 0; return issue(); }
    const int rc = issue();
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipError_t er = hipStreamEndCapture(e->stream, &graph);
    if (rc) {
        // A launch failed INSIDE the capture.  The arguments were validated above, so the likeliest cause is the capture itself having been
        // invalidated from outside (another host thread's legacy-stream operation while this stream was capturing): run the sequence once
        // more, eagerly - if it fails again the error is real and is returned; graph mode stays on either way.
        if (graph) hipGraphDestroy(graph);
        (void)hipGetLastError();
        return issue();
    }
    if (er == hipSuccess && graph) er = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (er != hipSuccess || !exec) {                                       // capture is not available here: plain launches from now on
        if (graph) hipGraphDestroy(graph);
        (void)hipGetLastError();
        e->graph_mode = 0;
        return issue();
    }
    GraphSlot* v = &e->gslots[0];
    for (GraphSlot& g : e->gslots) if (!g.exec || g.used < v->used) { v = &g; if (!g.exec) break; }
    if (v->exec) hipGraphExecDestroy(v->exec);
    if (v->graph) hipGraphDestroy(v->graph);
    v->key = key; v->graph = graph; v->exec = exec; v->used = ++e->gclock;
    v->left = e->last;
    HIPCHK(hipGraphLaunch(exec, e->stream));
    return 0;
}

static bool stream_capturing(const srt_engine* e) { hipStreamCaptureStatus cap = hipStreamCaptureStatusNone; if (e->stream) (void)hipStreamIsCapturing(e->stream, &cap); return cap != hipStreamCaptureStatusNone; }

// Graph-mode preamble of srtForward / srtSeparateEx: completes `valid` with the weights, allocates the split-K workspace (never inside a capture) and
// starts the key - zeroed, the call kind and the switches; the caller adds its arguments.  Returns `valid`.
static bool graph_prepare(srt_engine* e, bool valid, size_t ntiles, int kind, const SrtSwitches& sw, GraphKey* k)
{
    for (int s = 0; s < e->cfg.n_stems; ++s) valid = valid && e->have_coeff[s];
    if (valid && !stream_capturing(e)) ensure_ws(e, (size_t)e->cfg.n_stems * ntiles);
    memset(k, 0, sizeof *k);
    k->kind = kind; k->sw = sw;
    return valid;
}

// first element of (stem, tile) in an all-stem activation buffer of a forward over ntiles tiles (stem stride = ntiles instances of `per` elements);
// the elements are halves or floats as the engine stores activations (eoff) unless f32 says floats (up6's plane, the fp32 copies, the masks)
static inline float* stem_at(const srt_engine* e, float* buf, size_t per, int ntiles, int stem, bool f32 = false, int tile = 0) { const size_t el = ((size_t)stem * ntiles + tile) * per; return f32 ? buf + el : eoff(e, buf, el); }

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
    if (rc == 1 && e->wino_u[i] && (!f.few || srt_wino_force())) rc = srt_launch_dec_wino(p, e->wino_u[i] + (size_t)f.s0 * e->wino_u_stem[i], e->wino_u_stem[i], sw, e->stream);
    if (rc == 1 && e->cfg.impl == SRT_IMPL_MFMA) rc = srt_launch_dec2(p, e->stream);
    if (rc < 0) return fail(-2, "decoder launch failed");
    if (rc == 1 && srt_launch_dec(p, e->cfg.impl, e->stream)) return fail(-2, "decoder launch failed");
    return 0;
}

// Sub-networks [s0, s0+ns) on ntiles tiles.  Buffers keep their all-stem layout (stem stride = ntiles instances), so a
// later call for other stems of the same batch lands beside this one's results.  masks16_req: the masks may leave as halves
// (honoured only for the engine's own mask buffer and where the head kernel takes it; e->last.masks16 says what happened).
static int forward_range(srt_engine* e, const SrtSwitches& sw, const float* d_mag, int ntiles, float* d_masks, int s0, int ns, bool masks16_req = false)
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

int srtRatioMask(srt_engine* e, float* d_masks, int ntiles)
{
    if (!e || !d_masks || ntiles < 1) return fail(-1, "srtRatioMask: bad argument");
    DeviceScope ds(e->device);
    TimerScope ts(e, "ratio");
    if (srt_launch_ratio_mask(d_masks, e->cfg.n_stems, (size_t)ntiles * 2 * e->cfg.T * e->cfg.F, e->stream)) return fail(-2, "ratio-mask launch failed");
    return 0;
}

static SrtDspTables tables_of(const srt_engine* e) { SrtDspTables t; t.preWin = e->preWin; t.postWin = e->postWin; t.twiddle = e->twiddle; return t; }

int srtStftEx(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_spec, float* d_mag)
{
    if (!e || !d_L || !d_R || !d_spec) return fail(-1, "srtStft: null argument");
    DeviceScope ds(e->device);
    if (rows < 1 || frames > rows) return fail(-1, "srtStft: need 1 <= frames <= rows");
    const int T = e->cfg.T, O = d_mag ? e->overlap : 0;
    const size_t ntiles = tiles_of(e, rows);
    if (d_mag && ntiles > (size_t)e->cfg.max_tiles) return fail(-1, e->overlap ? "srtStft: more than max_tiles tiles at this overlap (srtOverlapTiles)" : "srtStft: more than max_tiles * T rows");
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

int srtStft(srt_engine* e, const float* d_L, const float* d_R, size_t n, float* d_spec, float* d_mag)
{
    if (n < SRT_FFT) return fail(-1, "srtStft: need at least 4096 samples");          // the reference underflows here (stftFix.c:378)
    return srtStftEx(e, d_L, d_R, n, srtStftFrames(n), srtStftRows(n), d_spec, d_mag);
}

// average mask extension: the gain table of the inverse transform that follows on the same stream, from the masks that transform will apply
// (rows <= rows_cap: every caller has checked its tiles against max_tiles)
// (tracks: a packed batch with overlapped tiles - rows = the packed rows, each mapped inside its own track: srt_launch_mask_ext_batch)
static int mask_ext_issue(srt_engine* e, const float* masks, int masks16, int nstems, int ntiles, int rows, int ratio, int O, const SrtBatchTrack* tracks = nullptr, int ntracks = 0)
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
static int istft_launch(srt_engine* e, const float2* spec, size_t rows, const float* masks, int nstems, const float* oob, bool ratio, bool masks16, float* d_out, bool mix = false)
{
    DeviceScope ds(e->device);
    const int T = e->cfg.T;
    SrtIstftParams p; memset(&p, 0, sizeof p);
    p.spec = spec; p.spec_ch_stride = rows * SRT_SPEC_LD;
    const int O = masks ? e->overlap : 0;               // (the single-stem callers - CLI flows, Wiener filter - refuse an overlap before they get here)
    p.frames = (int)rows; p.masks = masks; p.nstems = nstems; p.ntiles = (int)(O ? tiles_of(e, rows) : (rows + T - 1) / T);
    p.T = T; p.F = e->cfg.F;
    const bool ext = e->mask_ext == SRT_MASK_EXT_AVERAGE;      // (its single-stem callers - CLI flows, Wiener filter - refuse the mode before they get here)
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
static int istft_one(srt_engine* e, const float2* spec, size_t rows, const float* mask_stem, float oob, float* d_dst) { return istft_launch(e, spec, rows, mask_stem, 1, &oob, false, false, d_dst); }
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
static int wiener_issue(srt_engine* e, const float* d_spec, size_t rows, const float* d_masks, int iters, float* d_out)
{
    const int T = e->cfg.T, S = e->cfg.n_stems, F = e->cfg.F;
    SrtWienerParams w; memset(&w, 0, sizeof w);
    w.spec = (const float2*)d_spec; w.spec_ch_stride = rows * SRT_SPEC_LD; w.rows = (int)rows;
    w.masks = d_masks; w.nstems = S; w.ntiles = (int)((rows + T - 1) / T); w.T = T; w.F = F;
    int nch = (int)((rows + 15) / 16); if (nch > SRT_WIENER_MAX_CHUNKS) nch = SRT_WIENER_MAX_CHUNKS;
    w.rpc = (int)((rows + nch - 1) / nch); w.nchunks = (int)((rows + w.rpc - 1) / w.rpc);
    w.slab = e->wslab; w.slab_max = e->wslab + (size_t)SRT_WIENER_MAX_CHUNKS * S * 4 * F;
    w.rtab = e->wtab; w.wsum = e->wtab + (size_t)SRT_WIENER_MAX_ITERS * S * F * 4; w.scal = w.wsum + (size_t)SRT_WIENER_MAX_ITERS * S * F;
    w.out = e->wspec; w.out_stem = 2 * rows * SRT_SPEC_LD;
    for (int pass = 1; pass <= iters; ++pass) {
        { TimerScope ts(e, "wiener_stats"); if (srt_launch_wiener_stats(w, pass, e->stream)) return fail(-2, "Wiener statistics launch failed"); }
        { TimerScope ts(e, "wiener_cov"); if (srt_launch_wiener_finalize(w, pass, e->stream)) return fail(-2, "Wiener finalize launch failed"); }
    }
    { TimerScope ts(e, "wiener_filter"); if (srt_launch_wiener_filter(w, iters, e->stream)) return fail(-2, "Wiener filter launch failed"); }
    e->last.wiener_last = iters; e->last.wiener_tracks = 0;
    const size_t len = srtIstftLength(rows);
    for (int j = 0; j < S; ++j) {
        const int rc = istft_one(e, e->wspec + (size_t)j * w.out_stem, rows, nullptr, e->cfg.oob_weight[j], d_out + (size_t)j * 2 * len);
        if (rc) return rc;
    }
    return 0;
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
static bool masks16_wanted(const srt_engine* e, const SrtSwitches& sw) { return e->cfg.precision == SRT_PREC_F16 && e->act16 && !e->cfg.ratio_mask && !e->wiener && !e->mix_out && e->cfg.F <= 1024 && sw.m16; }

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

int srtSetGraphMode(srt_engine* e, int enable)
{
    if (!e) return fail(-1, "null engine");
    DeviceScope ds(e->device);
    if (!enable) { hipStreamSynchronize(e->stream); free_graphs(e); }
    e->graph_mode = enable != 0;
    return 0;
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
static int cli_time_residual(srt_engine* e, const float* d_L, const float* d_R, size_t n, int stems, float* d_out, size_t len, size_t lo = 0, size_t hi = 0)
{
    TimerScope ts(e, "residual");
    if (!hi) hi = len;
    const int rc = stems == 2 ? srt_launch_time_residual(d_L, d_R, n, d_out, len, d_out + 2 * len, lo, hi, e->stream)
                              : srt_launch_time_residual(d_out + 4 * len, d_out + 5 * len, len, d_out + 2 * len, len, d_out + 4 * len, lo, hi, e->stream);
    return rc ? fail(-2, "residual launch failed") : 0;
}

static int cli_issue(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, int stems, float* d_out, bool residual_now)
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

static int cli_check(srt_engine* e, int stems)
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

// Grow-only device staging shared by the host-buffer entry points (kept in the engine, freed by srtDestroy).
static int ensure_staging(srt_engine* e, size_t in_floats, size_t out_floats, size_t carry_floats, int nbuf)
{
    HostStaging& h = e->hs;
    if (!h.ready) {
        HIPCHK(hipStreamCreateWithFlags(&h.s_in, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&h.s_out, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipEventCreateWithFlags(&h.ev_in[b], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h.ev_cmp[b], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h.ev_out[b], hipEventDisableTiming));
        }
        h.ready = true;
    }
    if (in_floats > h.in_cap || out_floats > h.out_cap || carry_floats > h.carry_cap) {
        // buffers may still be in use by an earlier call's asynchronous work: drain before replacing them
        HIPCHK(hipStreamSynchronize(h.s_in)); HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipStreamSynchronize(h.s_out));
    }
    for (int b = 0; b < 2; ++b) {
        if (in_floats > h.in_cap || (b < nbuf && !h.d_in[b])) {
            if (h.d_in[b]) { hipFree(h.d_in[b]); h.d_in[b] = nullptr; }
            if (b < nbuf) HIPCHK(hipMalloc((void**)&h.d_in[b], (in_floats > h.in_cap ? in_floats : h.in_cap) * sizeof(float)));
        }
        if (out_floats > h.out_cap || (b < nbuf && !h.d_out[b])) {
            if (h.d_out[b]) { hipFree(h.d_out[b]); h.d_out[b] = nullptr; }
            if (b < nbuf) HIPCHK(hipMalloc((void**)&h.d_out[b], (out_floats > h.out_cap ? out_floats : h.out_cap) * sizeof(float)));
        }
    }
    if (in_floats > h.in_cap) h.in_cap = in_floats;
    if (out_floats > h.out_cap) h.out_cap = out_floats;
    if (carry_floats > h.carry_cap) {
        if (h.d_carry) { hipFree(h.d_carry); h.d_carry = nullptr; }
        HIPCHK(hipMalloc((void**)&h.d_carry, carry_floats * sizeof(float)));
        h.carry_cap = carry_floats;
    }
    return 0;
}

// The 16-bit staging of the PCM16 flags, after ensure_staging (streams exist): grow-only like the float buffers; 0 frames = not wanted by this call.
static int ensure_staging16(srt_engine* e, size_t in_frames, size_t out_frames)
{
    HostStaging& h = e->hs;
    if (in_frames > h.in16_cap || out_frames > h.out16_cap) {
        HIPCHK(hipStreamSynchronize(h.s_in)); HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipStreamSynchronize(h.s_out));
    }
    for (int b = 0; b < 2; ++b) {
        if (in_frames > h.in16_cap) {
            if (h.d_in16[b]) { hipFree(h.d_in16[b]); h.d_in16[b] = nullptr; }
            HIPCHK(hipMalloc((void**)&h.d_in16[b], in_frames * 2 * sizeof(int16_t)));
        }
        if (out_frames > h.out16_cap) {
            if (h.d_out16[b]) { hipFree(h.d_out16[b]); h.d_out16[b] = nullptr; }
            HIPCHK(hipMalloc((void**)&h.d_out16[b], out_frames * 2 * sizeof(int16_t)));
        }
    }
    if (in_frames > h.in16_cap) h.in16_cap = in_frames;
    if (out_frames > h.out16_cap) h.out16_cap = out_frames;
    if (out_frames && !h.d_clip) HIPCHK(hipMalloc((void**)&h.d_clip, (SRT_MAX_STEMS + srt_pcm16_pack_scratch(SRT_MAX_STEMS)) * sizeof(unsigned long long)));
    return 0;
}

// seam: how a tile RANGE of a longer stream joins its neighbours when they run on other devices (srt_multi.hip); {0, nullptr, false} = the whole stream
struct SrtSeam { size_t out_stride; float* h_tail; bool head; };
static int host_stream(srt_engine* e, const void* h_in, const void* h_in2, size_t n, size_t frames, size_t rows, void* h_out, unsigned flags, int cli_stems,
                       SrtSeam seam = SrtSeam{0, nullptr, false}, unsigned long long* h_clipped = nullptr);

// Host-buffer form of srtSeparateCli for plain-C callers (the CLI harness): synchronous.  A file that fits the engine's capacity
// (max_tiles tiles) is one resident batch: H2D, chain, D2H.  A longer one - any length, as the reference's tile loop over a
// host-resident spectrogram handles (main.c:455-495) - goes through the chunked pipeline of srtSeparateHostStream: max_tiles tiles
// at a time, copies overlapped with compute, the residual chain evaluated per chunk (it is row-local) and the time-domain
// subtraction applied after the 3072-sample chunk overlaps have been added on the device.
// flags: SRT_HOST_* (srtSeparateCliHostIo).  A 16-bit side always takes the chunked pipeline, whose staging holds the conversion (one chunk when the file fits).
static int cli_host(srt_engine* e, const void* h_in, const void* h_in2, size_t n, int stems, void* h_out_, unsigned flags, unsigned long long* h_clipped)
{
    const bool pcm16 = flags & (SRT_HOST_IN_PCM16 | SRT_HOST_OUT_PCM16);
    if (!e || !h_in || (!(flags & SRT_HOST_IN_PCM16) && !h_in2) || !h_out_) return fail(-1, "srtSeparateCliHost: null argument");
    DeviceScope ds(e->device);
    int rc = cli_check(e, stems);
    if (rc) return rc;
    if (n < SRT_FFT) return fail(-1, "srtSeparateCli: need at least 4096 samples");
    const size_t rows = srtStftRows(n), len = srtIstftLength(rows);
    if (pcm16 || (rows + e->cfg.T - 1) / e->cfg.T > (size_t)e->cfg.max_tiles)
        return host_stream(e, h_in, h_in2, n, srtStftFrames(n), rows, h_out_, flags, stems, SrtSeam{0, nullptr, false}, h_clipped);
    const float *h_L = (const float*)h_in, *h_R = (const float*)h_in2;
    float* h_out = (float*)h_out_;
    if (h_clipped) memset(h_clipped, 0, (size_t)stems * sizeof *h_clipped);
    rc = ensure_staging(e, 2 * n, (size_t)stems * 2 * len, 0, 1);
    if (rc) return rc;
    float *d_in = e->hs.d_in[0], *d_out = e->hs.d_out[0];
    hipError_t er = hipMemcpyAsync(d_in, h_L, n * sizeof(float), hipMemcpyHostToDevice, e->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(d_in + n, h_R, n * sizeof(float), hipMemcpyHostToDevice, e->stream);
    rc = er == hipSuccess ? srtSeparateCli(e, d_in, d_in + n, n, stems, d_out) : fail(-2, "HIP error: %s", hipGetErrorString(er));
    if (!rc) {
        er = hipMemcpyAsync(h_out, d_out, (size_t)stems * 2 * len * sizeof(float), hipMemcpyDeviceToHost, e->stream);
        if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
        if (er != hipSuccess) rc = fail(-2, "HIP error: %s", hipGetErrorString(er));
    }
    hipStreamSynchronize(e->stream);
    return rc;                                                 // (the staging is grow-only and reused by later calls; srtReleaseStaging frees it)
}

int srtSeparateCliHost(srt_engine* e, const float* h_L, const float* h_R, size_t n, int stems, float* h_out)
{
    return cli_host(e, h_L, h_R, n, stems, h_out, 0, nullptr);
}

static const unsigned SRT_HOST_FLAGS = SRT_HOST_PINNED | SRT_HOST_IN_PCM16 | SRT_HOST_OUT_PCM16;
int srtSeparateCliHostIo(srt_engine* e, const void* h_in, const void* h_in2, size_t n, int stems, void* h_out, unsigned flags, unsigned long long* h_clipped)
{
    if (flags & ~SRT_HOST_FLAGS) return fail(-1, "srtSeparateCliHostIo: unknown flag bits");
    return cli_host(e, h_in, h_in2, n, stems, h_out, flags, h_clipped);
}

int srtSeparate(srt_engine* e, const float* d_L, const float* d_R, size_t n, float* d_out)
{
    if (n < SRT_FFT) return fail(-1, "srtSeparate: need at least 4096 samples");
    return srtSeparateEx(e, d_L, d_R, n, srtStftFrames(n), srtStftRows(n), d_out);
}

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
struct BatchCall { size_t total; SrtBatchGrid g; size_t ch_stride; int wchunks; };
static int batch_forward(srt_engine* e, const char* who, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out,
                         int wiener, int overlap, BatchCall* bc)
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
    if (e->mix_out) return fail(-1, MIX_REFUSED, who);
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
    if (srt_batch_geometry(h, ntracks, T, F, S, &bc->g)) return fail(-1, "%s: batch geometry out of range", who);
    bc->wchunks = 0;
    SrtBatchWiener* hw = wiener ? e->bwpin + (size_t)slot * e->cfg.max_tiles : nullptr;
    if (wiener) {
        bc->wchunks = srt_batch_wiener_geometry(h, hw, ntracks);
        if (bc->wchunks < 1 || (size_t)bc->wchunks > batch_wiener_chunk_cap(e)) return fail(-1, "%s: batch geometry out of range", who);
    }
    HIPCHK(hipMemcpyAsync(e->btab, h, (size_t)ntracks * sizeof(SrtBatchTrack), hipMemcpyHostToDevice, e->stream));
    if (wiener) HIPCHK(hipMemcpyAsync(e->bwtab, hw, (size_t)ntracks * sizeof(SrtBatchWiener), hipMemcpyHostToDevice, e->stream));
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
    return forward_range(e, sw, e->mag, (int)total, e->masks, 0, S, !wiener && masks16_wanted(e, sw));
}

// srtSeparateBatch (overlap = -1) and srtSeparateBatchOverlap (overlap >= 0): the shared front, the gain table of the average mask extension, one batched inverse
static int batch_separate(srt_engine* e, const char* who, int ntracks, const float* const* d_L, const float* const* d_R, const size_t* n, float* const* d_out, int overlap)
{
    DeviceScope ds(e->device);
    BatchCall bc;
    int rc = batch_forward(e, who, ntracks, d_L, d_R, n, d_out, 0, overlap, &bc);
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
    if (srt_launch_istft_batch(q, e->btab, ntracks, bc.g, e->stream, O)) return fail(-2, "batched istft launch failed");
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

// Long host-resident stream through one GPU: the stream is cut into chunks of max_tiles tiles (tiles are independent,
// main.c:455-495); chunk c+1's PCM goes up and chunk c-1's stems come down on two copy streams while chunk c computes,
// and the 3072-sample overlap between consecutive chunks is added on the device (srt_carry_kernel), so every output
// sample crosses PCIe exactly once.  Geometry as srtSeparateEx (a tile range of a longer stream: rows = whole tiles,
// frames = rows; the whole stream: rows = srtStftRows(n), frames = srtStftFrames(n)).
// cli_stems = 0: the n_stems sub-networks on the same input (srtSeparateEx per chunk); 2 / 3: the CLI's flows (cli_issue per chunk)
// seam (multi-device ranges, srt_multi.hip): h_out points at the range's first sample inside planes of seam.out_stride floats (the whole
// stream's output length); with seam.h_tail the range's last 3072 samples - the overlap-add contribution that belongs to the NEXT range's
// first samples - go to h_tail [planes][3072] instead of h_out; seam.head says a previous range will add its tail to this range's first
// 3072 samples.  The CLI flows' time-domain subtraction is left out on exactly those seam samples (both contributions have to be added
// first: the joiner does that, as the reference's main() does its subtraction on the host, main.c:794-798).
// 16-bit PCM (flags).  SRT_HOST_IN_PCM16: h_in is int16 [n][2] (h_in2 unused); a chunk's frames go up as one copy into d_in16[b] and are unpacked
// into d_in[b] on the compute stream (ev_cmp[b] releases both).  SRT_HOST_OUT_PCM16: h_out is int16 [planes / 2][total_len][2]; after the seam add (and the CLI
// flows' subtraction) the samples this chunk downloads - each plane's [0, take) - are packed into d_out16[b], so every output sample is quantised and counted
// once, and ev_cmp[b] is recorded after the pack.  h_clipped [stems]: the clipped samples of each stem (zero without the flag).
static int host_stream(srt_engine* e, const void* h_in, const void* h_in2, size_t n, size_t frames, size_t rows, void* h_out_, unsigned flags, int cli_stems, SrtSeam seam,
                       unsigned long long* h_clipped)
{
    const bool in16 = flags & SRT_HOST_IN_PCM16, out16 = flags & SRT_HOST_OUT_PCM16;
    if (!e || !h_in || (!in16 && !h_in2) || !h_out_) return fail(-1, "srtSeparateHostStream: null argument");
    if (in16 && h_in2) return fail(-1, "srtSeparateHostStream: SRT_HOST_IN_PCM16 takes one interleaved buffer (h_in2 must be NULL)");
    if ((in16 || out16) && seam.out_stride) return fail(-1, "srtSeparateHostStream: the 16-bit PCM forms do not apply to a tile range of a multi-device stream (the seam join adds floats on the host)");
    const float *h_L = (const float*)h_in, *h_R = (const float*)h_in2;
    float* h_out = (float*)h_out_;
    if (rows < 1 || frames > rows) return fail(-1, "srtSeparateHostStream: need 1 <= frames <= rows");
    if (e->overlap) return fail(-1, OVERLAP_REFUSED, "srtSeparateHostStream");  // the blend would have to cross the chunk seams
    if (e->wiener) return fail(-1, "srtSeparateHostStream: the Wiener filter's statistics span the whole signal (chunks would each get their own covariance): use srtSeparate, or srtSetWiener(e, 0)");
    DeviceScope ds(e->device);
    const int S = cli_stems ? cli_stems : e->mix_out ? e->mix_out : e->cfg.n_stems, T = e->cfg.T, NP = S * 2;     // pairs staged, carried, packed and downloaded: the outputs of a remix
    const size_t chunk_rows = (size_t)e->cfg.max_tiles * T, tail = SRT_FFT - SRT_HOP;
    const size_t nchunks = (rows + chunk_rows - 1) / chunk_rows, total_len = seam.out_stride ? seam.out_stride : srtIstftLength(rows);
    const size_t in_cap = chunk_rows * SRT_HOP + tail, out_cap = srtIstftLength(chunk_rows);
    int rc = ensure_staging(e, 2 * in_cap, (size_t)NP * out_cap, (size_t)NP * tail, 2);
    if (rc) return rc;
    if ((in16 || out16) && (rc = ensure_staging16(e, in16 ? in_cap : 0, out16 ? (size_t)S * out_cap : 0))) return rc;
    HostStaging& h = e->hs;
    if (h_clipped) memset(h_clipped, 0, (size_t)S * sizeof *h_clipped);
    unsigned long long* d_clip = out16 && h_clipped ? h.d_clip : nullptr;
    if (d_clip) HIPCHK(hipMemsetAsync(d_clip, 0, (size_t)S * sizeof *d_clip, e->stream));
    // Page-locked caller buffers let the copies run asynchronously.  SRT_HOST_PINNED: the caller guarantees they already are
    // (hipHostMalloc / hipHostRegister / torch pin_memory) and nothing is registered here; otherwise the three buffers are
    // registered for the duration of the call (if that fails the copies still work, staged by the runtime).
    bool pinL = false, pinR = false, pinO = false;
    if (!(flags & SRT_HOST_PINNED)) {
        pinL = hipHostRegister((void*)h_in, n * sizeof(float), hipHostRegisterDefault) == hipSuccess;       // int16 [n][2] is n * 4 bytes too
        pinR = !in16 && hipHostRegister((void*)h_R, n * sizeof(float), hipHostRegisterDefault) == hipSuccess;
        pinO = !seam.out_stride && hipHostRegister((void*)h_out, (size_t)NP * total_len * (out16 ? sizeof(int16_t) : sizeof(float)), hipHostRegisterDefault) == hipSuccess;
        (void)hipGetLastError();
    }
    hipError_t er = hipSuccess;
#define STEP(x) do { if (er == hipSuccess) er = (x); } while (0)
    for (size_t c = 0; c < nchunks && er == hipSuccess && rc == 0; ++c) {
        const int b = (int)(c & 1);
        const size_t row0 = c * chunk_rows, row1 = row0 + chunk_rows < rows ? row0 + chunk_rows : rows, crow = row1 - row0;
        const size_t s0 = row0 * SRT_HOP, send = row1 * SRT_HOP + tail < n ? row1 * SRT_HOP + tail : n;
        const size_t ns = send > s0 ? send - s0 : 0;
        const size_t cfr = frames > row0 ? (frames - row0 < crow ? frames - row0 : crow) : 0;
        const size_t clen = srtIstftLength(crow);
        // upload: the input buffer is free once the compute that read it two chunks ago has finished
        if (c >= 2) STEP(hipStreamWaitEvent(h.s_in, h.ev_cmp[b], 0));
        if (ns && in16) STEP(hipMemcpyAsync(h.d_in16[b], (const int16_t*)h_in + 2 * s0, ns * 2 * sizeof(int16_t), hipMemcpyHostToDevice, h.s_in));
        else if (ns) {
            STEP(hipMemcpyAsync(h.d_in[b], h_L + s0, ns * sizeof(float), hipMemcpyHostToDevice, h.s_in));
            STEP(hipMemcpyAsync(h.d_in[b] + in_cap, h_R + s0, ns * sizeof(float), hipMemcpyHostToDevice, h.s_in));
        }
        STEP(hipEventRecord(h.ev_in[b], h.s_in));
        // compute: needs this chunk's PCM and the output buffer drained by the download of two chunks ago
        STEP(hipStreamWaitEvent(e->stream, h.ev_in[b], 0));
        if (c >= 2) STEP(hipStreamWaitEvent(e->stream, h.ev_out[b], 0));
        if (er != hipSuccess) break;
        if (in16 && ns) {
            TimerScope ts(e, "pcm16_unpack");
            if (srt_launch_pcm16_unpack(h.d_in16[b], ns, h.d_in[b], h.d_in[b] + in_cap, e->stream)) { rc = fail(-2, "pcm16 unpack launch failed"); break; }
        }
        rc = cli_stems ? cli_issue(e, h.d_in[b], h.d_in[b] + in_cap, ns, cfr, crow, cli_stems, h.d_out[b], false)
                       : srtSeparateEx(e, h.d_in[b], h.d_in[b] + in_cap, ns, cfr, crow, h.d_out[b]);
        if (rc) break;
        if (srt_launch_carry(h.d_out[b], clen, NP, crow * SRT_HOP, h.d_carry, c == 0, c + 1 == nchunks, e->stream)) { rc = fail(-2, "carry launch failed"); break; }
        // CLI flows: the time-domain subtraction comes after the seam has been added (the planes now hold the stitched signals)
        const bool to_tail = c + 1 == nchunks && seam.h_tail;                      // the range's last 3072 samples belong to the next range's seam
        if (cli_stems) {
            const size_t lo = c == 0 && seam.head ? tail : 0, hi = to_tail ? crow * SRT_HOP : clen;
            if (hi > lo && (rc = cli_time_residual(e, h.d_in[b], h.d_in[b] + in_cap, ns, cli_stems, h.d_out[b], clen, lo, hi))) break;
        }
        const size_t take = c + 1 == nchunks && !to_tail ? clen : crow * SRT_HOP;
        if (out16) {
            TimerScope ts(e, "pcm16_pack");
            if (srt_launch_pcm16_pack(h.d_out[b], clen, S, take, h.d_out16[b], clen, d_clip, d_clip ? d_clip + SRT_MAX_STEMS : nullptr, e->stream)) { rc = fail(-2, "pcm16 pack launch failed"); break; }
        }
        STEP(hipEventRecord(h.ev_cmp[b], e->stream));
        // download: every plane's [0, crow*1024) (+ the final 3072 on the last chunk) lands at its place in h_out
        STEP(hipStreamWaitEvent(h.s_out, h.ev_cmp[b], 0));
        if (out16) STEP(hipMemcpy2DAsync((int16_t*)h_out_ + 2 * s0, total_len * 2 * sizeof(int16_t), h.d_out16[b], clen * 2 * sizeof(int16_t), take * 2 * sizeof(int16_t), S, hipMemcpyDeviceToHost, h.s_out));
        else STEP(hipMemcpy2DAsync(h_out + s0, total_len * sizeof(float), h.d_out[b], clen * sizeof(float), take * sizeof(float), NP, hipMemcpyDeviceToHost, h.s_out));
        if (to_tail) STEP(hipMemcpy2DAsync(seam.h_tail, tail * sizeof(float), h.d_out[b] + crow * SRT_HOP, clen * sizeof(float), tail * sizeof(float), NP, hipMemcpyDeviceToHost, h.s_out));
        STEP(hipEventRecord(h.ev_out[b], h.s_out));
    }
#undef STEP
    hipStreamSynchronize(h.s_in);
    hipStreamSynchronize(e->stream);
    hipStreamSynchronize(h.s_out);
    if (rc == 0 && er == hipSuccess && d_clip) {      // once, after the last chunk
        er = hipMemcpyAsync(h_clipped, d_clip, (size_t)S * sizeof *d_clip, hipMemcpyDeviceToHost, e->stream);
        if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    }
    if (rc == 0 && er != hipSuccess) rc = fail(-2, "HIP error: %s", hipGetErrorString(er));
    if (pinL) hipHostUnregister((void*)h_in);
    if (pinR) hipHostUnregister((void*)h_R);
    if (pinO) hipHostUnregister((void*)h_out);
    return rc;
}

int srt_engine_host_range(srt_engine* e, const float* h_L, const float* h_R, size_t n, size_t frames, size_t rows, float* h_out, size_t out_stride,
                          float* h_tail, bool head, unsigned flags, int cli_stems)
{
    if (cli_stems) { DeviceScope ds(e->device); const int rc = cli_check(e, cli_stems); if (rc) return rc; }
    return host_stream(e, h_L, h_R, n, frames, rows, h_out, flags, cli_stems, SrtSeam{out_stride, h_tail, head});
}
const float* srt_engine_coeff_device(const srt_engine* e, int stem) { return e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE; }
int srt_engine_device(const srt_engine* e) { return e->device; }
void* srt_engine_stream(const srt_engine* e) { return (void*)e->stream; }

int srtSeparateHostStreamEx(srt_engine* e, const float* h_L, const float* h_R, size_t n, size_t frames, size_t rows, float* h_out, unsigned flags)
{
    return host_stream(e, h_L, h_R, n, frames, rows, h_out, flags & SRT_HOST_PINNED, 0);      // float buffers by its types: the 16-bit forms are srtSeparateHostStreamIo's
}

int srtSeparateHostStreamIo(srt_engine* e, const void* h_in, const void* h_in2, size_t n, size_t frames, size_t rows, void* h_out, unsigned flags, unsigned long long* h_clipped)
{
    if (flags & ~SRT_HOST_FLAGS) return fail(-1, "srtSeparateHostStreamIo: unknown flag bits");
    return host_stream(e, h_in, h_in2, n, frames, rows, h_out, flags, 0, SrtSeam{0, nullptr, false}, h_clipped);
}

int srtSeparateHostStream(srt_engine* e, const float* h_L, const float* h_R, size_t n, size_t frames, size_t rows, float* h_out)
{
    return srtSeparateHostStreamEx(e, h_L, h_R, n, frames, rows, h_out, 0);
}

int srtCopyTensor(srt_engine* e, const char* name, int stem, int tile, float* h_dst, size_t max_floats)
{
    if (!e || !name || !h_dst) return fail(-1, "srtCopyTensor: null argument");
    DeviceScope ds(e->device);
    if (!name[0]) return fail(-1, "srtCopyTensor: empty tensor name");
    if (!strcmp(name, "wiener_cov")) {                                       // R_j of one iteration [F][4], its weight sums [F], a [1]; tile = 4 * track + iteration
        const int S = e->cfg.n_stems, F = e->cfg.F, trk = tile < 0 ? -1 : tile / 4, it = tile < 0 ? 0 : tile % 4, K = e->last.wiener_tracks;     // (track 0 of a single-signal call: tile = iteration)
        const float* tab = K ? e->bwtabf : e->wtab;
        if (!tab || stem < 0 || stem >= S || it < 1 || it > e->last.wiener_last || trk < 0 || trk >= (K ? K : 1))
            return fail(-1, "srtCopyTensor: wiener_cov needs a stem and 1 <= iteration <= the iterations of the last filtered call (after srtSeparateBatchWiener: tile = 4 * track + iteration)");
        if ((size_t)5 * F + 1 > max_floats) return fail(-1, "srtCopyTensor: destination too small");
        // slots of [SRT_WIENER_MAX_ITERS][S][F]: one (the call's) in wtab, max_tiles (one per track) in the batch tables
        const size_t slots = K ? (size_t)e->cfg.max_tiles : 1, per = (size_t)SRT_WIENER_MAX_ITERS * S * F;
        const size_t o = (size_t)trk * per + (size_t)(it - 1) * S * F + (size_t)stem * F;
        const float* wsum = tab + slots * per * 4;
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipMemcpy(h_dst, tab + o * 4, (size_t)F * 4 * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h_dst + 4 * F, wsum + o, (size_t)F * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h_dst + 5 * F, wsum + slots * per + trk, sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    if (!strcmp(name, "mask_ext")) {                                         // the gains of bins >= F the last inverse transform applied: [rows][2] of one stem
        const size_t rows = (size_t)e->last.ext_rows;
        if (!e->ext || !rows || stem < 0 || stem >= e->cfg.n_stems || tile != 0) return fail(-1, "srtCopyTensor: mask_ext needs a stem, tile 0 and an earlier call with the average mask extension on");
        if (max_floats < 2 * rows) return fail(-1, "srtCopyTensor: destination too small");
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipMemcpy(h_dst, e->ext + (size_t)stem * e->rows_cap * 2, 2 * rows * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    const ForwardRecord& last = e->last;
    if (stem < 0 || stem >= e->cfg.n_stems || tile < 0 || tile >= last.ntiles) return fail(-1, "srtCopyTensor: stem / tile outside the last forward batch");
    const int idx = name[strlen(name) - 1] - '1';
    float* base = nullptr; size_t per = 0; bool derived = false;
    if (!strncmp(name, "conv", 4) && idx >= 0 && idx < 6) { base = e->raw[idx]; per = e->raw_tile[idx]; }
    else if (!strncmp(name, "act", 3) && idx >= 0 && idx < 5) { base = e->raw[idx]; per = e->raw_tile[idx]; derived = true; }
    else if (!strncmp(name, "up", 2) && idx >= 0 && idx < 6) { base = e->up[idx]; per = e->up_tile[idx]; }
    else return fail(-1, "srtCopyTensor: unknown tensor %s", name);
    if (per > max_floats) return fail(-1, "srtCopyTensor: destination too small");
    if (name[0] == 'u' && idx == 5 && ((last.up6_fused >> stem) & 1u)) {     // the fused launch kept the plane in LDS: materialise the tap with the plain up6 kernel
        if (stem < last.up6_s0 || stem >= last.up6_s0 + last.up6_params.nstems) return fail(-1, "srtCopyTensor: up6 of this stem was not stored by the fused up6 + head launch of an earlier stem range");
        if (srt_launch_dec(last.up6_params, e->cfg.impl, e->stream)) return fail(-2, "up6 launch failed");
    }
    const bool halves = e->act16 && !(name[0] == 'u' && idx == 5);           // up6 (the head's input) is always fp32
    const float* src = stem_at(e, base, per, last.ntiles, stem, !halves, tile);     // instance stride = ntiles of the last forward
    struct DeviceTemp { float* p = nullptr; ~DeviceTemp() { if (p) hipFree(p); } } buf;     // the tap's two conversion stages [2][per], freed on every exit
    // raw2..raw6 (and the act taps derived from them) and up1..up5 of a large fp16-storage batch are channel-interleaved by eight (srt_nn5.hip): the tap
    // is returned planar, like every other
    const bool c8 = halves && last.c8 && ((name[0] == 'u') ? idx <= 4 : (idx >= 1 || last.c8_l1));
    const bool halves_in = halves && !c8;
    if (c8 || derived || halves_in) HIPCHK(hipMalloc((void**)&buf.p, 2 * per * sizeof(float)));
    float* const planar = buf.p; float* const tmp = buf.p + per;
    if (c8) {
        const int C = name[0] == 'u' ? DEC_CH[idx][1] : ENC_CH[idx][1];
        if (srt_launch_c8_to_float(src, planar, C, per / C, e->stream)) return fail(-2, "conversion launch failed");
        src = planar;
    }
    if (derived) {
        // "actN" is no longer stored: the next encoder layer applies act(bn(convN)) while staging.  Materialise it for the tap.
        const LayerOff& L = e->lo.down[idx];
        const float* c = e->coeff_all + (size_t)stem * SRT_COEFF_STRIDE;
        if (srt_launch_bn_act(src, halves_in, tmp, c + L.bn + L.cout, c + L.bn, L.cout, per / L.cout, e->cfg.stem_mode[stem] ? SRT_ACT_ELU : SRT_ACT_LEAKY, e->cfg.variant, e->stream)) return fail(-2, "bn-act launch failed");
        src = tmp;
    } else if (halves_in) {
        if (srt_launch_half_to_float(src, tmp, per, e->stream)) return fail(-2, "conversion launch failed");
        src = tmp;
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(h_dst, src, per * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int srtSetTiming(srt_engine* e, int enable)
{
    if (!e) return fail(-1, "null engine");
    DeviceScope ds(e->device);
    for (auto& t : e->tlog) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
    e->tlog.clear();
    e->timing = enable != 0;
    return 0;
}

int srtGetTiming(srt_engine* e, char* names, size_t names_bytes, float* ms, int max_entries)
{
    if (!e || !ms || max_entries < 0) return fail(-1, "srtGetTiming: bad argument");
    DeviceScope ds(e->device);
    HIPCHK(hipStreamSynchronize(e->stream));
    int n = 0; size_t used = 0;
    if (names && names_bytes) names[0] = 0;
    for (auto& t : e->tlog) {
        if (n >= max_entries) break;
        float v = 0; hipEventElapsedTime(&v, t.a, t.b);
        ms[n++] = v;
        if (names && used + t.name.size() + 2 < names_bytes) { memcpy(names + used, t.name.c_str(), t.name.size()); used += t.name.size(); names[used++] = ','; names[used] = 0; }
    }
    return n;
}

// The kernel that ran each timed launch (same order and count as srtGetTiming), ';'-separated, as rocprofv3 prints kernel names:
// the demangled symbol without its return type and argument list, e.g. "srt_dec_wino<4, 16, 1, 0>".  For a split-K layer this is
// the layer kernel (the reduction that follows it is not named).  If the runtime cannot resolve a symbol the launch expression's
// source text is reported instead.
int srtGetTimingKernels(srt_engine* e, char* kernels, size_t kernels_bytes)
{
    if (!e || !kernels || !kernels_bytes) return fail(-1, "srtGetTimingKernels: bad argument");
    DeviceScope ds(e->device);
    kernels[0] = 0;
    size_t used = 0; int n = 0;
    for (auto& t : e->tlog) {
        std::string nm;
        const char* sym = t.kfn ? hipKernelNameRefByPtr(t.kfn, e->stream) : nullptr;
        (void)hipGetLastError();
        if (sym && sym[0]) {
            int st = 0;
            char* dm = abi::__cxa_demangle(sym, nullptr, nullptr, &st);
            nm = (st == 0 && dm) ? dm : sym;
            free(dm);
            if (!nm.compare(0, 5, "void ")) nm.erase(0, 5);
            // cut the argument list: the '(' that closes the name is the first one outside template brackets
            int depth = 0;
            for (size_t i = 0; i < nm.size(); ++i) {
                if (nm[i] == '<') ++depth; else if (nm[i] == '>') --depth;
                else if (nm[i] == '(' && depth == 0) { nm.erase(i); break; }
            }
        } else if (t.ktext) {
            nm = t.ktext;
            if (nm.size() >= 2 && nm.front() == '(' && nm.back() == ')') nm = nm.substr(1, nm.size() - 2);
        } else nm = "?";
        if (used + nm.size() + 2 >= kernels_bytes) break;
        memcpy(kernels + used, nm.c_str(), nm.size()); used += nm.size(); kernels[used++] = ';'; kernels[used] = 0;
        ++n;
    }
    return n;
}
