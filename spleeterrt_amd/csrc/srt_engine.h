// srt_engine.h — private to the engine units (srt_engine.hip, srt_separate.hip, srt_host.hip, srt_batch.hip, srt_taps.hip): the engine struct,
// the weight layout, the graph cache's types and the helpers those units call across files.  No other unit includes it.
#pragma once
#include "srt_internal.h"
#include "srt_checks.h"
#include "srt_rs.h"
#include "../../include/spleeterrt_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <deque>
#include <string>
#include <vector>

static inline int fail(int code, const char* fmt, const char* detail = "") { return srt_set_error(code, fmt, detail); }
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(-2, "HIP error: %s", hipGetErrorString(_e)); } while (0)

static const int ENC_CH[6][2] = { {2, 16}, {16, 32}, {32, 64}, {64, 128}, {128, 256}, {256, 512} };
static const int DEC_CH[6][2] = { {512, 256}, {512, 128}, {256, 64}, {128, 32}, {64, 16}, {32, 1} };

struct LayerOff { size_t w, b, bn; int cin, cout, cp; };
#define SRT_W16CS_U5 ((size_t)(64 / 16) * 15 * 2 * 32 * 8)    // halves per stem of up5's class-stacked fp16 weights
struct Layout { LayerOff down[6], up[6]; size_t head_w, head_b, total; };

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
    // integer PCM forms (SRT_HOST_IN_PCM16 / _PCM24, SRT_HOST_OUT_PCM16 / _PCM24, srt_pcm.hip): one set for every format, allocated only when a call asks for one
    void* d_inq[2]; void* d_outq[2];
    size_t inq_cap, outq_cap;                          // bytes
    unsigned long long* d_clip;                        // [SRT_MAX_STEMS] clipped-sample counters, then the pack's workgroup counts
    // srtSeparateHostWiener's / srtSeparateHostWienerOverlap's store: every piece's spectrum, fp32 masks and mask carry (host_wiener_layout, srt_host.hip), grow-only like the rest
    char* d_wstore; size_t wstore_cap;                 // bytes
    // srtSeparateHostStreamOverlap's mask seam carry [n_stems][2][O][F] (srt_mask_seam_save_kernel), grow-only like the rest
    float* d_mseam; size_t mseam_cap;                  // floats
    // srtSeparateHostStreamRate: a piece's source frames at in_rate (L, then R), its converted planes [pairs * 2][frames] at out_rate, and
    // the rate carry [pairs * 2][2 LO + 1] of the last finalised 44.1 kHz samples; grow-only like the rest, each allocated only when a call converts on that side
    float* d_rin[2]; float* d_rout[2]; float* d_rcarry;
    size_t rin_cap, rout_cap, rcarry_cap;              // floats
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
#define SRT_BATCH_GAIN_FLOATS (SRT_MAX_STEMS * (SRT_MAX_STEMS + 1))      // the largest remix matrix of one track (srtSeparateBatchMix)
// `wiener`, `overlap`, `mask_ext`, `mix_gen`: the call's options (graph_key_opts) - a sequence captured under one record is never replayed under another.  mix_gen is
// the generation of the remix matrix (srtSetMix bumps it; 0 while the mix is off): the matrix travels by value in the captured launch.
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

// The options of ONE separation call.  A public entry point resolves them once - engine_opts(e) where the call runs under the engine's setters, its
// own arguments where it takes options (srtIstftWienerEx, srtSeparateWiener, srtSeparateBatchOverlap / Mix / Wiener / WienerEx) - refuses what it cannot run, and hands the record
// down by reference: nothing below an entry point reads the engine's option fields.  SepOpts{} is every option off (the CLI flows, the filter's mask-free inverses).
struct SepOpts {
    int overlap = 0;                                   // rows two consecutive tiles of one signal share, 0: back-to-back tiles (the reference's cut)
    int mask_ext = SRT_MASK_EXT_CONSTANT;              // the rule for bins >= F
    int wiener = 0;                                    // EM iterations of the multichannel Wiener filter, 0: off
    int n_out = 0;                                     // stem remix: > 0 - the inverse transform writes n_out pairs, pair m the chain of mix[m] over the stems' gains
    float mix[SRT_MAX_STEMS][SRT_MAX_STEMS + 1] = {};  // (a batch's per-track matrices travel beside the record)
    unsigned mix_gen = 0;                              // the engine's count of the srtSetMix calls that switched the mix on: graph key only
    unsigned long long dither_seed = 0;                // SRT_HOST_OUT_DITHER's seed (srtSetDitherSeed): read by the host paths' pack alone
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
    unsigned long long dither_seed = 0;                // srtSetDitherSeed
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
    // ... with the stem remix per track (srtSeparateBatchMix): the device gain table, max_tiles matrices of SRT_BATCH_GAIN_FLOATS, and the same ring
    // of pinned slots; a call uploads ntracks x [n_out][n_stems + 1] beside the track table.  Allocated by the first such call, owned by bwmem as well
    float* bgtab = nullptr; float* bgpin = nullptr;
    // srtSeparateHostStreamRate's converters (built-in filter), one per rate pair, built at the first call that needs it and kept until srtDestroy
    struct RateFilter { int fs_in, fs_out; SrtRsFilter f; };
    std::deque<RateFilter> rate_filters;
    // timing
    bool timing = false; std::vector<TimingEntry> tlog;
};

static const char* const OVERLAP_REFUSED = "%s: not available with overlapped tiles (srtSetOverlap > 0; DESIGN.md 13 lists it as a follow-up): srtSetOverlap(e, 0) first";
static const char* const MIX_REFUSED = "%s: not available with the stem remix on (srtSetMix; DESIGN.md 16 lists it as a follow-up): srtSetMix(e, 0, NULL) first";
static const char* const MASK_EXT_REFUSED = "%s: not available with the average mask extension (srtSetMaskExtension; DESIGN.md 15 lists it as a follow-up): srtSetMaskExtension(e, SRT_MASK_EXT_CONSTANT) first";

// Overlapped network tiles, the one rule (mirrored by spleeterrt_amd/stream.py:overlap_tiles): stride S = T - O, tile j covers rows [jS, jS + T); one tile up
// to T rows, else ceil((rows - O) / S) - every tile then owns a row no earlier tile covers, and the tiles cover all rows.  O = 0: ceil(rows / T).
static inline size_t overlap_tiles(size_t rows, int T, int O) { return rows == 0 ? 0 : rows <= (size_t)T ? 1 : (rows - O + (T - O) - 1) / (T - O); }

// element offset into an activation tensor whose elements are halves (act16) or floats
static inline float* eoff(const srt_engine* e, float* base, size_t elems) { return (float*)((char*)base + elems * (e->act16 ? 2 : 4)); }

// first element of (stem, tile) in an all-stem activation buffer of a forward over ntiles tiles (stem stride = ntiles instances of `per` elements);
// the elements are halves or floats as the engine stores activations (eoff) unless f32 says floats (up6's plane, the fp32 copies, the masks)
static inline float* stem_at(const srt_engine* e, float* buf, size_t per, int ntiles, int stem, bool f32 = false, int tile = 0) { const size_t el = ((size_t)stem * ntiles + tile) * per; return f32 ? buf + el : eoff(e, buf, el); }

// seam: how a tile RANGE of a longer stream joins its neighbours when they run on other devices (srt_multi.hip); {0, nullptr, false} = the whole stream
struct SrtSeam { size_t out_stride; float* h_tail; bool head; };

// per-launch timer of srtSetTiming (defined in srt_engine.hip, beside the kernel note it reads)
struct TimerScope {
    srt_engine* e; size_t idx; bool on;
    TimerScope(srt_engine* e_, const char* name);
    ~TimerScope();
};

// ---- helpers called across the engine units (each defined once, with its comment, in the unit named)
// srt_engine.hip
bool stream_capturing(const srt_engine* e);
bool graph_prepare(srt_engine* e, bool valid, size_t ntiles, int kind, const SrtSwitches& sw, GraphKey* k);
int forward_range(srt_engine* e, const SrtSwitches& sw, const float* d_mag, int ntiles, float* d_masks, int s0, int ns, bool masks16_req = false);
SepOpts engine_opts(const srt_engine* e);
void graph_key_opts(GraphKey* k, const SepOpts& o);
// srt_separate.hip
SrtDspTables tables_of(const srt_engine* e);
int ensure_wiener_ws(srt_engine* e);
int ensure_mask_ext_table(srt_engine* e, const char* who);
int mask_ext_issue(srt_engine* e, const float* masks, int masks16, int nstems, int ntiles, int rows, int ratio, int O, const SrtBatchTrack* tracks = nullptr, int ntracks = 0, const float* seam = nullptr);
bool masks16_wanted(const srt_engine* e, const SrtSwitches& sw, const SepOpts& o);
int separate_run(srt_engine* e, const SepOpts& o, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, float* d_out);
// ... a piece of srtSeparateHostStreamOverlap's plan (srtHostOverlapPieces): `tiles` overlapped tiles over stft_rows spectrum rows, of which the piece owns (inverts)
// the first own_rows; seam: the mask seam carry of the piece before it (nullptr: the stream's first piece)
struct HostOvPiece { size_t tiles, own_rows, stft_rows; const float* seam; };
int separate_piece(srt_engine* e, const SrtSwitches& sw, const SepOpts& o, const float* d_L, const float* d_R, size_t n, size_t frames, const HostOvPiece& pc, float* d_seam, float* d_out);
int cli_time_residual(srt_engine* e, const float* d_L, const float* d_R, size_t n, int stems, float* d_out, size_t len, size_t lo = 0, size_t hi = 0);
int cli_issue(srt_engine* e, const float* d_L, const float* d_R, size_t n, size_t frames, size_t rows, int stems, float* d_out, bool residual_now);
int cli_check(srt_engine* e, int stems);
// ... srtSeparateHostWiener's stages (srt_host.hip drives them): a piece is rows [row0, row0 + rows) of the signal, spectrum [2][rows][SRT_SPEC_LD] and fp32 masks
// [n_stems][ntiles][2][T][F] in the device store
// ... and srtSeparateHostWienerOverlap's (ov / O > 0): `rows` are the rows the piece owns, the first of the stft_rows its spectrum holds and its ntiles overlapped tiles
// cover; seam: the mask carry [n_stems][2][O][F] of the piece before it (nullptr: the first piece), seam_out: its own slot for the next (nullptr: the last piece).
// Without an overlap stft_rows = rows and both are null.
struct HostWienerPiece { float2* spec; float* masks; size_t row0, rows; int ntiles; size_t stft_rows; const float* seam; float* seam_out; };
int host_wiener_check(const srt_engine* e, const srt_wiener_opts* opts, size_t n, SepOpts* o, bool ov);
int host_wiener_ws(srt_engine* e, const SepOpts& o, const char* who);
int host_wiener_analyse(srt_engine* e, const SrtSwitches& sw, const float* d_L, const float* d_R, size_t n, size_t frames, const HostWienerPiece& pc, int O);
SrtWienerParams wiener_geometry(const srt_engine* e, size_t rows);
int host_wiener_stats(srt_engine* e, const SrtWienerParams& w, const HostWienerPiece& pc, int pass, int O);
int host_wiener_finalize(srt_engine* e, const SrtWienerParams& w, int pass);
int host_wiener_render(srt_engine* e, const SrtWienerParams& w, const SepOpts& o, const HostWienerPiece& pc, float* d_out);

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
