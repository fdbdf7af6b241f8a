// srt_stream.hip — the reference's real-time streaming surface (include/Spleeter4Stems.h) and its low-latency generalisation, the live
// stream (srtLive*, include/spleeterrt_amd.h), on the GPU engine.  One code path serves both.
//
// A live stream has a network window of T frames, a run every K = hops_per_run hops and a lookahead of L frames.  Host side keeps exactly
// the reference's bookkeeping (input ring, "samples needed" counter, two queued output segments interleaved by 2*n_stems:
// VST/Source/Spleeter4Stems.c:512-582); every completed hop h launches
//   srt_stream_inverse_kernel x S stems : frame h-D's spectrum x its mask row -> inverse FFT -> synthesis window -> 50 % OLA
//   srt_stream_forward_kernel           : asymmetric-window FFT of the current 4096 samples -> spectrum + magnitude row of frame h
// on the hop stream and copies the 1024 x 2S segment back.  At every hop h = K-1 (mod K) the run started K hops ago is joined, the
// magnitude ring is gathered into the window [h-T+1, h] and the U-Nets start on it on the engine's own stream (the reference's task_type2
// threads, Spleeter4Stems.c:135,351-371).  Frame g takes row T-1-(h_r-g) of the run h_r with h_r-g in [L, L+K-1] and is synthesised at
// hop g + D, D = L + 2K.  The plugin's instance (Spleeter4StemsInit) is K = T, L = 0: runs at the T-hop flips, D = 2T, rows 0..T-1.
#include "srt_internal.h"
#include "../../include/spleeterrt_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "../../include/Spleeter4Stems.h"
#undef min   // the header keeps the reference's C macro (Spleeter4Stems.h:10-12) for the plugin; not wanted in this C++ file

// Failure policy (this is the host's real-time audio thread, VST/Source/PluginProcessor.cpp:178-179): never abort(), never a
// CPU path.  The first failure is reported once (stderr + srtLastError()), the instance is marked failed and from then on it
// emits SILENCE with the reference's exact sample accounting, without touching the device again.
static bool stream_fail(const char* where, const char* why)
{
    char buf[400];
    snprintf(buf, sizeof buf, "%s: %s", where, why ? why : srtLastError());
    srt_set_error(-2, "%s", buf);
    fprintf(stderr, "libspleeterrt_amd: %s (no CPU fallback exists; the stream is muted)\n", buf);
    return false;
}
#define HIPTRY(x, where) do { hipError_t _e = (x); if (_e != hipSuccess) { s->failed = true; stream_fail(where, hipGetErrorString(_e)); goto failed; } } while (0)


struct srt_live {
    srt_engine* eng;
    hipStream_t hop, nn;
    hipEvent_t evMag, evNN, evOut;
    int F, T, S, K, L, D;
    long long hops;                      // hops completed (= frame index of the next hop)
    long long runHop, joinedHop;         // end hop of the run in flight / of the last joined run (-1: none yet)
    int runBuf, joinedBuf;               // mask buffer each of them writes / wrote (run r writes buffer r & 1)
    bool nnRunning, failed, ratio;
    float oob[SRT_MAX_STEMS];
    // device: input ring [2][4096], spectrum ring [2][D][SPEC_LD] (frame g at row g mod D), magnitude ring [2][T][F] (frame g at row g mod T),
    // network window [2][T][F], masks [2 buffers][S][2][T][F], overlap [2S][1024], segment [1024][2S]
    float* d_ring; float2* d_spec; float* d_mag; float* d_tmp; float* d_masks; float* d_overlap; float* d_out;
    float *d_awin, *d_swin; float2* d_tw;
    size_t hw;
    // host state, mirrors Spleeter4Stems.h:35-47
    float ring[2][FFTSIZE];
    unsigned inPos, needed;
    float* outq[2]; float* pinned; float* hostq; // two queued segments of OUTPUTSEG*2S floats (pinned for the D2H copy; plain host memory on a failed instance)
    int outCount, outReadOff;
};

namespace {
void asymmetric_window(std::vector<float>& an, std::vector<float>& sy)      // Spleeter4Stems.c:383-401 with k=4096, m=1024, p=1
{
    const int k = FFTSIZE, m = OVPSIZE;
    const double PI = 3.141592653589793;
    an.assign(k, 0.f); sy.assign(k, 0.f);
    int n = ((k - m) << 1) + 2;
    for (int i = 0; i < k - m; ++i) an[i] = (float)pow(0.5 * (1.0 - cos(2.0 * PI * (i + 1.0) / (double)n)), 1.0);
    n = (m << 1) + 2;
    for (int i = k - m; i < k; ++i) an[i] = (float)pow(sqrt(0.5 * (1.0 - cos(2.0 * PI * ((m + i - (k - m)) + 1.0) / (double)n))), 1.0);
    n = m << 1;
    for (int i = k - (m << 1); i < k; ++i) sy[i] = (float)(0.5 * (1.0 - cos(2.0 * PI * (double)(i - (k - (m << 1))) / (double)n))) / an[i];
    for (int i = 0; i < k - SAMPLESHIFT; ++i) sy[i] = sy[i + SAMPLESHIFT];   // pre-shift
    for (int i = 0; i < k; ++i) an[i] *= (1.0 / FFTSIZE) * 0.5f;             // Spleeter4Stems.c:414-416 (double product, float store)
}


float* masks_buf(const srt_live* s, int b) { return s->d_masks + (size_t)b * s->S * 2 * s->hw; }

// the hop kernels' arguments for hop h: frame h is written to spectrum row h mod D and magnitude row h mod T after frame h-D has been
// read from the same spectrum row under row T-1-(h_r-(h-D)) of the last joined run h_r
SrtStreamHop hop_params(const srt_live* s, long long h)
{
    SrtStreamHop p; memset(&p, 0, sizeof p);
    const size_t rowF2 = SRT_SPEC_LD;
    const long long g = h - s->D;
    const int prow = s->joinedHop >= 0 ? s->T - 1 - (int)(s->joinedHop - g) : s->T - 1 - s->L;     // before the first join: zero spectrum, unit masks
    p.ring = s->d_ring; p.inPos = (int)s->inPos;
    p.specRow = s->d_spec + (size_t)(h % s->D) * rowF2; p.specChStride = (size_t)s->D * rowF2;
    p.magRow = s->d_mag + (size_t)(h % s->T) * s->F; p.magChStride = s->hw;
    p.maskRow = masks_buf(s, s->joinedBuf) + (size_t)prow * s->F; p.maskStemStride = 2 * s->hw; p.maskChStride = s->hw;
    p.F = s->F; p.nstems = s->S;
    for (int k = 0; k < s->S; ++k) p.oob[k] = s->oob[k];
    p.overlap = s->d_overlap; p.out = s->d_out;
    p.analysisWnd = s->d_awin; p.synthesisWnd = s->d_swin; p.twiddle = s->d_tw;
    return p;
}

void process_hop(srt_live* s)                                                // LLPAMSProcessNPR, Spleeter4Stems.c:257-381
{
    const size_t seg = (size_t)OUTPUTSEG * 2 * s->S;
    if (s->outCount >= 2) { float* t = s->outq[0]; s->outq[0] = s->outq[1]; s->outq[1] = t; s->outCount = 1; s->outReadOff = 0; }   // the reference overruns its 2-slot queue here (caller passed > 1024 samples without draining); drop the oldest segment instead
    float* dst = s->outq[s->outCount];
    s->outCount++;
    s->needed = OUTPUTSEG;
    if (s->failed) goto failed;
    {
        const long long h = s->hops;
        HIPTRY(hipMemcpyAsync(s->d_ring, s->ring, sizeof s->ring, hipMemcpyHostToDevice, s->hop), "stream hop");
        const SrtStreamHop p = hop_params(s, h);
        if (srt_launch_stream_hop(p, s->hop)) { s->failed = true; stream_fail("stream hop", "kernel launch failed"); goto failed; }
        HIPTRY(hipMemcpyAsync(dst, s->d_out, seg * sizeof(float), hipMemcpyDeviceToHost, s->hop), "stream hop");
        HIPTRY(hipEventRecord(s->evOut, s->hop), "stream hop");
        s->hops = h + 1;
        if (h % s->K == s->K - 1) {
            // join the run started K hops ago (its masks serve the next K hops), then start one on the window [h-T+1, h]
            if (s->nnRunning) {
                HIPTRY(hipStreamWaitEvent(s->hop, s->evNN, 0), "stream join");
                s->joinedHop = s->runHop; s->joinedBuf = s->runBuf;
            }
            const int b = !s->runBuf;                                         // the buffer the joined run's predecessor wrote: its last reader was this hop
            if (srt_launch_live_gather(s->d_mag, s->d_tmp, s->T, s->F, (int)((h + 1) % s->T), s->hop)) { s->failed = true; stream_fail("stream window", "kernel launch failed"); goto failed; }   // replaces the "Prevent race condition" copy (:364-365)
            HIPTRY(hipEventRecord(s->evMag, s->hop), "stream flip");
            HIPTRY(hipStreamWaitEvent(s->nn, s->evMag, 0), "stream flip");
            if (srtForward(s->eng, s->d_tmp, 1, masks_buf(s, b))) { s->failed = true; stream_fail("stream networks", nullptr); goto failed; }
            if (s->ratio && srtRatioMask(s->eng, masks_buf(s, b), 1)) { s->failed = true; stream_fail("stream ratio mask", nullptr); goto failed; }
            HIPTRY(hipEventRecord(s->evNN, s->nn), "stream flip");
            s->nnRunning = true; s->runHop = h; s->runBuf = b;
        }
        // the segment must be in host memory before the callback returns.  With K < T the call waits for its segment only, not for the join it just
        // queued (at K = 1 the run the previous call started would otherwise be on every call's critical path); K = T (the plugin) keeps the
        // whole-stream wait it always had
        if (s->K < s->T) HIPTRY(hipEventSynchronize(s->evOut), "stream hop");
        else HIPTRY(hipStreamSynchronize(s->hop), "stream hop");
        return;
    }
failed:
    memset(dst, 0, seg * sizeof(float));                                      // silence for this hop, same sample accounting
}

// host state only: a failed instance still accounts for samples (and emits silence) through its queue.  NULL: out of host memory.
srt_live* live_new(int F, int T, int S, int K, int L)
{
    srt_live* s = new (std::nothrow) srt_live();
    if (!s) return nullptr;
    memset(s, 0, sizeof *s);
    s->F = F; s->T = T; s->S = S; s->K = K; s->L = L; s->D = L + 2 * K; s->hw = (size_t)F * T;
    s->needed = OUTPUTSEG;
    s->runHop = s->joinedHop = -1;
    s->runBuf = s->joinedBuf = 1;                                             // run 0 writes buffer 0; until it is joined the hops read buffer 1
    s->failed = true;                                                         // until live_init has succeeded
    s->pinned = nullptr;
    const size_t seg = (size_t)OUTPUTSEG * 2 * S;
    s->hostq = (float*)calloc(2 * seg, sizeof(float));
    s->outq[0] = s->hostq; s->outq[1] = s->hostq ? s->hostq + seg : nullptr;
    return s;
}

void live_free(srt_live* s)
{
    if (!s) return;
    if (s->hop) hipStreamSynchronize(s->hop);
    if (s->nn) hipStreamSynchronize(s->nn);
    if (s->eng) srtDestroy(s->eng);
    void* d[] = { s->d_ring, s->d_spec, s->d_mag, s->d_tmp, s->d_masks, s->d_overlap, s->d_out, s->d_awin, s->d_swin, s->d_tw };
    for (void* q : d) if (q) hipFree(q);
    if (s->pinned) hipHostFree(s->pinned);
    free(s->hostq);
    hipEvent_t ev[] = { s->evMag, s->evNN, s->evOut };
    for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
    if (s->hop) hipStreamDestroy(s->hop);
    if (s->nn) hipStreamDestroy(s->nn);
    delete s;
}

// Everything the hops need - engine, weights, buffers, both network graphs, the hop kernels' code - set up on the calling thread.
// 0, or a negative code with the reason reported once (the instance stays muted).  The caller has checked every argument and that a device exists.
int live_init(srt_live* s, const srt_config& cfg, const void* const* coeff, const char* who)
{
    for (int k = 0; k < s->S; ++k) s->oob[k] = cfg.oob_weight[k];
    s->ratio = cfg.ratio_mask != 0;
#define INITTRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) { stream_fail(who, hipGetErrorString(_e)); return -2; } } while (0)
    // non-blocking streams: no implicit ordering against the legacy null stream, so another instance's (another host thread's) synchronous
    // copies and memsets during ITS Init can neither stall this instance's hops nor invalidate the graph capture of this one's pre-warm
    // Priorities: the per-hop stream (one forward + S inverse FFTs the audio callback WAITS for) gets the device's highest priority, the
    // network stream (the U-Nets, joined K hops after they start) the lowest - the reference gives the per-hop iFFT its own thread and joins the
    // network threads every T hops (Spleeter4Stems.c:351-371).  With several plugin instances on one GPU a hop's kernels are then dispatched
    // ahead of every instance's queued network kernels instead of waiting their turn behind them.
    int prLeast = 0, prGreatest = 0;
    INITTRY(hipDeviceGetStreamPriorityRange(&prLeast, &prGreatest));
    INITTRY(hipStreamCreateWithPriority(&s->hop, hipStreamNonBlocking, prGreatest));
    INITTRY(hipStreamCreateWithPriority(&s->nn, hipStreamNonBlocking, prLeast));
    INITTRY(hipEventCreateWithFlags(&s->evMag, hipEventDisableTiming));
    INITTRY(hipEventCreateWithFlags(&s->evNN, hipEventDisableTiming));
    INITTRY(hipEventCreateWithFlags(&s->evOut, hipEventDisableTiming));
    if (srtCreate(&cfg, s->nn, &s->eng)) { s->eng = nullptr; stream_fail(who, nullptr); return -2; }
    for (int k = 0; k < s->S; ++k)
        if (srtSetCoeffHost(s->eng, k, coeff[k])) { stream_fail(who, nullptr); return -2; }
    srtSetGraphMode(s->eng, 1);                           // the U-Nets run on the same buffers every K hops: replay one hipGraph per mask buffer
    const size_t S = s->S, specF = 2 * (size_t)s->D * SRT_SPEC_LD * 2, maskF = 2 * S * 2 * s->hw;
    INITTRY(hipMalloc((void**)&s->d_ring, sizeof s->ring));
    INITTRY(hipMalloc((void**)&s->d_spec, specF * sizeof(float)));
    INITTRY(hipMalloc((void**)&s->d_mag, 2 * s->hw * sizeof(float)));
    INITTRY(hipMalloc((void**)&s->d_tmp, 2 * s->hw * sizeof(float)));
    INITTRY(hipMalloc((void**)&s->d_masks, maskF * sizeof(float)));
    INITTRY(hipMalloc((void**)&s->d_overlap, 2 * S * 1024 * sizeof(float)));
    INITTRY(hipMalloc((void**)&s->d_out, OUTPUTSEG * 2 * S * sizeof(float)));
    INITTRY(hipMalloc((void**)&s->d_awin, FFTSIZE * sizeof(float)));
    INITTRY(hipMalloc((void**)&s->d_swin, FFTSIZE * sizeof(float)));
    INITTRY(hipMalloc((void**)&s->d_tw, FFTSIZE * sizeof(float2)));
    INITTRY(hipMemset(s->d_spec, 0, specF * sizeof(float)));              // zero spectrum for the first D hops (:423-438)
    INITTRY(hipMemset(s->d_mag, 0, 2 * s->hw * sizeof(float)));           // frames before 0 have zero magnitude
    INITTRY(hipMemset(s->d_overlap, 0, 2 * S * 1024 * sizeof(float)));
    // Pre-warm on THIS thread: the split-K workspace allocation and the capture + instantiation of one hipGraph per mask buffer
    // would otherwise happen inside the host's audio callback at the first runs (an allocation and a graph build there risk a dropout).
    INITTRY(hipMemset(s->d_tmp, 0, 2 * s->hw * sizeof(float)));
    INITTRY(hipStreamSynchronize(nullptr));               // the null-stream memsets are done before the two private (non-blocking) streams touch the buffers
    for (int b = 0; b < 2; ++b)
        if (srtPrepareForward(s->eng, s->d_tmp, 1, masks_buf(s, b))) { stream_fail(who, nullptr); return -2; }
    if (s->ratio) {                                       // loads the ratio kernel's code now, not in the first run's hop
        if (srtRatioMask(s->eng, masks_buf(s, 0), 1)) { stream_fail(who, nullptr); return -2; }
        INITTRY(hipStreamSynchronize(s->nn));
    }
    std::vector<float> ones(maskF, 1.0f), an, sy, tw(2 * FFTSIZE);           // masks start at 1.0 (:456-467)
    INITTRY(hipMemcpy(s->d_masks, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice));
    asymmetric_window(an, sy);
    const double w0 = 6.283185307179586476925286766559 / FFTSIZE;
    for (int i = 0; i < FFTSIZE; ++i) { tw[2 * i] = (float)cos(w0 * i); tw[2 * i + 1] = (float)(-sin(w0 * i)); }
    INITTRY(hipMemcpy(s->d_awin, an.data(), FFTSIZE * 4, hipMemcpyHostToDevice));
    INITTRY(hipMemcpy(s->d_swin, sy.data(), FFTSIZE * 4, hipMemcpyHostToDevice));
    INITTRY(hipMemcpy(s->d_tw, tw.data(), 2 * FFTSIZE * 4, hipMemcpyHostToDevice));
    INITTRY(hipHostMalloc((void**)&s->pinned, 2 * OUTPUTSEG * 2 * S * sizeof(float), hipHostMallocDefault));   // pinned queue for the per-hop D2H copy
    INITTRY(hipStreamSynchronize(nullptr));               // masks / windows / twiddles (null-stream copies) are in place before the first hop
    // Pre-warm the per-hop path too: the first launch of the hop kernels loads their code, and eight plugin instances making their first call at
    // the same time queued behind each other for it - the slowest call of every instance was its FIRST one, 7.5 ms (round 6, host/rt_latency.c
    // `worst_hop`).  One hop on silence here, on this thread: zero ring, zero spectrum, unit masks - every buffer it writes stays zero; then one
    // window gather of the zero magnitude ring.
    INITTRY(hipMemsetAsync(s->d_ring, 0, sizeof s->ring, s->hop));
    {
        const SrtStreamHop p = hop_params(s, 0);
        if (srt_launch_stream_hop(p, s->hop)) { stream_fail(who, "hop pre-warm: kernel launch failed"); return -2; }
        if (srt_launch_live_gather(s->d_mag, s->d_tmp, s->T, s->F, 0, s->hop)) { stream_fail(who, "window pre-warm: kernel launch failed"); return -2; }
        INITTRY(hipMemcpyAsync(s->pinned, s->d_out, OUTPUTSEG * 2 * S * sizeof(float), hipMemcpyDeviceToHost, s->hop));
        INITTRY(hipStreamSynchronize(s->hop));
    }
#undef INITTRY
    s->outq[0] = s->pinned; s->outq[1] = s->pinned + OUTPUTSEG * 2 * S;
    s->failed = false;
    return 0;
}

// Spleeter4StemsProcessSamples' accounting (Spleeter4Stems.c:512-582) for 2S planar outputs; returns the samples written to each
int live_process(srt_live* s, const float* inLeft, const float* inRight, int inSampleCount, float* const* components)
{
    const int nc = 2 * s->S;
    int outSampleCount = 0;
    const int maxOut = inSampleCount;
    while (inSampleCount > 0) {                                             // Spleeter4Stems.c:518-537
        const int c = (int)s->needed < inSampleCount ? (int)s->needed : inSampleCount;
        memcpy(&s->ring[0][s->inPos], inLeft, c * sizeof(float));
        memcpy(&s->ring[1][s->inPos], inRight, c * sizeof(float));
        inLeft += c; inRight += c; inSampleCount -= c;
        s->inPos = (s->inPos + c) & (FFTSIZE - 1);
        s->needed -= c;
        if (s->needed == 0) process_hop(s);
    }
    float* io[2 * SRT_MAX_STEMS];
    for (int j = 0; j < nc; ++j) io[j] = components[j];
    while (s->outCount > 0 && outSampleCount < maxOut) {                    // Spleeter4Stems.c:540-581
        const float* src = s->outq[0] + (size_t)s->outReadOff * nc;
        int c = OUTPUTSEG - s->outReadOff;
        if (c > maxOut - outSampleCount) c = maxOut - outSampleCount;
        for (int i = 0; i < c; ++i)
            for (int j = 0; j < nc; ++j) *io[j]++ = *src++;
        outSampleCount += c;
        s->outReadOff += c;
        if (s->outReadOff == OUTPUTSEG) {
            s->outCount--;
            s->outReadOff = 0;
            if (s->outCount > 0) { float* t = s->outq[0]; s->outq[0] = s->outq[1]; s->outq[1] = t; }
        }
    }
    return outSampleCount;
}

int live_latency(int K, int L) { return (L + 2 * K) * OUTPUTSEG + OUTPUTSEG; }

// the plugin surface: VST config (4 stems, ELU, oob 0.25 / 0 / 0.25 / 0.25, Spleeter4Stems.c:444-447), K and L as given
void s4s_init(Spleeter4Stems* msr, int F, int T, void* coeffProvider[4], int K, int L, const char* who)
{
    if (!msr) return;
    SrtSetupLock setup;                                      // (srt_internal.h: set-up paths are serialised process-wide)
    memset(msr, 0, sizeof *msr);
    srt_config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.F = F; cfg.T = T; cfg.n_stems = 4; cfg.variant = SRT_VARIANT_VST; cfg.max_tiles = 1; cfg.impl = SRT_IMPL_MFMA;
    for (int k = 0; k < 4; ++k) { cfg.stem_mode[k] = 1; cfg.oob_weight[k] = k == 1 ? 0.0f : 0.25f; }      // Spleeter4Stems.c:444-447
    const bool args_ok = T >= 1 && K >= 1 && K <= T && L >= 0 && L <= T - K;
    srt_live* s = live_new(F, T, 4, args_ok ? K : (T >= 1 ? T : 1), args_ok ? L : 0);
    if (!s) { stream_fail(who, "out of host memory"); return; }
    msr->impl = s;
    if (!s->hostq) { stream_fail(who, "out of host memory"); return; }
    if (!args_ok) { stream_fail(who, "hopsPerRun must be in 1..timeStep and lookahead in 0..timeStep-hopsPerRun"); return; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { stream_fail(who, "no HIP device (this library has no CPU path)"); return; }
    for (int k = 0; k < 4; ++k) if (!coeffProvider || !coeffProvider[k]) { stream_fail(who, "null coefficient pointer"); return; }
    const void* coeff[4] = { coeffProvider[0], coeffProvider[1], coeffProvider[2], coeffProvider[3] };
    live_init(s, cfg, coeff, who);
}
}  // namespace

void Spleeter4StemsInit(Spleeter4Stems* msr, int F, int T, void* coeffProvider[4])
{
    s4s_init(msr, F, T, coeffProvider, T, 0, "Spleeter4StemsInit");
}

void Spleeter4StemsInitLive(Spleeter4Stems* msr, int F, int T, void* coeffProvider[4], int hopsPerRun, int lookahead)
{
    s4s_init(msr, F, T, coeffProvider, hopsPerRun, lookahead, "Spleeter4StemsInitLive");
}

int Spleeter4StemsLatency(const Spleeter4Stems* msr)
{
    const srt_live* s = msr ? (const srt_live*)msr->impl : nullptr;
    return s ? live_latency(s->K, s->L) : 0;
}

void Spleeter4StemsFree(Spleeter4Stems* msr)
{
    if (!msr || !msr->impl) return;
    live_free((srt_live*)msr->impl);
    msr->impl = nullptr;
}

void Spleeter4StemsProcessSamples(Spleeter4Stems* msr, const float* inLeft, const float* inRight, int inSampleCount, float** components)
{
    srt_live* s = msr ? (srt_live*)msr->impl : nullptr;
    if (!s || !s->outq[0]) return;                                          // Init could not even allocate its host state: nothing is written
    live_process(s, inLeft, inRight, inSampleCount, components);
}

// ---- C API (include/spleeterrt_amd.h)
int srtLiveCreate(const srt_config* cfg, int hops_per_run, int lookahead, const void* const* h_coeff, srt_live** out)
{
    if (!cfg || !h_coeff || !out) return srt_set_error(-1, "%s", "srtLiveCreate: null argument");
    *out = nullptr;
    if (const int rc = srt_check_config(cfg, "srtLiveCreate")) return rc;             // srtCreate's own checks, before any HIP call
    if (cfg->max_tiles != 1) return srt_set_error(-1, "%s", "srtLiveCreate: max_tiles must be 1 (a run is one window)");
    if (hops_per_run < 1 || hops_per_run > cfg->T) return srt_set_error(-1, "%s", "srtLiveCreate: hops_per_run must be in 1..T");
    if (lookahead < 0 || lookahead > cfg->T - hops_per_run) return srt_set_error(-1, "%s", "srtLiveCreate: lookahead must be in 0..T-hops_per_run");
    for (int k = 0; k < cfg->n_stems; ++k)
        if (!h_coeff[k]) return srt_set_error(-1, "%s", "srtLiveCreate: null coefficient blob");
    SrtSetupLock setup;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return srt_set_error(-3, "%s", "srtLiveCreate: no HIP device (this library has no CPU path)");
    srt_live* s = live_new(cfg->F, cfg->T, cfg->n_stems, hops_per_run, lookahead);
    if (!s || !s->hostq) { live_free(s); return srt_set_error(-2, "%s", "srtLiveCreate: out of host memory"); }
    if (const int rc = live_init(s, *cfg, h_coeff, "srtLiveCreate")) { live_free(s); return rc; }
    *out = s;
    return 0;
}

int srtLiveProcess(srt_live* s, const float* inL, const float* inR, int n, float* const* out)
{
    if (!s || n < 0 || (n > 0 && (!inL || !inR || !out))) return srt_set_error(-1, "%s", "srtLiveProcess: bad argument");
    if (n > 0) for (int j = 0; j < 2 * s->S; ++j) if (!out[j]) return srt_set_error(-1, "%s", "srtLiveProcess: null output plane");
    return live_process(s, inL, inR, n, out);
}

int srtLiveLatency(const srt_live* s)
{
    if (!s) return srt_set_error(-1, "%s", "srtLiveLatency: null argument");
    return live_latency(s->K, s->L);
}

void srtLiveDestroy(srt_live* s)
{
    live_free(s);
}
