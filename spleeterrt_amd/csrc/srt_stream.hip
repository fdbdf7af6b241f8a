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
// An instance of srtLiveCreateEx with a stem remix and / or the average mask extension writes P = n_out pairs instead of S: its hops run
//   srt_live_combine_inverse_kernel x P outputs : frame h-D's spectrum x the chain over all S mask rows under the matrix in force
// and every run is followed, on the network stream, by the extension's table for the K rows it serves.
// An instance of srtLiveCreateWiener with iterations > 0 keeps a spectrum ring of max(D, T) rows; at a run's launch the window's spectrum rows are
// gathered beside the magnitudes, the run is followed by the offline filter's statistics launches over that window into its table set, and the hops run
//   srt_live_wiener_inverse_kernel x P outputs : the filter's chain for every stem from the joined run's masks and tables, folded into the inverse's prologue.
#include "srt_internal.h"
#include "srt_rs.h"
#include "srt_checks.h"
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
#define SRT_LIVE_MAX_BLOCK 65536      // largest slice of a rate instance's call (max_block)
#define HIPTRY(x, where) do { hipError_t _e = (x); if (_e != hipSuccess) { s->failed = true; stream_fail(where, hipGetErrorString(_e)); goto failed; } } while (0)


struct srt_live {
    SrtMem mem;                          // every device and pinned buffer below
    srt_engine* eng;
    hipStream_t hop, nn;
    hipEvent_t evMag, evNN, evOut;
    int F, T, S, K, L, D;
    long long hops;                      // hops completed (= frame index of the next hop)
    long long runHop, joinedHop;         // end hop of the run in flight / of the last joined run (-1: none yet)
    int runBuf, joinedBuf;               // mask buffer each of them writes / wrote (run r writes buffer r & 1)
    bool nnRunning, failed, ratio;
    float oob[SRT_MAX_STEMS];
    // srtLiveCreateEx.  P: stereo pairs a call writes (nOut while the mix is on, else S); combine: the hops run the combining inverse (the
    // mix and / or the average extension; off: exactly the launches of srtLiveCreate).  G: the matrix in force, by value into every hop's launch (mix off
    // with the extension: the S x S identity).  d_ext: the extension's table [2 buffers][S][K][2], buffer b written by the run that writes mask buffer b
    int P, nOut;
    bool combine, ext;
    float G[SRT_MAX_STEMS][SRT_MAX_STEMS + 1];
    float* d_ext;
    // srtLiveCreateWiener.  W: the filter's iterations, 0: off (then nothing below exists and every launch is srtLiveCreateEx's).  R: rows of the
    // spectrum ring, D without the filter, max(D, T) with it (the ring then holds a whole network window).  d_wspec: the window of the run launched last, gathered
    // [2][T][SPEC_LD]; d_wslab: the statistics kernels' partial sums; d_wtab: the table sets [2 buffers][wtabF], buffer b written by the run that writes mask buffer b
    int W, R;
    float2* d_wspec; float* d_wslab; float* d_wtab;
    size_t wtabF;
    // device: input ring [2][4096], spectrum ring [2][R][SPEC_LD] (frame g at row g mod R; R = D unless the filter is on), magnitude ring [2][T][F] (frame g at row g mod T),
    // network window [2][T][F], masks [2 buffers][S][2][T][F], overlap [2P][1024], segment [1024][2P]
    float* d_ring; float2* d_spec; float* d_mag; float* d_tmp; float* d_masks; float* d_overlap; float* d_out;
    float *d_awin, *d_swin; float2* d_tw;
    size_t hw;
    // host state, mirrors Spleeter4Stems.h:35-47
    float ring[2][FFTSIZE];
    unsigned inPos, needed;
    float* outq[2]; float* pinned; float* hostq; // two queued segments of OUTPUTSEG*2P floats (pinned for the D2H copy; plain host memory on a failed instance)
    int outCount, outReadOff;
    // rate instance (srtLiveCreateRate): n samples out for n in at the host's rate fs, one constant delay A.  fs != 44100: the block
    // goes H2D into d_blk, the input-side converter (ring d_hin [capIn][2] of host-rate history) writes the new 44.1 kHz frames into d_ring, every hop's
    // segment lands in the stem ring d_sring [capS][2P] (hop h at slot h mod capS/1024), the output-side converter writes the call's n frames of
    // all 2P planes into d_planes [2P][n], one D2H brings them to pinOut.  fs == 44100: no converter; the host ring and a pinned queue of nq segments.
    bool rate;
    int fs, maxBlock, A, nq;
    long long nHost, c44;                // host samples received / 44.1 kHz frames written to d_ring
    SrtRsFilter fin, fout;
    int Bin, Bout, capIn, capS;
    size_t ldsIn, ldsOut;
    float *d_blk, *d_hin, *d_sring, *d_planes, *pinIn, *pinOut;
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

// the hop kernels' arguments for hop h: frame h is written to spectrum row h mod R (R = D without the filter) and magnitude row h mod T after frame h-D
// has been read - without the filter from the same spectrum row - under row T-1-(h_r-(h-D)) of the last joined run h_r
SrtStreamHop hop_params(const srt_live* s, long long h)
{
    SrtStreamHop p; memset(&p, 0, sizeof p);
    const size_t rowF2 = SRT_SPEC_LD;
    const long long g = h - s->D;
    const int prow = s->joinedHop >= 0 ? s->T - 1 - (int)(s->joinedHop - g) : s->T - 1 - s->L;     // before the first join: zero spectrum, unit masks
    p.ring = s->d_ring; p.inPos = (int)s->inPos;
    p.specRow = s->d_spec + (size_t)(h % s->R) * rowF2; p.specChStride = (size_t)s->R * rowF2;
    p.magRow = s->d_mag + (size_t)(h % s->T) * s->F; p.magChStride = s->hw;
    p.maskRow = masks_buf(s, s->joinedBuf) + (size_t)prow * s->F; p.maskStemStride = 2 * s->hw; p.maskChStride = s->hw;
    p.F = s->F; p.nstems = s->S;
    for (int k = 0; k < s->S; ++k) p.oob[k] = s->oob[k];
    p.overlap = s->d_overlap; p.out = s->d_out;
    p.analysisWnd = s->d_awin; p.synthesisWnd = s->d_swin; p.twiddle = s->d_tw;
    return p;
}

// the combining inverse's arguments for the same hop: frame h-D under the matrix in force now; the extension's row f = prow - (T-L-K) of the joined run's table
SrtLiveCombineHop combine_params(const srt_live* s, const SrtStreamHop& p, long long h)
{
    SrtLiveCombineHop q; memset(&q, 0, sizeof q);
    const long long g = h - s->D;
    const int f = s->joinedHop >= 0 ? s->K - 1 - (int)(s->joinedHop - g - s->L) : s->K - 1;     // before the first join: a row of the initial table (1.0)
    q.specRow = p.specRow; q.specChStride = p.specChStride;
    q.maskRow = p.maskRow; q.maskStemStride = p.maskStemStride; q.maskChStride = p.maskChStride;
    q.F = s->F; q.nstems = s->S; q.n_out = s->P;
    for (int k = 0; k < s->S; ++k) q.oob[k] = s->oob[k];
    if (s->ext) { q.ext = s->d_ext + ((size_t)s->joinedBuf * s->S * s->K + f) * 2; q.extStemStride = (size_t)s->K * 2; }
    memcpy(q.gain, s->G, sizeof q.gain);
    q.overlap = s->d_overlap; q.out = p.out;
    q.synthesisWnd = s->d_swin; q.twiddle = s->d_tw;
    return q;
}

// the statistics launches' arguments for the run that writes mask buffer b (a filter instance): srtIstftWiener's on (d_wspec, T rows, that buffer's masks) - one tile,
// wiener_issue's chunk rule on rows = T - with the instance's own slab and table set b in the engine's table layout (R [iters][S][F][4], weight sums [iters][S][F], a)
SrtWienerParams wiener_params(const srt_live* s, int b)
{
    const int S = s->S, F = s->F, T = s->T;
    SrtWienerParams w; memset(&w, 0, sizeof w);
    w.spec = s->d_wspec; w.spec_ch_stride = (size_t)T * SRT_SPEC_LD;
    w.rows = T; w.masks = masks_buf(s, b); w.nstems = S; w.ntiles = 1; w.T = T; w.F = F;
    int nch = (T + 15) / 16; if (nch > SRT_WIENER_MAX_CHUNKS) nch = SRT_WIENER_MAX_CHUNKS;
    w.rpc = (T + nch - 1) / nch; w.nchunks = (T + w.rpc - 1) / w.rpc;
    w.slab = s->d_wslab; w.slab_max = s->d_wslab + (size_t)w.nchunks * S * 4 * F;
    w.rtab = s->d_wtab + (size_t)b * s->wtabF; w.wsum = w.rtab + (size_t)SRT_WIENER_MAX_ITERS * S * F * 4; w.scal = w.wsum + (size_t)SRT_WIENER_MAX_ITERS * S * F;
    return w;
}
size_t wiener_slab_floats(int T, int S, int F)
{
    int nch = (T + 15) / 16; if (nch > SRT_WIENER_MAX_CHUNKS) nch = SRT_WIENER_MAX_CHUNKS;
    return (size_t)nch * S * 4 * F + (size_t)nch * SRT_WIENER_BINBLK;
}

// the filtering inverse's arguments for hop h: frame h-D at ring row (h-D) mod R (rows of frames before 0 are still zero), its mask row and extension row as the
// combining inverse takes them, the joined run's table set
SrtLiveWienerHop wiener_hop_params(const srt_live* s, const SrtStreamHop& p, long long h)
{
    SrtLiveWienerHop q; memset(&q, 0, sizeof q);
    const long long g = h - s->D;
    const int f = s->joinedHop >= 0 ? s->K - 1 - (int)(s->joinedHop - g - s->L) : s->K - 1;
    const SrtWienerParams w = wiener_params(s, s->joinedBuf);
    q.specRow = s->d_spec + (size_t)(((g % s->R) + s->R) % s->R) * SRT_SPEC_LD; q.specChStride = p.specChStride;
    q.maskRow = p.maskRow; q.maskStemStride = p.maskStemStride; q.maskChStride = p.maskChStride;
    q.F = s->F; q.nstems = s->S; q.n_out = s->P; q.iters = s->W;
    q.rtab = reinterpret_cast<const float4*>(w.rtab); q.scal = w.scal;
    for (int k = 0; k < s->S; ++k) q.oob[k] = s->oob[k];
    if (s->ext) { q.ext = s->d_ext + ((size_t)s->joinedBuf * s->S * s->K + f) * 2; q.extStemStride = (size_t)s->K * 2; }
    memcpy(q.gain, s->G, sizeof q.gain);
    q.overlap = s->d_overlap; q.out = p.out;
    q.synthesisWnd = s->d_swin; q.twiddle = s->d_tw;
    return q;
}

// one hop's kernels: the inverse of frame h-D (one workgroup per output pair) and the forward transform of frame h.  0, or -1: launch failed
int launch_hop(const srt_live* s, const SrtStreamHop& p, long long h)
{
    if (s->W) return srt_launch_live_wiener_hop(wiener_hop_params(s, p, h), p, s->hop);
    if (!s->combine) return srt_launch_stream_hop(p, s->hop);
    return srt_launch_live_combine_hop(combine_params(s, p, h), p, s->hop);
}

// the R tables of the run that has just been queued into mask buffer b, on the network stream behind it: srtIstftWiener's launches over the gathered window
int launch_wiener_tables(const srt_live* s, int b)
{
    const SrtWienerParams w = wiener_params(s, b);
    for (int pass = 1; pass <= s->W; ++pass)
        if (srt_launch_wiener_stats(w, pass, s->nn) || srt_launch_wiener_finalize(w, pass, s->nn)) return -1;
    return 0;
}

// the average extension's table for the run that has just been queued into mask buffer b: srt_launch_mask_ext over the K rows T-L-K .. T-L-1 the run serves
// (the masks as the hops read them: after srtRatioMask, so no ratio here), on the network stream behind the run
int launch_ext_table(const srt_live* s, int b)
{
    SrtMaskExtParams m; memset(&m, 0, sizeof m);
    m.masks = masks_buf(s, b) + (size_t)(s->T - s->L - s->K) * s->F;
    m.nstems = s->S; m.ntiles = 1; m.T = s->T; m.F = s->F; m.rows = s->K;
    m.ext = s->d_ext + (size_t)b * s->S * s->K * 2; m.ext_stem = (size_t)s->K * 2;
    return srt_launch_mask_ext(m, s->nn);
}

// At every hop h = K-1 (mod K): join the run started K hops ago (its masks serve the next K hops), then start one on the window [h-T+1, h].
// false: a device call failed (reported, the instance is muted)
#define HIPOK(x, where) do { hipError_t _e = (x); if (_e != hipSuccess) { s->failed = true; stream_fail(where, hipGetErrorString(_e)); return false; } } while (0)
bool hop_schedule(srt_live* s, long long h)
{
    if (h % s->K != s->K - 1) return true;
    if (s->nnRunning) {
        HIPOK(hipStreamWaitEvent(s->hop, s->evNN, 0), "stream join");
        s->joinedHop = s->runHop; s->joinedBuf = s->runBuf;
    }
    const int b = !s->runBuf;                                             // the buffer the joined run's predecessor wrote: its last reader was this hop
    if (srt_launch_live_gather(s->d_mag, s->d_tmp, s->T, s->F, (int)((h + 1) % s->T), s->hop)) { s->failed = true; return stream_fail("stream window", "kernel launch failed"); }   // replaces the "Prevent race condition" copy (:364-365)
    // the filter's window: the spectrum rows of frames h-T+1 .. h, oldest first (frames before 0: ring rows nothing has written yet, zero).  One buffer: its last
    // reader, the previous run's statistics, has been joined above
    if (s->W && srt_launch_live_spec_gather(s->d_spec, s->d_wspec, s->T, s->R, (int)((((h + 1 - s->T) % s->R) + s->R) % s->R), s->hop)) { s->failed = true; return stream_fail("stream filter window", "kernel launch failed"); }
    HIPOK(hipEventRecord(s->evMag, s->hop), "stream flip");
    HIPOK(hipStreamWaitEvent(s->nn, s->evMag, 0), "stream flip");
    if (srtForward(s->eng, s->d_tmp, 1, masks_buf(s, b))) { s->failed = true; return stream_fail("stream networks", nullptr); }
    if (s->ratio && srtRatioMask(s->eng, masks_buf(s, b), 1)) { s->failed = true; return stream_fail("stream ratio mask", nullptr); }
    if (s->ext && launch_ext_table(s, b)) { s->failed = true; return stream_fail("stream mask extension", "kernel launch failed"); }
    if (s->W && launch_wiener_tables(s, b)) { s->failed = true; return stream_fail("stream filter statistics", "kernel launch failed"); }
    HIPOK(hipEventRecord(s->evNN, s->nn), "stream flip");
    s->nnRunning = true; s->runHop = h; s->runBuf = b;
    return true;
}

void process_hop(srt_live* s)                                                // LLPAMSProcessNPR, Spleeter4Stems.c:257-381
{
    const size_t seg = (size_t)OUTPUTSEG * 2 * s->P;
    float* dst;
    if (s->rate) dst = s->outq[0] + (size_t)(s->hops % s->nq) * seg;        // a 44.1 kHz rate instance: hop h in slot h mod nq of its queue (rate_slice_44100)
    else {
        if (s->outCount >= 2) { float* t = s->outq[0]; s->outq[0] = s->outq[1]; s->outq[1] = t; s->outCount = 1; s->outReadOff = 0; }   // the reference overruns its 2-slot queue here (caller passed > 1024 samples without draining); drop the oldest segment instead
        dst = s->outq[s->outCount];
        s->outCount++;
    }
    s->needed = OUTPUTSEG;
    if (s->failed) goto failed;
    {
        const long long h = s->hops;
        HIPTRY(hipMemcpyAsync(s->d_ring, s->ring, sizeof s->ring, hipMemcpyHostToDevice, s->hop), "stream hop");
        const SrtStreamHop p = hop_params(s, h);
        if (launch_hop(s, p, h)) { s->failed = true; stream_fail("stream hop", "kernel launch failed"); goto failed; }
        HIPTRY(hipMemcpyAsync(dst, s->d_out, seg * sizeof(float), hipMemcpyDeviceToHost, s->hop), "stream hop");
        HIPTRY(hipEventRecord(s->evOut, s->hop), "stream hop");
        s->hops = h + 1;
        if (!hop_schedule(s, h)) goto failed;
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
srt_live* live_new(int F, int T, int S, int K, int L, int P)
{
    srt_live* s = new (std::nothrow) srt_live();           // value-initialised: every field zero
    if (!s) return nullptr;
    s->F = F; s->T = T; s->S = S; s->K = K; s->L = L; s->D = L + 2 * K; s->hw = (size_t)F * T;
    s->R = s->D;
    s->P = P;
    s->needed = OUTPUTSEG;
    s->nq = 2;
    s->runHop = s->joinedHop = -1;
    s->runBuf = s->joinedBuf = 1;                                             // run 0 writes buffer 0; until it is joined the hops read buffer 1
    s->failed = true;                                                         // until live_init has succeeded
    const size_t seg = (size_t)OUTPUTSEG * 2 * P;
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
    s->mem.clear();
    srt_rs_filter_free(&s->fin);
    srt_rs_filter_free(&s->fout);
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
    const size_t S = s->S, P = s->P, specF = 2 * (size_t)s->R * SRT_SPEC_LD * 2, maskF = 2 * S * 2 * s->hw;
    INITTRY(s->mem.alloc(&s->d_ring, sizeof s->ring));
    INITTRY(s->mem.alloc(&s->d_spec, specF * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_mag, 2 * s->hw * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_tmp, 2 * s->hw * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_masks, maskF * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_overlap, 2 * P * 1024 * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_out, OUTPUTSEG * 2 * P * sizeof(float)));
    if (s->ext) INITTRY(s->mem.alloc(&s->d_ext, 2 * S * s->K * 2 * sizeof(float)));
    if (s->W) {
        s->wtabF = (size_t)SRT_WIENER_MAX_ITERS * S * s->F * 5 + 4;
        INITTRY(s->mem.alloc(&s->d_wspec, 2 * (size_t)s->T * SRT_SPEC_LD * sizeof(float2)));
        INITTRY(s->mem.alloc(&s->d_wslab, wiener_slab_floats(s->T, s->S, s->F) * sizeof(float)));
        INITTRY(s->mem.alloc(&s->d_wtab, 2 * s->wtabF * sizeof(float)));
        INITTRY(hipMemset(s->d_wspec, 0, 2 * (size_t)s->T * SRT_SPEC_LD * sizeof(float2)));
    }
    INITTRY(s->mem.alloc(&s->d_awin, FFTSIZE * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_swin, FFTSIZE * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_tw, FFTSIZE * sizeof(float2)));
    INITTRY(hipMemset(s->d_spec, 0, specF * sizeof(float)));              // zero spectrum for the first D hops (:423-438)
    INITTRY(hipMemset(s->d_mag, 0, 2 * s->hw * sizeof(float)));           // frames before 0 have zero magnitude
    INITTRY(hipMemset(s->d_overlap, 0, 2 * P * 1024 * sizeof(float)));
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
    INITTRY(s->mem.alloc(&s->pinned, s->nq * OUTPUTSEG * 2 * P * sizeof(float), true));   // pinned queue for the per-hop D2H copy
    if (s->ext) {
        INITTRY(hipStreamSynchronize(nullptr));           // the unit masks are in place
        // the table launch loads its kernel's code now, on unit masks (every mean is exactly 1.0); then both buffers start at 1.0 as the masks do
        if (launch_ext_table(s, 0)) { stream_fail(who, "mask extension pre-warm: kernel launch failed"); return -2; }
        INITTRY(hipStreamSynchronize(s->nn));
        const std::vector<float> one(2 * S * s->K * 2, 1.0f);
        INITTRY(hipMemcpy(s->d_ext, one.data(), one.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    INITTRY(hipStreamSynchronize(nullptr));               // masks / windows / twiddles (null-stream copies) are in place before the first hop
    if (s->W) {
        // the filter's per-run launches load their code now: the window gather of the zero spectrum ring, then every statistics pass on it under the unit masks.
        // Then both table sets start as the definition has them before the first join: R = 0, a = 1 (zero spectra only are synthesised until then)
        if (srt_launch_live_spec_gather(s->d_spec, s->d_wspec, s->T, s->R, 0, s->hop)) { stream_fail(who, "filter window pre-warm: kernel launch failed"); return -2; }
        INITTRY(hipStreamSynchronize(s->hop));
        if (launch_wiener_tables(s, 0)) { stream_fail(who, "filter statistics pre-warm: kernel launch failed"); return -2; }
        INITTRY(hipStreamSynchronize(s->nn));
        INITTRY(hipMemset(s->d_wtab, 0, 2 * s->wtabF * sizeof(float)));
        const float one = 1.0f;
        for (int b = 0; b < 2; ++b) INITTRY(hipMemcpy(wiener_params(s, b).scal, &one, sizeof one, hipMemcpyHostToDevice));
        INITTRY(hipStreamSynchronize(nullptr));
    }
    // Pre-warm the per-hop path too: the first launch of the hop kernels loads their code, and eight plugin instances making their first call at
    // the same time queued behind each other for it - the slowest call of every instance was its FIRST one, 7.5 ms (round 6, host/rt_latency.c
    // `worst_hop`).  One hop on silence here, on this thread: zero ring, zero spectrum, unit masks - every buffer it writes stays zero; then one
    // window gather of the zero magnitude ring.
    INITTRY(hipMemsetAsync(s->d_ring, 0, sizeof s->ring, s->hop));
    {
        const SrtStreamHop p = hop_params(s, 0);
        if (launch_hop(s, p, 0)) { stream_fail(who, "hop pre-warm: kernel launch failed"); return -2; }
        if (srt_launch_live_gather(s->d_mag, s->d_tmp, s->T, s->F, 0, s->hop)) { stream_fail(who, "window pre-warm: kernel launch failed"); return -2; }
        INITTRY(hipMemcpyAsync(s->pinned, s->d_out, OUTPUTSEG * 2 * P * sizeof(float), hipMemcpyDeviceToHost, s->hop));
        INITTRY(hipStreamSynchronize(s->hop));
    }
#undef INITTRY
    s->outq[0] = s->pinned; s->outq[1] = s->pinned + OUTPUTSEG * 2 * P;
    s->failed = false;
    return 0;
}

int live_process_rate(srt_live* s, const float* inL, const float* inR, int n, float* const* out);      // rate instances, below

// Spleeter4StemsProcessSamples' accounting (Spleeter4Stems.c:512-582) for 2P planar outputs; returns the samples written to each
int live_process(srt_live* s, const float* inLeft, const float* inRight, int inSampleCount, float* const* components)
{
    if (s->rate) return live_process_rate(s, inLeft, inRight, inSampleCount, components);
    const int nc = 2 * s->P;
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

// ---- rate instances (srtLiveCreateRate)
long long fdiv_ll(long long a, long long b) { long long q = a / b; if (a - q * b < 0) --q; return q; }      // floor(a / b), b > 0
long long cdiv_ll(long long a, long long b) { return -fdiv_ll(-a, b); }

// The smallest delay A (host samples) that is causal for every call size.  P / Q = fs / 44100 reduced; H1, H2: horizons of the fs -> 44.1 k and the
// 44.1 k -> fs converter (0, 0 at fs = 44100).  Hop h + 1 is complete once N_h = floor((1024 h + 1023) P / Q) + H1 + 1 host samples have arrived; the
// first output sample that needs it is m_h = A + ceil((1024 h - Dl - H2) P / Q), Dl = (D + 1) * 1024, and m_h + 1 >= N_h must hold for every h >= 0.
// The difference is periodic in h with period Q, so A = H1 + max over one period of floor((1024 h + 1023) P / Q) - ceil((1024 h - Dl - H2) P / Q),
// which is H1 + floor((1023 + Dl + H2) P / Q) whenever Q is odd (then some h makes the second term an integer).
int rate_latency(long long P, long long Q, int H1, int H2, int D)
{
    const long long Dl = (long long)(D + 1) * OUTPUTSEG;
    long long best = 0;
    for (long long h = 0; h < Q; ++h) {
        const long long v = fdiv_ll((OUTPUTSEG * h + OUTPUTSEG - 1) * P, Q) - cdiv_ll((OUTPUTSEG * h - Dl - H2) * P, Q);
        if (h == 0 || v > best) best = v;
    }
    return (int)(H1 + best);
}

// geometry of both converters of a rate instance (the built-in filter) and its latency; no HIP call.  0, or -1 with the error set
int rate_geometry(int fs, int K, int L, const char* who, SrtRsGeom* gin, SrtRsGeom* gout, int* A)
{
    if (fs == 44100) { *A = rate_latency(1, 1, 0, 0, L + 2 * K); return 0; }
    if (const int rc = srt_rs_geometry(fs, 44100, false, 0, 0, who, gin)) return rc;
    if (const int rc = srt_rs_geometry(44100, fs, false, 0, 0, who, gout)) return rc;
    *A = rate_latency(gin->P, gin->Q, srt_rs_horizon(*gin), srt_rs_horizon(*gout), L + 2 * K);
    return 0;
}

// allocation, filter banks and the pre-warm of the two converter kernels, after live_init
int live_rate_init(srt_live* s, const SrtRsGeom& gin, const SrtRsGeom& gout, const char* who)
{
    if (s->fs == 44100) return 0;
#define INITTRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) { s->failed = true; stream_fail(who, hipGetErrorString(_e)); return -2; } } while (0)
    const int nc = 2 * s->P;
    s->failed = true;                                                          // until everything below has succeeded
    s->Bin = srt_rsstream_block(gin, &s->ldsIn);
    s->Bout = srt_rsstream_block(gout, &s->ldsOut);
    if (!s->Bin || !s->Bout) { stream_fail(who, "filter too long for this sample rate"); return -2; }
    if (srt_rs_filter_create(gin, nullptr, 0, s->hop, who, &s->fin) || srt_rs_filter_create(gout, nullptr, 0, s->hop, who, &s->fout)) { stream_fail(who, nullptr); return -2; }
    s->capIn = s->maxBlock + 2 * gin.LO + 1;
    // stem ring: the frames a call's output windows span (max_block host samples of 44.1 kHz frames + both filter halves) plus the hops that may
    // already be written ahead of the newest window (one hop of accounting, one of slack), rounded up to whole segments
    const long long span = cdiv_ll((long long)s->maxBlock * gin.Q, gin.P) + 2 * gout.LO + srt_rs_horizon(gout) + 3 * OUTPUTSEG + 16;
    s->capS = (int)(cdiv_ll(span, OUTPUTSEG) * OUTPUTSEG);
    INITTRY(s->mem.alloc(&s->d_blk, 2 * (size_t)s->maxBlock * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_hin, 2 * (size_t)s->capIn * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_sring, (size_t)s->capS * nc * sizeof(float)));
    INITTRY(s->mem.alloc(&s->d_planes, (size_t)nc * s->maxBlock * sizeof(float)));
    INITTRY(s->mem.alloc(&s->pinIn, 2 * (size_t)s->maxBlock * sizeof(float), true));
    INITTRY(s->mem.alloc(&s->pinOut, (size_t)nc * s->maxBlock * sizeof(float), true));
    INITTRY(hipMemsetAsync(s->d_blk, 0, 2 * (size_t)s->maxBlock * sizeof(float), s->hop));
    INITTRY(hipMemsetAsync(s->d_hin, 0, 2 * (size_t)s->capIn * sizeof(float), s->hop));          // zero weights must meet finite values (padded taps)
    INITTRY(hipMemsetAsync(s->d_sring, 0, (size_t)s->capS * nc * sizeof(float), s->hop));
    INITTRY(hipMemsetAsync(s->d_ring, 0, sizeof s->ring, s->hop));
    // pre-warm: one launch of each converter kernel on silence (loads their code on this thread); the state stays as created - the input side appends
    // one zero frame at slot 0 and writes one zero frame into d_ring, the output side writes one zero into d_planes
    {
        SrtRsStreamArgs a; memset(&a, 0, sizeof a);
        a.ring = s->d_hin; a.cap = s->capIn; a.C = 2; a.in = s->d_blk; a.inStride = 1; a.have = 0; a.n = 1; a.append = 1; a.end = 1;
        a.out0 = 0; a.nOut = 1; a.out = s->d_ring; a.outStride = FFTSIZE; a.outPos = 0; a.outMask = FFTSIZE - 1; a.B = s->Bin;
        if (srt_rsstream_launch(s->fin, a, s->ldsIn, s->hop)) { stream_fail(who, "converter pre-warm: kernel launch failed"); return -2; }
        memset(&a, 0, sizeof a);
        a.ring = s->d_sring; a.cap = s->capS; a.C = nc; a.out0 = 0; a.nOut = 1; a.out = s->d_planes; a.outStride = 1; a.outMask = 0x7fffffff; a.B = s->Bout;
        if (srt_rsstream_launch(s->fout, a, s->ldsOut, s->hop)) { stream_fail(who, "converter pre-warm: kernel launch failed"); return -2; }
        INITTRY(hipMemcpyAsync(s->pinOut, s->d_planes, nc * sizeof(float), hipMemcpyDeviceToHost, s->hop));
        INITTRY(hipStreamSynchronize(s->hop));
    }
#undef INITTRY
    s->failed = false;
    return 0;
}

// the hop that the 44.1 kHz frames in d_ring complete: hop kernels (segment into the stem ring), then the run / join schedule.  false: failed
bool rate_hop(srt_live* s)
{
    const long long h = s->hops;
    SrtStreamHop p = hop_params(s, h);
    p.out = s->d_sring + (size_t)(h % (s->capS / OUTPUTSEG)) * OUTPUTSEG * 2 * s->P;
    if (launch_hop(s, p, h)) { s->failed = true; return stream_fail("stream hop", "kernel launch failed"); }
    s->hops = h + 1;
    return hop_schedule(s, h);
}

// one call of n <= max_block samples at fs != 44100: one H2D, converter -> hops -> converter, one D2H, one wait.  false: failed (the caller emits silence)
bool rate_slice(srt_live* s, const float* inL, const float* inR, int n, float* const* planes)
{
    const int nc = 2 * s->P;
    memcpy(s->pinIn, inL, n * sizeof(float));
    memcpy(s->pinIn + n, inR, n * sizeof(float));
    HIPOK(hipMemcpyAsync(s->d_blk, s->pinIn, 2 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, s->hop), "stream block");
    const long long cNew = srt_rs_computable(s->fin.g, s->nHost + n);
    long long j = s->c44;
    bool first = true;
    for (;;) {
        // d_ring holds one 4096-sample frame: the frames of hop h + 1 may only be written after hop h's kernels have read it, so the input side is
        // launched once per hop the call completes and once for the frames after the last one (stream order does the rest)
        const long long boundary = (s->hops + 1) * OUTPUTSEG, e = cNew < boundary ? cNew : boundary;
        if (first || e > j) {
            SrtRsStreamArgs a; memset(&a, 0, sizeof a);
            a.ring = s->d_hin; a.cap = s->capIn; a.C = 2;
            a.in = s->d_blk; a.inStride = n; a.have = s->nHost; a.n = n; a.append = first; a.end = s->nHost + n;
            a.out0 = j; a.nOut = (int)(e - j);
            a.out = s->d_ring; a.outStride = FFTSIZE; a.outPos = (int)(j & (FFTSIZE - 1)); a.outMask = FFTSIZE - 1;
            a.B = s->Bin;
            if (srt_rsstream_launch(s->fin, a, s->ldsIn, s->hop)) { s->failed = true; return stream_fail("stream converter", "kernel launch failed"); }
            first = false;
        }
        j = e;
        s->inPos = (unsigned)(j & (FFTSIZE - 1));
        if (j < boundary) break;
        if (!rate_hop(s)) return false;
    }
    const long long m0 = s->nHost;
    s->nHost += n; s->c44 = cNew;
    {
        // out[m] = the 44.1 k -> fs converter's frame m - A of the stem stream shifted by Dl = (D + 1) * 1024 input frames
        SrtRsStreamArgs a; memset(&a, 0, sizeof a);
        a.ring = s->d_sring; a.cap = s->capS; a.C = nc;
        a.have = a.end = s->hops * OUTPUTSEG; a.shift = (long long)(s->D + 1) * OUTPUTSEG;
        a.out0 = m0 - s->A; a.nOut = n;
        a.out = s->d_planes; a.outStride = n; a.outPos = 0; a.outMask = 0x7fffffff;
        a.B = s->Bout;
        if (srt_rsstream_launch(s->fout, a, s->ldsOut, s->hop)) { s->failed = true; return stream_fail("stream converter", "kernel launch failed"); }
    }
    HIPOK(hipMemcpyAsync(s->pinOut, s->d_planes, (size_t)nc * n * sizeof(float), hipMemcpyDeviceToHost, s->hop), "stream block");
    HIPOK(hipEventRecord(s->evOut, s->hop), "stream block");
    if (s->K < s->T) HIPOK(hipEventSynchronize(s->evOut), "stream block");       // as process_hop: the call's own output only, not the run it queued
    else HIPOK(hipStreamSynchronize(s->hop), "stream block");
    for (int c = 0; c < nc; ++c) memcpy(planes[c], s->pinOut + (size_t)c * n, n * sizeof(float));
    return true;
}

// fs == 44100: the 44.1 kHz hop path as it is (host ring, one H2D and one D2H per hop), the segments queued in nq pinned slots; out[m] = y44[m - 1023].
// false: failed
bool rate_slice_44100(srt_live* s, const float* inL, const float* inR, int n, float* const* planes)
{
    const int nc = 2 * s->P;
    int left = n;
    while (left > 0) {
        const int c = (int)s->needed < left ? (int)s->needed : left;
        memcpy(&s->ring[0][s->inPos], inL, c * sizeof(float));
        memcpy(&s->ring[1][s->inPos], inR, c * sizeof(float));
        inL += c; inR += c; left -= c;
        s->inPos = (s->inPos + c) & (FFTSIZE - 1);
        s->needed -= c;
        if (s->needed == 0) process_hop(s);
    }
    s->nHost += n;
    if (s->failed) return false;
    const size_t seg = (size_t)OUTPUTSEG * nc;
    for (int i = 0; i < n; ++i) {
        const long long k = s->nHost - n + i - (OUTPUTSEG - 1);
        if (k < 0) { for (int c = 0; c < nc; ++c) planes[c][i] = 0.0f; continue; }
        const float* src = s->outq[0] + (size_t)((k / OUTPUTSEG) % s->nq) * seg + (size_t)(k % OUTPUTSEG) * nc;
        for (int c = 0; c < nc; ++c) planes[c][i] = src[c];
    }
    return true;
}

int live_process_rate(srt_live* s, const float* inL, const float* inR, int n, float* const* out)
{
    const int nc = 2 * s->P;
    float* planes[2 * SRT_MAX_STEMS];
    for (int done = 0; done < n; ) {
        const int c = n - done < s->maxBlock ? n - done : s->maxBlock;
        for (int j = 0; j < nc; ++j) planes[j] = out[j] + done;
        if (s->failed || !(s->fs == 44100 ? rate_slice_44100(s, inL + done, inR + done, c, planes) : rate_slice(s, inL + done, inR + done, c, planes)))
            for (int j = 0; j < nc; ++j) memset(planes[j], 0, c * sizeof(float));       // muted: silence, n written per call
        done += c;
    }
    return n;
}

int live_latency(int K, int L) { return (L + 2 * K) * OUTPUTSEG + OUTPUTSEG; }

// the plugin surface: VST config (4 stems, ELU, oob 0.25 / 0 / 0.25 / 0.25, Spleeter4Stems.c:444-447), K and L as given
void s4s_init(Spleeter4Stems* msr, int F, int T, void* coeffProvider[4], int K, int L, const char* who, int sampleRate = 0, int maxBlock = 0)
{
    if (!msr) return;
    SrtSetupLock setup;                                      // (srt_internal.h: set-up paths are serialised process-wide)
    memset(msr, 0, sizeof *msr);
    srt_config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.F = F; cfg.T = T; cfg.n_stems = 4; cfg.variant = SRT_VARIANT_VST; cfg.max_tiles = 1; cfg.impl = SRT_IMPL_MFMA;
    for (int k = 0; k < 4; ++k) { cfg.stem_mode[k] = 1; cfg.oob_weight[k] = k == 1 ? 0.0f : 0.25f; }      // Spleeter4Stems.c:444-447
    const bool args_ok = T >= 1 && K >= 1 && K <= T && L >= 0 && L <= T - K;
    srt_live* s = live_new(F, T, 4, args_ok ? K : (T >= 1 ? T : 1), args_ok ? L : 0, 4);
    if (!s) { stream_fail(who, "out of host memory"); return; }
    msr->impl = s;
    if (sampleRate) { s->rate = true; s->fs = sampleRate; s->maxBlock = maxBlock >= 1 ? maxBlock : 1; }     // a muted rate instance still writes inSampleCount samples per call
    if (!s->hostq) { stream_fail(who, "out of host memory"); return; }
    if (!args_ok) { stream_fail(who, "hopsPerRun must be in 1..timeStep and lookahead in 0..timeStep-hopsPerRun"); return; }
    SrtRsGeom gin, gout;
    if (sampleRate) {
        if (maxBlock < 1 || maxBlock > SRT_LIVE_MAX_BLOCK) { stream_fail(who, "maxBlock must be in 1..65536"); return; }
        if (rate_geometry(sampleRate, K, L, who, &gin, &gout, &s->A)) { stream_fail(who, nullptr); return; }
        if (sampleRate == 44100) s->nq = (maxBlock + OUTPUTSEG - 1) / OUTPUTSEG + 2;    // only the 44.1 kHz path queues segments on the host
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { stream_fail(who, "no HIP device (this library has no CPU path)"); return; }
    for (int k = 0; k < 4; ++k) if (!coeffProvider || !coeffProvider[k]) { stream_fail(who, "null coefficient pointer"); return; }
    const void* coeff[4] = { coeffProvider[0], coeffProvider[1], coeffProvider[2], coeffProvider[3] };
    if (live_init(s, cfg, coeff, who) == 0 && sampleRate) live_rate_init(s, gin, gout, who);
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

void Spleeter4StemsInitRate(Spleeter4Stems* msr, int F, int T, void* coeffProvider[4], int hopsPerRun, int lookahead, int sampleRate, int maxBlock)
{
    s4s_init(msr, F, T, coeffProvider, hopsPerRun, lookahead, "Spleeter4StemsInitRate", sampleRate ? sampleRate : -1, maxBlock);
}

int Spleeter4StemsLatency(const Spleeter4Stems* msr)
{
    const srt_live* s = msr ? (const srt_live*)msr->impl : nullptr;
    return s ? (s->rate ? s->A : live_latency(s->K, s->L)) : 0;
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
// One body behind srtLiveCreate, srtLiveCreateRate and srtLiveCreateEx; `who` names the caller in every message.  rate: a rate instance (sample_rate, max_block).
// o: srtLiveCreateEx's options (never null; all zero for the two older calls).  Every argument is checked before any HIP call.
namespace {
int live_create(const srt_config* cfg, int hops_per_run, int lookahead, bool rate, const srt_live_opts& o, const void* const* h_coeff, srt_live** out, const char* who, int iterations = 0)
{
    if (!cfg || !h_coeff || !out) return srt_set_error(-1, "%s: null argument", who);
    *out = nullptr;
    if (const int rc = srt_check_config(cfg, who)) return rc;             // srtCreate's own checks, before any HIP call
    if (cfg->max_tiles != 1) return srt_set_error(-1, "%s: max_tiles must be 1 (a run is one window)", who);
    if (hops_per_run < 1 || hops_per_run > cfg->T) return srt_set_error(-1, "%s: hops_per_run must be in 1..T", who);
    if (lookahead < 0 || lookahead > cfg->T - hops_per_run) return srt_set_error(-1, "%s: lookahead must be in 0..T-hops_per_run", who);
    SrtRsGeom gin, gout;
    int A = 0;
    if (rate) {
        if (o.max_block < 1 || o.max_block > SRT_LIVE_MAX_BLOCK) return srt_set_error(-1, "%s: max_block must be in 1..65536", who);
        if (const int rc = rate_geometry(o.sample_rate, hops_per_run, lookahead, who, &gin, &gout, &A)) return rc;
    }
    if (o.n_out < 0 || o.n_out > SRT_MAX_STEMS) return srt_set_error(-1, "%s: n_out must be in 0..SRT_MAX_STEMS (8)", who);
    if (o.n_out > 0 && !o.h_gain) return srt_set_error(-1, "%s: null h_gain with n_out > 0", who);
    if (o.n_out > 0 && !gain_finite(o.h_gain, o.n_out * (cfg->n_stems + 1))) return srt_set_error(-1, "%s: h_gain has an entry that is not finite", who);
    if (o.mask_extension != SRT_MASK_EXT_CONSTANT && o.mask_extension != SRT_MASK_EXT_AVERAGE) return srt_set_error(-1, "%s: unknown mask_extension (SRT_MASK_EXT_CONSTANT or SRT_MASK_EXT_AVERAGE)", who);
    if (iterations < 0 || iterations > SRT_WIENER_MAX_ITERS) return srt_set_error(-1, "%s: iterations must be 0 (the filter off) .. 3", who);
    if (iterations > 0 && cfg->ratio_mask) return srt_set_error(-1, "%s: the Wiener filter and ratio_mask exclude each other (both are the post-processing of the masks)", who);
    for (int k = 0; k < cfg->n_stems; ++k)
        if (!h_coeff[k]) return srt_set_error(-1, "%s: null coefficient blob", who);
    SrtSetupLock setup;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return srt_set_error(-3, "%s: no HIP device (this library has no CPU path)", who);
    const int S = cfg->n_stems;
    srt_live* s = live_new(cfg->F, cfg->T, S, hops_per_run, lookahead, o.n_out > 0 ? o.n_out : S);
    if (!s || !s->hostq) { live_free(s); return srt_set_error(-2, "%s: out of host memory", who); }
    s->nOut = o.n_out;
    s->ext = o.mask_extension == SRT_MASK_EXT_AVERAGE;
    s->combine = s->nOut > 0 || s->ext;                                       // neither: the launches of srtLiveCreate, untouched
    s->W = iterations;
    if (s->W && s->T > s->D) s->R = s->T;                                     // the filter's statistics read the whole window's spectrum rows
    if (s->nOut > 0) for (int m = 0; m < s->nOut; ++m) memcpy(s->G[m], o.h_gain + (size_t)m * (S + 1), (S + 1) * sizeof(float));
    else for (int m = 0; m < S; ++m) s->G[m][m] = 1.0f;                       // the extension alone: every stem through the identity (a one-hot chain gives g_s exactly)
    if (rate) {
        s->rate = true; s->fs = o.sample_rate; s->maxBlock = o.max_block; s->A = A;
        if (o.sample_rate == 44100) s->nq = (o.max_block + OUTPUTSEG - 1) / OUTPUTSEG + 2;     // only the 44.1 kHz path queues segments on the host
    }
    int rc = live_init(s, *cfg, h_coeff, who);
    if (rc == 0 && rate) rc = live_rate_init(s, gin, gout, who);
    if (rc) { live_free(s); return rc; }
    *out = s;
    return 0;
}
}  // namespace

int srtLiveCreate(const srt_config* cfg, int hops_per_run, int lookahead, const void* const* h_coeff, srt_live** out)
{
    srt_live_opts o; memset(&o, 0, sizeof o);
    return live_create(cfg, hops_per_run, lookahead, false, o, h_coeff, out, "srtLiveCreate");
}

int srtLiveCreateEx(const srt_config* cfg, int hops_per_run, int lookahead, const srt_live_opts* opts, const void* const* h_coeff, srt_live** out)
{
    srt_live_opts o; memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    return live_create(cfg, hops_per_run, lookahead, o.sample_rate != 0, o, h_coeff, out, "srtLiveCreateEx");
}

int srtLiveSetMix(srt_live* s, const float* h_gain)
{
    if (!s) return srt_set_error(-1, "%s", "srtLiveSetMix: null argument");
    if (s->nOut == 0) return srt_set_error(-1, "%s", "srtLiveSetMix: the instance was created with n_out = 0 (the number of outputs is fixed at creation)");
    if (!h_gain) return srt_set_error(-1, "%s", "srtLiveSetMix: null h_gain");
    if (!gain_finite(h_gain, s->nOut * (s->S + 1))) return srt_set_error(-1, "%s", "srtLiveSetMix: h_gain has an entry that is not finite");
    for (int m = 0; m < s->nOut; ++m) memcpy(s->G[m], h_gain + (size_t)m * (s->S + 1), (s->S + 1) * sizeof(float));     // host state only: the next hop's launch carries it
    return 0;
}

int srtLiveOutputs(const srt_live* s)
{
    return s ? s->P : 0;
}

int srtLiveCreateWiener(const srt_config* cfg, int hops_per_run, int lookahead, const srt_live_opts* opts, int iterations, const void* const* h_coeff, srt_live** out)
{
    srt_live_opts o; memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    return live_create(cfg, hops_per_run, lookahead, o.sample_rate != 0, o, h_coeff, out, "srtLiveCreateWiener", iterations);
}

int srtLiveWiener(const srt_live* s)
{
    return s ? s->W : 0;
}

// debug read-back of the run launched last (not for the audio thread: both streams are drained).  Every argument is checked before any HIP call.
int srtLiveCopyTensor(srt_live* s, const char* name, int stem, int index, float* h_dst, size_t max_floats, long long* run_hop)
{
    if (!s || !name || !h_dst) return srt_set_error(-1, "%s", "srtLiveCopyTensor: null argument");
    const size_t F = (size_t)s->F;
    const bool cov = !strcmp(name, "wiener_cov"), spec = !strcmp(name, "wiener_spec"), masks = !strcmp(name, "masks");
    if (!cov && !spec && !masks) return srt_set_error(-1, "srtLiveCopyTensor: unknown tensor %s (wiener_cov, wiener_spec, masks)", name);
    if ((cov || spec) && !s->W) return srt_set_error(-1, "srtLiveCopyTensor: %s needs an instance of srtLiveCreateWiener with iterations > 0", name);
    if ((cov || masks) && (stem < 0 || stem >= s->S)) return srt_set_error(-1, "srtLiveCopyTensor: %s needs a stem in 0..n_stems-1", name);
    if (cov && (index < 1 || index > s->W)) return srt_set_error(-1, "%s", "srtLiveCopyTensor: wiener_cov needs 1 <= index (the iteration) <= the instance's iterations");
    const size_t count = cov ? 5 * F + 1 : spec ? 2 * (size_t)s->T * SRT_SPEC_LD * 2 : 2 * s->hw;
    if (count > max_floats) return srt_set_error(-1, "%s", "srtLiveCopyTensor: destination too small");
    if (s->failed) return srt_set_error(-1, "%s", "srtLiveCopyTensor: the instance is muted (an earlier device call failed)");
    if (run_hop) *run_hop = s->runHop;
    if (s->runHop < 0) return 0;
#define COPYTRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return srt_set_error(-2, "srtLiveCopyTensor: %s", hipGetErrorString(_e)); } while (0)
    COPYTRY(hipStreamSynchronize(s->hop));
    COPYTRY(hipStreamSynchronize(s->nn));
    if (cov) {                                                               // srtCopyTensor("wiener_cov")'s layout: R [F][4], the weight sums [F], a
        const SrtWienerParams w = wiener_params(s, s->runBuf);
        const size_t o = ((size_t)(index - 1) * s->S + stem) * F;
        COPYTRY(hipMemcpy(h_dst, w.rtab + o * 4, F * 4 * sizeof(float), hipMemcpyDeviceToHost));
        COPYTRY(hipMemcpy(h_dst + 4 * F, w.wsum + o, F * sizeof(float), hipMemcpyDeviceToHost));
        COPYTRY(hipMemcpy(h_dst + 5 * F, w.scal, sizeof(float), hipMemcpyDeviceToHost));
    } else if (spec) COPYTRY(hipMemcpy(h_dst, s->d_wspec, count * sizeof(float), hipMemcpyDeviceToHost));
    else COPYTRY(hipMemcpy(h_dst, masks_buf(s, s->runBuf) + (size_t)stem * 2 * s->hw, count * sizeof(float), hipMemcpyDeviceToHost));
#undef COPYTRY
    return (int)count;
}

int srtLiveRateLatency(int sample_rate, int hops_per_run, int lookahead)
{
    if (hops_per_run < 1 || lookahead < 0) return srt_set_error(-1, "%s", "srtLiveRateLatency: hops_per_run must be at least 1 and lookahead at least 0");
    SrtRsGeom gin, gout;
    int A = 0;
    if (const int rc = rate_geometry(sample_rate, hops_per_run, lookahead, "srtLiveRateLatency", &gin, &gout, &A)) return rc;
    return A;
}

int srtLiveCreateRate(const srt_config* cfg, int hops_per_run, int lookahead, int sample_rate, int max_block, const void* const* h_coeff, srt_live** out)
{
    srt_live_opts o; memset(&o, 0, sizeof o);
    o.sample_rate = sample_rate; o.max_block = max_block;
    return live_create(cfg, hops_per_run, lookahead, true, o, h_coeff, out, "srtLiveCreateRate");
}

int srtLiveProcess(srt_live* s, const float* inL, const float* inR, int n, float* const* out)
{
    if (!s || n < 0 || (n > 0 && (!inL || !inR || !out))) return srt_set_error(-1, "%s", "srtLiveProcess: bad argument");
    if (n > 0) for (int j = 0; j < 2 * s->P; ++j) if (!out[j]) return srt_set_error(-1, "%s", "srtLiveProcess: null output plane");
    return live_process(s, inL, inR, n, out);
}

int srtLiveLatency(const srt_live* s)
{
    if (!s) return srt_set_error(-1, "%s", "srtLiveLatency: null argument");
    return s->rate ? s->A : live_latency(s->K, s->L);
}

void srtLiveDestroy(srt_live* s)
{
    live_free(s);
}
