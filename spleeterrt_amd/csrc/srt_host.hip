// srt_host.hip — the host-buffer entry points of the engine: the device staging, srtSeparateCliHost and the chunk pipeline of srtSeparateHostStream (its private declarations: srt_engine.h).
#include "srt_engine.h"

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

// Long host-resident stream through one GPU: the stream is cut into chunks of max_tiles tiles (tiles are independent,
// main.c:455-495); chunk c+1's PCM goes up and chunk c-1's stems come down on two copy streams while chunk c computes,
// and the 3072-sample overlap between consecutive chunks is added on the device (srt_carry_kernel), so every output
// sample crosses PCIe exactly once.  Geometry as srtSeparateEx (a tile range of a longer stream: rows = whole tiles,
// frames = rows; the whole stream: rows = srtStftRows(n), frames = srtStftFrames(n)).
// cli_stems = 0: the n_stems sub-networks on the same input (separate_run per chunk, srtSeparateEx's body); 2 / 3: the CLI's flows (cli_issue per chunk)
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
    const SepOpts o = engine_opts(e);                   // once for the call: the refusals, the plane count and every chunk's separate_run
    if (o.overlap) return fail(-1, OVERLAP_REFUSED, "srtSeparateHostStream");   // the blend would have to cross the chunk seams
    if (o.wiener) return fail(-1, "srtSeparateHostStream: the Wiener filter's statistics span the whole signal (chunks would each get their own covariance): use srtSeparate, or srtSetWiener(e, 0)");
    DeviceScope ds(e->device);
    const int S = cli_stems ? cli_stems : o.n_out ? o.n_out : e->cfg.n_stems, T = e->cfg.T, NP = S * 2;     // pairs staged, carried, packed and downloaded: the outputs of a remix
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
                       : separate_run(e, o, h.d_in[b], h.d_in[b] + in_cap, ns, cfr, crow, h.d_out[b]);
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
