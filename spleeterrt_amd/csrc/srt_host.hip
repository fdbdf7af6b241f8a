// srt_host.hip — the host-buffer entry points of the engine: the device staging, srtSeparateCliHost, the chunk pipeline of srtSeparateHostStream (with the converters of
// srtSeparateHostStreamRate at both ends of a piece) and the two sweeps of srtSeparateHostWiener / srtSeparateHostWienerOverlap (its private declarations: srt_engine.h).
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

// The integer staging of the PCM flags (16- and 24-bit share it), after ensure_staging (streams exist): grow-only like the float buffers; 0 bytes = not wanted
// by this call.
static int ensure_staging_pcm(srt_engine* e, size_t in_bytes, size_t out_bytes)
{
    HostStaging& h = e->hs;
    if (in_bytes > h.inq_cap || out_bytes > h.outq_cap) {
        HIPCHK(hipStreamSynchronize(h.s_in)); HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipStreamSynchronize(h.s_out));
    }
    for (int b = 0; b < 2; ++b) {
        if (in_bytes > h.inq_cap) {
            if (h.d_inq[b]) { hipFree(h.d_inq[b]); h.d_inq[b] = nullptr; }
            HIPCHK(hipMalloc(&h.d_inq[b], in_bytes));
        }
        if (out_bytes > h.outq_cap) {
            if (h.d_outq[b]) { hipFree(h.d_outq[b]); h.d_outq[b] = nullptr; }
            HIPCHK(hipMalloc(&h.d_outq[b], out_bytes));
        }
    }
    if (in_bytes > h.inq_cap) h.inq_cap = in_bytes;
    if (out_bytes > h.outq_cap) h.outq_cap = out_bytes;
    if (out_bytes && !h.d_clip) HIPCHK(hipMalloc((void**)&h.d_clip, (SRT_MAX_STEMS + srt_pcm16_pack_scratch(SRT_MAX_STEMS)) * sizeof(unsigned long long)));
    return 0;
}

// srtSeparateHostStreamOverlap's mask seam carry, after ensure_staging: grow-only like the rest
static int ensure_mask_seam(srt_engine* e, size_t floats)
{
    HostStaging& h = e->hs;
    if (floats <= h.mseam_cap) return 0;
    HIPCHK(hipStreamSynchronize(e->stream));
    if (h.d_mseam) { hipFree(h.d_mseam); h.d_mseam = nullptr; h.mseam_cap = 0; }
    HIPCHK(hipMalloc((void**)&h.d_mseam, floats * sizeof(float)));
    h.mseam_cap = floats;
    return 0;
}

// Piece p of a stream of `rows` rows under overlap O on an engine of P = max_tiles (N = overlap_tiles(rows, T, O), p * P < N): tiles
// [pP, min((p + 1) P, N)); it owns the rows whose primary tile is one of them - [pPS, (p + 1) PS), the last piece up to `rows` - and analyses the rows its tiles
// cover, (tiles - 1) S + T from row0 (the last piece: what is left), O of them owned by the next piece.  O = 0: chunks of P * T rows.
static srt_host_piece host_ov_piece(size_t rows, int T, int O, int P, size_t N, size_t p)
{
    const size_t S = (size_t)(T - O);
    srt_host_piece pc;
    pc.tile0 = p * P;
    pc.tiles = N - pc.tile0 < (size_t)P ? N - pc.tile0 : (size_t)P;
    pc.row0 = pc.tile0 * S;
    pc.own_rows = pc.tile0 + pc.tiles == N ? rows - pc.row0 : pc.tiles * S;
    const size_t span = (pc.tiles - 1) * S + T;
    pc.stft_rows = rows - pc.row0 < span ? rows - pc.row0 : span;
    return pc;
}

size_t srtHostOverlapPieces(size_t rows, int T, int overlap_rows, int max_tiles, srt_host_piece* pieces, size_t max_pieces)
{
    if (T < 1 || !overlap_ok(overlap_rows, T)) { fail(-1, "srtHostOverlapPieces: need T >= 1 and 0 <= overlap_rows <= T / 2"); return 0; }
    if (max_tiles < 1) { fail(-1, "srtHostOverlapPieces: need max_tiles >= 1"); return 0; }
    const size_t N = overlap_tiles(rows, T, overlap_rows), count = (N + max_tiles - 1) / max_tiles;
    for (size_t p = 0; pieces && p < count && p < max_pieces; ++p) pieces[p] = host_ov_piece(rows, T, overlap_rows, max_tiles, N, p);
    return count;
}

// srtSeparateHostStreamRate's side of host_stream, resolved by the entry point: h_in holds n_src frames at the caller's rate (host_stream's n is then
// the 44.1 kHz length), fin / fout the converters of the two sides (nullptr: that side is at 44.1 kHz), len_out the frames of an output plane
struct HostRate { size_t n_src; const SrtRsFilter* fin; const SrtRsFilter* fout; size_t len_out; };
// ---- srtSeparateHostStreamRate's plan.  Piece `pc` of a 44.1 kHz stream of n44 samples (len44 per output plane) whose source holds n_src frames; gi / go: the
// geometry of in_rate -> 44100 / 44100 -> out_rate, nullptr where that side is at 44.1 kHz.  The source window is every frame a window of 44.1 kHz frames [s0, s0 + ns) starts
// or ends on, cut to [0, n_src); the output range ends at the last frame whose weighted taps lie before fin1 (srt_rs_computable), so the ranges of the pieces tile [0, len_out).
static srt_host_rate_piece host_rate_piece(const srt_host_piece& pc, bool last, size_t n_src, size_t n44, size_t len44, size_t len_out, const SrtRsGeom* gi, const SrtRsGeom* go)
{
    const size_t tail = SRT_FFT - SRT_HOP, row1 = pc.row0 + pc.stft_rows;
    srt_host_rate_piece r;
    r.s0 = pc.row0 * SRT_HOP;
    const size_t send = row1 * SRT_HOP + tail < n44 ? row1 * SRT_HOP + tail : n44;
    r.ns = send > r.s0 ? send - r.s0 : 0;
    r.src0 = r.s0; r.src_len = r.ns;
    if (gi) {
        long long lo = 0, hi = 0;
        if (r.ns) {
            lo = (long long)((unsigned __int128)r.s0 * gi->P / gi->Q) - gi->LO;
            hi = (long long)((unsigned __int128)(send - 1) * gi->P / gi->Q) - gi->LO + gi->T4;
            if (lo < 0) lo = 0;
            if (hi > (long long)n_src) hi = (long long)n_src;
            if (hi < lo) hi = lo;
        }
        r.src0 = (size_t)lo; r.src_len = (size_t)(hi - lo);
    }
    r.fin0 = r.s0; r.fin1 = last ? len44 : r.s0 + pc.own_rows * SRT_HOP;
    r.out0 = r.fin0; r.out1 = r.fin1;
    if (go) {
        const size_t j0 = (size_t)srt_rs_computable(*go, (long long)r.fin0), j1 = (size_t)srt_rs_computable(*go, (long long)r.fin1);
        r.out0 = j0 < len_out ? j0 : len_out;
        r.out1 = last || j1 > len_out ? len_out : j1;
    }
    return r;
}

// rates, lengths and the two geometries of a call; 0, or -1 with the error set
struct HostRateDims { size_t n44, rows, len44, len_out; bool cin, cout; SrtRsGeom gi, go; };
static int host_rate_dims(size_t n, int in_rate, int out_rate, const char* who, HostRateDims* d)
{
    if (in_rate < SRT_RS_MIN_RATE || in_rate > SRT_RS_MAX_RATE || out_rate < SRT_RS_MIN_RATE || out_rate > SRT_RS_MAX_RATE) return fail(-1, "%s: sample rates must lie in 8000..384000 Hz", who);
    d->cin = in_rate != 44100; d->cout = out_rate != 44100;
    d->n44 = d->cin ? srtResampleLength(n, in_rate, 44100) : n;
    if (d->n44 < SRT_FFT) return fail(-1, "%s: need at least 4096 samples at 44.1 kHz", who);
    if (n > (size_t)1 << 42 || srtStftRows(d->n44) > (size_t)0x7fffffff - 4) return fail(-1, "%s: stream too long (more than 2^31 rows)", who);
    d->rows = srtStftRows(d->n44);
    d->len44 = srtIstftLength(d->rows);
    d->len_out = d->cout ? srtResampleLength(d->len44, 44100, out_rate) : d->len44;
    int B, np, wl;
    if (d->cin && (srt_rs_geometry(in_rate, 44100, false, 0, 0, who, &d->gi) || srt_rs_spans_shape(d->gi, 1, &B, &np, &wl)))
        return fail(-1, "%s: the input converter's window does not fit the LDS for this rate pair", who);
    if (d->cout && (srt_rs_geometry(44100, out_rate, false, 0, 0, who, &d->go) || srt_rs_spans_shape(d->go, 1, &B, &np, &wl)))
        return fail(-1, "%s: the output converter's window does not fit the LDS for this rate pair", who);
    return 0;
}

size_t srtHostRateLength(size_t n, int in_rate, int out_rate)
{
    HostRateDims d;
    return host_rate_dims(n, in_rate, out_rate, "srtHostRateLength", &d) ? 0 : d.len_out;
}

size_t srtHostRatePieces(const srt_config* cfg, size_t n, int in_rate, int out_rate, int overlap_rows, srt_host_rate_piece* pieces, size_t max_pieces)
{
    static const char* const who = "srtHostRatePieces";
    if (!cfg) { fail(-1, "%s: null config", who); return 0; }
    if (srt_check_config(cfg, who)) return 0;
    HostRateDims d;
    if (host_rate_dims(n, in_rate, out_rate, who, &d)) return 0;
    if (!overlap_ok(overlap_rows, cfg->T)) { fail(-1, "%s: overlap_rows must be 0 .. T / 2", who); return 0; }
    const size_t N = overlap_tiles(d.rows, cfg->T, overlap_rows), count = (N + cfg->max_tiles - 1) / cfg->max_tiles;
    for (size_t p = 0; pieces && p < count && p < max_pieces; ++p)
        pieces[p] = host_rate_piece(host_ov_piece(d.rows, cfg->T, overlap_rows, cfg->max_tiles, N, p), p + 1 == count, n, d.n44, d.len44, d.len_out, d.cin ? &d.gi : nullptr, d.cout ? &d.go : nullptr);
    return count;
}

// the staging of the rate forms, after ensure_staging (streams exist): grow-only like the rest; 0 floats = not wanted by this call
static int ensure_rate_staging(srt_engine* e, size_t in_floats, size_t out_floats, size_t carry_floats)
{
    HostStaging& h = e->hs;
    if (in_floats > h.rin_cap || out_floats > h.rout_cap || carry_floats > h.rcarry_cap) {
        HIPCHK(hipStreamSynchronize(h.s_in)); HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipStreamSynchronize(h.s_out));
    }
    for (int b = 0; b < 2; ++b) {
        if (in_floats > h.rin_cap) {
            if (h.d_rin[b]) { hipFree(h.d_rin[b]); h.d_rin[b] = nullptr; }
            HIPCHK(hipMalloc((void**)&h.d_rin[b], in_floats * sizeof(float)));
        }
        if (out_floats > h.rout_cap) {
            if (h.d_rout[b]) { hipFree(h.d_rout[b]); h.d_rout[b] = nullptr; }
            HIPCHK(hipMalloc((void**)&h.d_rout[b], out_floats * sizeof(float)));
        }
    }
    if (in_floats > h.rin_cap) h.rin_cap = in_floats;
    if (out_floats > h.rout_cap) h.rout_cap = out_floats;
    if (carry_floats > h.rcarry_cap) {
        if (h.d_rcarry) { hipFree(h.d_rcarry); h.d_rcarry = nullptr; h.rcarry_cap = 0; }
        HIPCHK(hipMalloc((void**)&h.d_rcarry, carry_floats * sizeof(float)));
        h.rcarry_cap = carry_floats;
    }
    return 0;
}

// The sample formats of a call's flags.  in_bytes / out_bytes: bytes of a stereo frame in the caller's buffers (8: floats, two planes of 4).
struct HostFmt {
    int in_bits, out_bits; bool dither;
    bool pcm_in() const { return in_bits != 32; }
    bool pcm_out() const { return out_bits != 32; }
    size_t in_bytes() const { return (size_t)in_bits / 4; }
    size_t out_bytes() const { return (size_t)out_bits / 4; }
};
static const unsigned SRT_HOST_FLAGS = SRT_HOST_PINNED | SRT_HOST_IN_PCM16 | SRT_HOST_OUT_PCM16 | SRT_HOST_IN_PCM24 | SRT_HOST_OUT_PCM24 | SRT_HOST_OUT_DITHER;
// 0, or -1 with the error set: nothing has touched the device
static int host_fmt(unsigned flags, const void* h_in2, const char* who, HostFmt* f)
{
    const bool in16 = flags & SRT_HOST_IN_PCM16, in24 = flags & SRT_HOST_IN_PCM24, out16 = flags & SRT_HOST_OUT_PCM16, out24 = flags & SRT_HOST_OUT_PCM24;
    if (in16 && in24) return fail(-1, "%s: SRT_HOST_IN_PCM16 and SRT_HOST_IN_PCM24 are two formats of one buffer: set one", who);
    if (out16 && out24) return fail(-1, "%s: SRT_HOST_OUT_PCM16 and SRT_HOST_OUT_PCM24 are two formats of one buffer: set one", who);
    if ((flags & SRT_HOST_OUT_DITHER) && !out16) return fail(-1, "%s: SRT_HOST_OUT_DITHER dithers the 16-bit output: it needs SRT_HOST_OUT_PCM16 (and is refused with 24-bit or float output)", who);
    if ((in16 || in24) && h_in2) return fail(-1, in16 ? "%s: SRT_HOST_IN_PCM16 takes one interleaved buffer (h_in2 must be NULL)" : "%s: SRT_HOST_IN_PCM24 takes one interleaved buffer (h_in2 must be NULL)", who);
    f->in_bits = in16 ? 16 : in24 ? 24 : 32;
    f->out_bits = out16 ? 16 : out24 ? 24 : 32;
    f->dither = flags & SRT_HOST_OUT_DITHER;
    return 0;
}
// a chunk's integer frames in d_inq -> planar floats; `count` frames of `pairs` pairs -> d_outq, pair p at p * stride frames, the clipped samples added to d_clip
// (then its scratch follows it).  first_index: the position of the launch's sample 0 in its output plane, for the dither.  Without the new bits the launches
// are the 16-bit ones under their timer names.
static int host_unpack(srt_engine* e, const HostFmt& f, const void* d_q, size_t n, float* L, float* R)
{
    TimerScope ts(e, f.in_bits == 24 ? "pcm24_unpack" : "pcm16_unpack");
    if (f.in_bits == 24 ? srt_launch_pcm24_unpack((const uint8_t*)d_q, n, L, R, e->stream) : srt_launch_pcm16_unpack((const int16_t*)d_q, n, L, R, e->stream))
        return fail(-2, f.in_bits == 24 ? "pcm24 unpack launch failed" : "pcm16 unpack launch failed");
    return 0;
}
static int host_pack(srt_engine* e, const HostFmt& f, const SepOpts& o, const float* planes, size_t stride, int pairs, size_t count, void* d_q, unsigned long long* d_clip, size_t first_index)
{
    unsigned long long* const scratch = d_clip ? d_clip + SRT_MAX_STEMS : nullptr;
    TimerScope ts(e, f.out_bits == 24 ? "pcm24_pack" : f.dither ? "pcm16_pack_dither" : "pcm16_pack");
    const int rc = f.out_bits == 24 ? srt_launch_pcm24_pack(planes, stride, pairs, count, (uint8_t*)d_q, stride, d_clip, scratch, e->stream)
                 : f.dither ? srt_launch_pcm16_pack_dither(planes, stride, pairs, count, (int16_t*)d_q, stride, d_clip, scratch, o.dither_seed, 0, first_index, e->stream)
                 : srt_launch_pcm16_pack(planes, stride, pairs, count, (int16_t*)d_q, stride, d_clip, scratch, e->stream);
    return rc ? fail(-2, f.out_bits == 24 ? "pcm24 pack launch failed" : "pcm16 pack launch failed") : 0;
}

static int host_stream(srt_engine* e, const void* h_in, const void* h_in2, size_t n, size_t frames, size_t rows, void* h_out, unsigned flags, int cli_stems,
                       SrtSeam seam = SrtSeam{0, nullptr, false}, unsigned long long* h_clipped = nullptr, int call_overlap = -1, const HostRate* rate = nullptr);

// Host-buffer form of srtSeparateCli for plain-C callers (the CLI harness): synchronous.  A file that fits the engine's capacity
// (max_tiles tiles) is one resident batch: H2D, chain, D2H.  A longer one - any length, as the reference's tile loop over a
// host-resident spectrogram handles (main.c:455-495) - goes through the chunked pipeline of srtSeparateHostStream: max_tiles tiles
// at a time, copies overlapped with compute, the residual chain evaluated per chunk (it is row-local) and the time-domain
// subtraction applied after the 3072-sample chunk overlaps have been added on the device.
// flags: SRT_HOST_* (srtSeparateCliHostIo).  An integer side always takes the chunked pipeline, whose staging holds the conversion (one chunk when the file fits).
static int cli_host(srt_engine* e, const void* h_in, const void* h_in2, size_t n, int stems, void* h_out_, unsigned flags, unsigned long long* h_clipped)
{
    const bool pcm = flags & (SRT_HOST_IN_PCM16 | SRT_HOST_OUT_PCM16 | SRT_HOST_IN_PCM24 | SRT_HOST_OUT_PCM24);
    HostFmt f;
    if (const int rc = host_fmt(flags, h_in2, "srtSeparateCliHostIo", &f)) return rc;
    if (!e || !h_in || (!f.pcm_in() && !h_in2) || !h_out_) return fail(-1, "srtSeparateCliHost: null argument");
    DeviceScope ds(e->device);
    int rc = cli_check(e, stems);
    if (rc) return rc;
    if (n < SRT_FFT) return fail(-1, "srtSeparateCli: need at least 4096 samples");
    const size_t rows = srtStftRows(n), len = srtIstftLength(rows);
    if (pcm || (rows + e->cfg.T - 1) / e->cfg.T > (size_t)e->cfg.max_tiles)
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
// Integer PCM (flags).  SRT_HOST_IN_PCM16 / _PCM24: h_in is int16 [n][2] / uint8 [n][2][3] (h_in2 unused); a chunk's frames go up as one copy
// into d_inq[b] and are unpacked into d_in[b] on the compute stream (ev_cmp[b] releases both).  SRT_HOST_OUT_PCM16 / _PCM24: h_out is int16 [planes / 2][total_len][2]
// / uint8 [planes / 2][total_len][2][3]; after the seam add (and the CLI flows' subtraction) the samples this chunk downloads - each plane's [0, take) - are packed
// into d_outq[b], so every output sample is quantised and counted once, and ev_cmp[b] is recorded after the pack.  SRT_HOST_OUT_DITHER: the 16-bit pack adds the
// TPDF dither of (o.dither_seed, plane, position in the whole output plane), so the chunking does not show.  h_clipped [stems]: the clipped samples of each stem
// (zero without an OUT flag).
// call_overlap >= 0: srtSeparateHostStreamOverlap - the call's own overlap in place of the engine's, which is then neither read nor refused.  The
// chunks are the pieces of host_ov_piece: a piece uploads and analyses stft_rows rows, of which it inverts, stitches and downloads the first own_rows
// (separate_piece); after every piece but the last the mask rows the next piece's first O rows blend with are kept (srt_mask_seam_save_kernel).  At 0 the pieces are
// the chunks and every launch is the one the engine's path issues.
// rate != nullptr: srtSeparateHostStreamRate.  With rate->fin a piece uploads the source frames host_rate_piece names into d_rin[b] (integer PCM: d_inq[b],
// unpacked into d_rin[b]) and the spans kernel writes d_in[b] in front of the transform; with rate->fout the spans kernel converts every pair behind the seam add - span A
// the rate carry, span B the piece's planes - into d_rout[b], which the pack and the download then take in d_out[b]'s place.  Without either the launches are the ones above.
static int host_stream(srt_engine* e, const void* h_in, const void* h_in2, size_t n, size_t frames, size_t rows, void* h_out_, unsigned flags, int cli_stems, SrtSeam seam,
                       unsigned long long* h_clipped, int call_overlap, const HostRate* rate)
{
    const char* const who = rate ? "srtSeparateHostStreamRate" : call_overlap >= 0 ? "srtSeparateHostStreamOverlap" : "srtSeparateHostStream";
    HostFmt f;
    if (const int frc = host_fmt(flags, h_in2, who, &f)) return frc;
    const bool inq = f.pcm_in(), outq = f.pcm_out();
    const size_t ib = f.in_bytes(), ob = f.out_bytes();
    if (!e || !h_in || (!inq && !h_in2) || !h_out_) return fail(-1, "%s: null argument", who);
    if ((inq || outq) && seam.out_stride) return fail(-1, "%s: the 16-bit and 24-bit PCM forms and the dither do not apply to a tile range of a multi-device stream (the seam join adds floats on the host)", who);
    const float *h_L = (const float*)h_in, *h_R = (const float*)h_in2;
    float* h_out = (float*)h_out_;
    if (rows < 1 || frames > rows) return fail(-1, "%s: need 1 <= frames <= rows", who);
    SepOpts o = engine_opts(e);                         // once for the call: the refusals, the plane count and every chunk's separate_run
    if (call_overlap >= 0) {
        if (!overlap_ok(call_overlap, e->cfg.T)) return fail(-1, "%s: overlap_rows must be 0 .. T / 2", who);
        o.overlap = call_overlap;
    } else if (o.overlap) return fail(-1, OVERLAP_REFUSED, who);   // the blend crosses the chunk seams: srtSeparateHostStreamOverlap carries it
    if (o.wiener) return fail(-1, "%s: the Wiener filter's statistics span the whole signal (chunks would each get their own covariance): use srtSeparate, or srtSetWiener(e, 0)", who);
    const int O = o.overlap;                            // > 0 only on srtSeparateHostStreamOverlap's path
    if (call_overlap >= 0) for (int s = 0; s < e->cfg.n_stems; ++s) if (!e->have_coeff[s]) return fail(-5, "%s: weights not set for every stem", who);
    DeviceScope ds(e->device);
    const int S = cli_stems ? cli_stems : o.n_out ? o.n_out : e->cfg.n_stems, T = e->cfg.T, NP = S * 2;     // pairs staged, carried, packed and downloaded: the outputs of a remix
    const size_t chunk_rows = (size_t)e->cfg.max_tiles * T, tail = SRT_FFT - SRT_HOP;
    const size_t ntiles_all = overlap_tiles(rows, T, O);
    const size_t nchunks = (ntiles_all + e->cfg.max_tiles - 1) / e->cfg.max_tiles, total_len = seam.out_stride ? seam.out_stride : srtIstftLength(rows);
    const size_t in_cap = chunk_rows * SRT_HOP + tail, out_cap = srtIstftLength(chunk_rows);
    int rc = ensure_staging(e, 2 * in_cap, (size_t)NP * out_cap, (size_t)NP * tail, 2);
    if (rc) return rc;
    if (O && nchunks > 1 && (rc = ensure_mask_seam(e, (size_t)e->cfg.n_stems * 2 * O * e->cfg.F))) return rc;
    const SrtSwitches sw = srt_read_switches();
    // the rate forms: the largest source window and the most output frames of a piece size the staging; the carry holds the 2 LO + 1 samples in front of a piece
    const SrtRsFilter* const fin = rate ? rate->fin : nullptr;
    const SrtRsFilter* const fout = rate ? rate->fout : nullptr;
    const size_t n_host = rate ? rate->n_src : n, out_len = fout ? rate->len_out : total_len, K = fout ? 2 * (size_t)fout->g.LO + 1 : 0;
    size_t rin_len = 0, rout_len = 0;
    for (size_t c = 0; (fin || fout) && c < nchunks; ++c) {
        const srt_host_piece pc = host_ov_piece(rows, T, O, e->cfg.max_tiles, ntiles_all, c);
        const srt_host_rate_piece rp = host_rate_piece(pc, c + 1 == nchunks, n_host, n, total_len, out_len, fin ? &fin->g : nullptr, fout ? &fout->g : nullptr);
        if (rp.src_len > rin_len) rin_len = rp.src_len;
        if (rp.out1 - rp.out0 > rout_len) rout_len = rp.out1 - rp.out0;
        if (fout && c + 1 < nchunks && rp.fin1 - rp.fin0 < K) return fail(-1, "%s: a piece finalises fewer samples than the output converter's history", who);
    }
    if ((fin || fout) && (rc = ensure_rate_staging(e, fin ? 2 * rin_len : 0, fout ? (size_t)NP * rout_len : 0, (size_t)NP * K))) return rc;
    if ((inq || outq) && (rc = ensure_staging_pcm(e, inq ? ib * (fin && rin_len > in_cap ? rin_len : in_cap) : 0, outq ? ob * S * (fout && rout_len > out_cap ? rout_len : out_cap) : 0))) return rc;
    HostStaging& h = e->hs;
    if (h_clipped) memset(h_clipped, 0, (size_t)S * sizeof *h_clipped);
    unsigned long long* d_clip = outq && h_clipped ? h.d_clip : nullptr;
    if (d_clip) HIPCHK(hipMemsetAsync(d_clip, 0, (size_t)S * sizeof *d_clip, e->stream));
    // Page-locked caller buffers let the copies run asynchronously.  SRT_HOST_PINNED: the caller guarantees they already are
    // (hipHostMalloc / hipHostRegister / torch pin_memory) and nothing is registered here; otherwise the three buffers are
    // registered for the duration of the call (if that fails the copies still work, staged by the runtime).
    bool pinL = false, pinR = false, pinO = false;
    if (!(flags & SRT_HOST_PINNED)) {
        pinL = hipHostRegister((void*)h_in, n_host * (inq ? ib : sizeof(float)), hipHostRegisterDefault) == hipSuccess;       // (int16 [n][2] is n * 4 bytes too)
        pinR = !inq && hipHostRegister((void*)h_R, n_host * sizeof(float), hipHostRegisterDefault) == hipSuccess;
        pinO = !seam.out_stride && hipHostRegister((void*)h_out, (size_t)S * out_len * ob, hipHostRegisterDefault) == hipSuccess;
        (void)hipGetLastError();
    }
    hipError_t er = hipSuccess;
#define STEP(x) do { if (er == hipSuccess) er = (x); } while (0)
    for (size_t c = 0; c < nchunks && er == hipSuccess && rc == 0; ++c) {
        const int b = (int)(c & 1);
        const srt_host_piece pc = host_ov_piece(rows, T, O, e->cfg.max_tiles, ntiles_all, c);
        const size_t row0 = pc.row0, crow = pc.own_rows, row1 = row0 + pc.stft_rows;       // rows [row0, row1) go up and are analysed, the first crow of them come down
        const size_t s0 = row0 * SRT_HOP, send = row1 * SRT_HOP + tail < n ? row1 * SRT_HOP + tail : n;
        const size_t ns = send > s0 ? send - s0 : 0;
        const size_t cfr = frames > row0 ? (frames - row0 < pc.stft_rows ? frames - row0 : pc.stft_rows) : 0;
        const size_t clen = srtIstftLength(crow);
        const srt_host_rate_piece rp = host_rate_piece(pc, c + 1 == nchunks, n_host, n, total_len, out_len, fin ? &fin->g : nullptr, fout ? &fout->g : nullptr);
        // upload: the input buffer is free once the compute that read it two chunks ago has finished
        if (c >= 2) STEP(hipStreamWaitEvent(h.s_in, h.ev_cmp[b], 0));
        if (fin) {                                          // the source window, at the caller's rate
            if (rp.src_len && inq) STEP(hipMemcpyAsync(h.d_inq[b], (const char*)h_in + ib * rp.src0, rp.src_len * ib, hipMemcpyHostToDevice, h.s_in));
            else if (rp.src_len) {
                STEP(hipMemcpyAsync(h.d_rin[b], h_L + rp.src0, rp.src_len * sizeof(float), hipMemcpyHostToDevice, h.s_in));
                STEP(hipMemcpyAsync(h.d_rin[b] + rin_len, h_R + rp.src0, rp.src_len * sizeof(float), hipMemcpyHostToDevice, h.s_in));
            }
        } else if (ns && inq) STEP(hipMemcpyAsync(h.d_inq[b], (const char*)h_in + ib * s0, ns * ib, hipMemcpyHostToDevice, h.s_in));
        else if (ns) {
            STEP(hipMemcpyAsync(h.d_in[b], h_L + s0, ns * sizeof(float), hipMemcpyHostToDevice, h.s_in));
            STEP(hipMemcpyAsync(h.d_in[b] + in_cap, h_R + s0, ns * sizeof(float), hipMemcpyHostToDevice, h.s_in));
        }
        STEP(hipEventRecord(h.ev_in[b], h.s_in));
        // compute: needs this chunk's PCM and the output buffer drained by the download of two chunks ago
        STEP(hipStreamWaitEvent(e->stream, h.ev_in[b], 0));
        if (c >= 2) STEP(hipStreamWaitEvent(e->stream, h.ev_out[b], 0));
        if (er != hipSuccess) break;
        if (inq && fin && rp.src_len) {
            if ((rc = host_unpack(e, f, h.d_inq[b], rp.src_len, h.d_rin[b], h.d_rin[b] + rin_len))) break;
        } else if (inq && ns && !fin) {
            if ((rc = host_unpack(e, f, h.d_inq[b], ns, h.d_in[b], h.d_in[b] + in_cap))) break;
        }
        if (fin && ns) {                                    // the piece's 44.1 kHz samples [s0, s0 + ns) from the source window: one span, one pair
            TimerScope ts(e, "rate_in");
            const SrtRsSpans sp = { 1, h.d_rin[b], rin_len, (long long)rp.src0, rp.src_len, nullptr, 0, 0, n_host, s0, ns, h.d_in[b], in_cap };
            if ((rc = srt_rs_spans_launch(*fin, sp, e->stream, who))) break;
        }
        if (O) {
            const HostOvPiece hp = { pc.tiles, pc.own_rows, pc.stft_rows, c ? h.d_mseam : nullptr };
            rc = separate_piece(e, sw, o, h.d_in[b], h.d_in[b] + in_cap, ns, cfr, hp, c + 1 < nchunks ? h.d_mseam : nullptr, h.d_out[b]);
        } else
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
        const size_t nj = rp.out1 - rp.out0;
        if (fout) {
            // output frames [out0, out1) of every pair in one launch: span A the carry (samples [fin0 - K, fin0); before the first piece nothing of it is read - those
            // positions are negative), span B the samples this piece has finalised, [fin0, fin0 + take)
            if (nj) {
                TimerScope ts(e, "rate_out");
                const SrtRsSpans sp = { S, h.d_rcarry, K, (long long)rp.fin0 - (long long)K, K, h.d_out[b], clen, take, total_len, rp.out0, nj, h.d_rout[b], rout_len };
                if ((rc = srt_rs_spans_launch(*fout, sp, e->stream, who))) break;
            }
            // then the piece's last K finalised samples become the carry (ordered behind the launch that read it)
            if (c + 1 < nchunks) STEP(hipMemcpy2DAsync(h.d_rcarry, K * sizeof(float), h.d_out[b] + take - K, clen * sizeof(float), K * sizeof(float), NP, hipMemcpyDeviceToDevice, e->stream));
            if (er != hipSuccess) break;
        }
        // (the dither's index is the sample's position in the whole output plane: the converted frames start at out0, the chunk's own at s0)
        if (outq && fout && nj) {
            if ((rc = host_pack(e, f, o, h.d_rout[b], rout_len, S, nj, h.d_outq[b], d_clip, rp.out0))) break;
        } else if (outq && !fout) {
            if ((rc = host_pack(e, f, o, h.d_out[b], clen, S, take, h.d_outq[b], d_clip, s0))) break;
        }
        STEP(hipEventRecord(h.ev_cmp[b], e->stream));
        // download: every plane's [0, crow*1024) (+ the final 3072 on the last chunk) lands at its place in h_out
        STEP(hipStreamWaitEvent(h.s_out, h.ev_cmp[b], 0));
        if (fout) {                                         // the converted planes: frames [out0, out1) of planes of out_len, one contiguous copy per plane (a pitched 2-D
                                                            // copy of this size slowed the next piece's first kernels and the copy itself: DESIGN.md 8.1)
            for (int p = 0; nj && outq && p < S; ++p) STEP(hipMemcpyAsync((char*)h_out_ + ob * ((size_t)p * out_len + rp.out0), (const char*)h.d_outq[b] + ob * (size_t)p * rout_len, nj * ob, hipMemcpyDeviceToHost, h.s_out));
            for (int p = 0; nj && !outq && p < NP; ++p) STEP(hipMemcpyAsync(h_out + (size_t)p * out_len + rp.out0, h.d_rout[b] + (size_t)p * rout_len, nj * sizeof(float), hipMemcpyDeviceToHost, h.s_out));
        } else if (outq) STEP(hipMemcpy2DAsync((char*)h_out_ + ob * s0, total_len * ob, h.d_outq[b], clen * ob, take * ob, S, hipMemcpyDeviceToHost, h.s_out));
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

int srtSeparateHostStreamOverlap(srt_engine* e, const void* h_in, const void* h_in2, size_t n, int overlap_rows, void* h_out, unsigned flags, unsigned long long* h_clipped)
{
    static const char* const who = "srtSeparateHostStreamOverlap";
    if (!e || !h_in || !h_out) return fail(-1, "%s: null argument", who);
    if (flags & ~SRT_HOST_FLAGS) return fail(-1, "%s: unknown flag bits", who);
    if (n < SRT_FFT) return fail(-1, "%s: need at least 4096 samples", who);
    if (overlap_rows < 0) return fail(-1, "%s: overlap_rows must be 0 .. T / 2", who);
    if (srtStftRows(n) > (size_t)0x7fffffff - 4) return fail(-1, "%s: more than 2^31 rows", who);
    return host_stream(e, h_in, h_in2, n, srtStftFrames(n), srtStftRows(n), h_out, flags, 0, SrtSeam{0, nullptr, false}, h_clipped, overlap_rows);
}

// the engine's converter of a rate pair (built-in filter): built on the first call that needs it, kept until srtDestroy
static int rate_filter(srt_engine* e, int fs_in, int fs_out, const SrtRsGeom& g, const char* who, const SrtRsFilter** out)
{
    for (const auto& rf : e->rate_filters) if (rf.fs_in == fs_in && rf.fs_out == fs_out) { *out = &rf.f; return 0; }
    srt_engine::RateFilter rf;
    rf.fs_in = fs_in; rf.fs_out = fs_out;
    if (const int rc = srt_rs_filter_create(g, nullptr, 0, e->stream, who, &rf.f)) return rc;
    e->rate_filters.push_back(rf);                              // (a deque: the filters handed out earlier stay where they are)
    *out = &e->rate_filters.back().f;
    return 0;
}

int srtSeparateHostStreamRate(srt_engine* e, const void* h_in, const void* h_in2, size_t n, int in_rate, int out_rate, int overlap_rows, void* h_out, unsigned flags,
                              unsigned long long* h_clipped)
{
    static const char* const who = "srtSeparateHostStreamRate";
    if (flags & ~SRT_HOST_FLAGS) return fail(-1, "%s: unknown flag bits", who);
    HostFmt f;
    if (const int rc = host_fmt(flags, h_in2, who, &f)) return rc;
    if (!e || !h_in || !h_out || (!f.pcm_in() && !h_in2)) return fail(-1, "%s: null argument", who);
    HostRateDims d;
    if (const int rc = host_rate_dims(n, in_rate, out_rate, who, &d)) return rc;
    if (!overlap_ok(overlap_rows, e->cfg.T)) return fail(-1, "%s: overlap_rows must be 0 .. T / 2", who);
    if (engine_opts(e).wiener) return fail(-1, "%s: the Wiener filter's statistics span the whole signal (chunks would each get their own covariance): srtSetWiener(e, 0) first", who);
    for (int s = 0; s < e->cfg.n_stems; ++s) if (!e->have_coeff[s]) return fail(-5, "%s: weights not set for every stem", who);
    HostRate rate = { n, nullptr, nullptr, d.len_out };
    {
        DeviceScope ds(e->device);
        if (d.cin) if (const int rc = rate_filter(e, in_rate, 44100, d.gi, who, &rate.fin)) return rc;
        if (d.cout) if (const int rc = rate_filter(e, 44100, out_rate, d.go, who, &rate.fout)) return rc;
    }
    return host_stream(e, h_in, h_in2, d.n44, srtStftFrames(d.n44), d.rows, h_out, flags, 0, SrtSeam{0, nullptr, false}, h_clipped, overlap_rows, &rate);
}

// ------------------------------------------------------------------------------------------- the Wiener filter over a host stream of any length
// The filter's statistics span the whole signal, so the stream is walked twice.  Sweep A is host_stream's upload pipeline: a piece (max_tiles tiles) goes up, its
// STFT and fp32 masks are written into a device store that holds them for the WHOLE stream, and pass 1 of the statistics runs over it.  Passes 2.. walk the store
// alone.  Sweep B filters one piece at a time into the engine's spectrum workspace, inverts it, adds the 3072-sample seam (srt_launch_carry) and sends the piece
// down on host_stream's download pipeline.  Nothing crosses PCIe twice, and the network runs once.

// the store: piece c at c * piece_bytes - its spectrum [2][stft_rows][SRT_SPEC_LD] float2, then its masks [n_stems][tiles][2][T][F] floats, then (under an overlap, every
// piece but the last) its mask seam carry [n_stems][2][O][F] floats.  The pieces are host_ov_piece's: every piece but the last is full - max_tiles tiles over
// (max_tiles - 1) (T - O) + T spectrum rows, O of them the look-ahead rows the next piece owns and holds again - the last one has its own row and tile count.
// O = 0: max_tiles * T rows a piece and no carry, srtSeparateHostWiener's store.
struct HostWienerLayout { size_t ntiles, npieces, piece_bytes, total; int O; };
static size_t wstore_spec_bytes(size_t crow) { return 2 * crow * SRT_SPEC_LD * sizeof(float2); }
static size_t wstore_mask_bytes(const srt_config& cfg, size_t tiles) { return (size_t)cfg.n_stems * tiles * 2 * cfg.T * cfg.F * sizeof(float); }
static size_t wstore_seam_bytes(const srt_config& cfg, int O) { return (size_t)cfg.n_stems * 2 * O * cfg.F * sizeof(float); }
static HostWienerLayout host_wiener_layout(const srt_config& cfg, size_t rows, int O)
{
    HostWienerLayout l;
    l.O = O;
    l.ntiles = overlap_tiles(rows, cfg.T, O);
    l.npieces = (l.ntiles + cfg.max_tiles - 1) / cfg.max_tiles;
    l.piece_bytes = wstore_spec_bytes((size_t)(cfg.max_tiles - 1) * (cfg.T - O) + cfg.T) + wstore_mask_bytes(cfg, (size_t)cfg.max_tiles) + wstore_seam_bytes(cfg, O);
    const srt_host_piece last = host_ov_piece(rows, cfg.T, O, cfg.max_tiles, l.ntiles, l.npieces - 1);
    l.total = (l.npieces - 1) * l.piece_bytes + wstore_spec_bytes(last.stft_rows) + wstore_mask_bytes(cfg, last.tiles);
    return l;
}
static HostWienerPiece host_wiener_piece(const srt_config& cfg, const HostWienerLayout& l, char* store, size_t rows, size_t c)
{
    const srt_host_piece hp = host_ov_piece(rows, cfg.T, l.O, cfg.max_tiles, l.ntiles, c);
    HostWienerPiece pc;
    pc.row0 = hp.row0; pc.rows = hp.own_rows; pc.stft_rows = hp.stft_rows; pc.ntiles = (int)hp.tiles;
    char* const base = store + c * l.piece_bytes;
    pc.spec = (float2*)base;
    pc.masks = (float*)(base + wstore_spec_bytes(pc.stft_rows));      // (a multiple of 16 bytes, as the carry behind it: the mask extension's kernel reads vectors)
    pc.seam_out = l.O && c + 1 < l.npieces ? (float*)((char*)pc.masks + wstore_mask_bytes(cfg, hp.tiles)) : nullptr;
    pc.seam = l.O && c ? (const float*)(base - wstore_seam_bytes(cfg, l.O)) : nullptr;      // the slot that closes the (full) piece before this one
    return pc;
}

size_t srtHostWienerBytes(const srt_config* cfg, size_t n)
{
    if (!cfg) { fail(-1, "srtHostWienerBytes: null config"); return 0; }
    if (srt_check_config(cfg, "srtHostWienerBytes")) return 0;
    if (n < SRT_FFT) { fail(-1, "srtHostWienerBytes: need at least 4096 samples"); return 0; }
    return host_wiener_layout(*cfg, srtStftRows(n), 0).total;
}

size_t srtHostWienerOverlapBytes(const srt_config* cfg, size_t n, int overlap_rows)
{
    if (!cfg) { fail(-1, "srtHostWienerOverlapBytes: null config"); return 0; }
    if (srt_check_config(cfg, "srtHostWienerOverlapBytes")) return 0;
    if (n < SRT_FFT) { fail(-1, "srtHostWienerOverlapBytes: need at least 4096 samples"); return 0; }
    if (!overlap_ok(overlap_rows, cfg->T)) { fail(-1, "srtHostWienerOverlapBytes: overlap_rows must be 0 .. T / 2"); return 0; }
    return host_wiener_layout(*cfg, srtStftRows(n), overlap_rows).total;
}

// grow-only like the rest of the staging (the streams exist: ensure_staging ran).  A failed allocation leaves the engine without a store and otherwise as it was.
static int ensure_wstore(srt_engine* e, size_t bytes, bool ov)
{
    HostStaging& h = e->hs;
    if (bytes <= h.wstore_cap) return 0;
    HIPCHK(hipStreamSynchronize(h.s_in)); HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipStreamSynchronize(h.s_out));
    if (h.d_wstore) { hipFree(h.d_wstore); h.d_wstore = nullptr; h.wstore_cap = 0; }
    const hipError_t er = hipMalloc((void**)&h.d_wstore, bytes);
    if (er != hipSuccess) {
        (void)hipGetLastError();
        h.d_wstore = nullptr;
        char what[160];
        snprintf(what, sizeof what, "%zu bytes (%s)", bytes, hipGetErrorString(er));
        return ov ? fail(-2, "srtSeparateHostWienerOverlap: HIP error allocating the device store of %s: srtHostWienerOverlapBytes gives its size; a shorter stream, a smaller overlap or fewer stems fit", what)
                  : fail(-2, "srtSeparateHostWiener: HIP error allocating the device store of %s: srtHostWienerBytes gives its size; a shorter stream or fewer stems fit", what);
    }
    h.wstore_cap = bytes;
    return 0;
}

// ov: srtSeparateHostWienerOverlap - the call takes opts->overlap_rows and names itself in every text.  The pieces are host_ov_piece's under the call's
// overlap O: a piece uploads and analyses stft_rows rows into the overlapped layout of its own tiles, and only the rows it owns enter the statistics, the filter, the
// inverse and the download; the first O rows of a later piece blend with the carry the piece before it left in the store (srt_mask_seam_save_kernel).  At O = 0 the
// pieces are max_tiles * T rows each and every launch is srtSeparateHostWiener's.
static int host_wiener(srt_engine* e, const void* h_in, const void* h_in2, size_t n, const srt_wiener_opts* opts, void* h_out_, unsigned flags, unsigned long long* h_clipped, bool ov)
{
    const char* const who = ov ? "srtSeparateHostWienerOverlap" : "srtSeparateHostWiener";
    if (flags & ~SRT_HOST_FLAGS) return fail(-1, "%s: unknown flag bits", who);
    HostFmt f;
    if (const int frc = host_fmt(flags, h_in2, who, &f)) return frc;
    const bool inq = f.pcm_in(), outq = f.pcm_out();
    const size_t ib = f.in_bytes(), ob = f.out_bytes();
    if (!e || !h_in || (!inq && !h_in2) || !opts || !h_out_) return fail(-1, "%s: null argument", who);
    DeviceScope ds(e->device);
    SepOpts o;
    int rc = host_wiener_check(e, opts, n, &o, ov);
    if (rc) return rc;
    o.dither_seed = e->dither_seed;                     // the call's options come from `opts`; the seed is the engine's (srtSetDitherSeed)
    if (stream_capturing(e)) return fail(-1, "%s: not available inside a stream capture (the call is synchronous and allocates)", who);
    const size_t rows = srtStftRows(n), frames = srtStftFrames(n);
    const int S = e->cfg.n_stems, NO = o.n_out ? o.n_out : S, NP = NO * 2, iters = o.wiener, O = o.overlap;      // NO pairs staged, carried, packed and downloaded
    const HostWienerLayout l = host_wiener_layout(e->cfg, rows, O);
    const size_t tail = SRT_FFT - SRT_HOP, total_len = srtIstftLength(rows);
    // a full piece analyses (max_tiles - 1) (T - O) + T rows; the LAST piece may own that many too (its last tile has no successor to hand its last O rows to)
    const size_t span = (size_t)(e->cfg.max_tiles - 1) * (e->cfg.T - O) + e->cfg.T;
    const size_t in_cap = span * SRT_HOP + tail, out_cap = srtIstftLength(span);
    if ((rc = host_wiener_ws(e, o, who))) return rc;
    if ((rc = ensure_staging(e, 2 * in_cap, (size_t)NP * out_cap, (size_t)NP * tail, 2))) return rc;
    if ((inq || outq) && (rc = ensure_staging_pcm(e, inq ? ib * in_cap : 0, outq ? ob * NO * out_cap : 0))) return rc;
    if ((rc = ensure_wstore(e, l.total, ov))) return rc;
    HostStaging& h = e->hs;
    if (h_clipped) memset(h_clipped, 0, (size_t)NO * sizeof *h_clipped);
    unsigned long long* d_clip = outq && h_clipped ? h.d_clip : nullptr;
    if (d_clip) HIPCHK(hipMemsetAsync(d_clip, 0, (size_t)NO * sizeof *d_clip, e->stream));
    bool pinL = false, pinR = false, pinO = false;                  // as host_stream: register the caller's buffers for the call unless they are pinned already
    if (!(flags & SRT_HOST_PINNED)) {
        pinL = hipHostRegister((void*)h_in, n * (inq ? ib : sizeof(float)), hipHostRegisterDefault) == hipSuccess;       // (int16 [n][2] is n * 4 bytes too)
        pinR = !inq && hipHostRegister((void*)h_in2, n * sizeof(float), hipHostRegisterDefault) == hipSuccess;
        pinO = hipHostRegister(h_out_, (size_t)NO * total_len * ob, hipHostRegisterDefault) == hipSuccess;
        (void)hipGetLastError();
    }
    const float *h_L = (const float*)h_in, *h_R = (const float*)h_in2;
    const SrtSwitches sw = srt_read_switches();
    const SrtWienerParams w = wiener_geometry(e, rows);      // the chunks and the tables of the WHOLE signal
    hipError_t er = hipSuccess;
#define STEP(x) do { if (er == hipSuccess) er = (x); } while (0)
    // sweep A: upload, unpack, STFT and networks into the store, statistics pass 1
    for (size_t c = 0; c < l.npieces && er == hipSuccess && rc == 0; ++c) {
        const int b = (int)(c & 1);
        const HostWienerPiece pc = host_wiener_piece(e->cfg, l, h.d_wstore, rows, c);
        const size_t row1 = pc.row0 + pc.stft_rows;                          // rows [row0, row1) go up and are analysed
        const size_t s0 = pc.row0 * SRT_HOP, send = row1 * SRT_HOP + tail < n ? row1 * SRT_HOP + tail : n;
        const size_t ns = send > s0 ? send - s0 : 0;
        const size_t cfr = frames > pc.row0 ? (frames - pc.row0 < pc.stft_rows ? frames - pc.row0 : pc.stft_rows) : 0;
        if (c >= 2) STEP(hipStreamWaitEvent(h.s_in, h.ev_cmp[b], 0));      // the input buffer is free once the transform that read it two pieces ago has finished
        if (ns && inq) STEP(hipMemcpyAsync(h.d_inq[b], (const char*)h_in + ib * s0, ns * ib, hipMemcpyHostToDevice, h.s_in));
        else if (ns) {
            STEP(hipMemcpyAsync(h.d_in[b], h_L + s0, ns * sizeof(float), hipMemcpyHostToDevice, h.s_in));
            STEP(hipMemcpyAsync(h.d_in[b] + in_cap, h_R + s0, ns * sizeof(float), hipMemcpyHostToDevice, h.s_in));
        }
        STEP(hipEventRecord(h.ev_in[b], h.s_in));
        STEP(hipStreamWaitEvent(e->stream, h.ev_in[b], 0));
        if (er != hipSuccess) break;
        if (inq && ns && (rc = host_unpack(e, f, h.d_inq[b], ns, h.d_in[b], h.d_in[b] + in_cap))) break;
        if ((rc = host_wiener_analyse(e, sw, h.d_in[b], h.d_in[b] + in_cap, ns, cfr, pc, O))) break;
        STEP(hipEventRecord(h.ev_cmp[b], e->stream));                       // (the networks read the magnitudes, not the PCM, but the event is one per piece)
        if ((rc = host_wiener_stats(e, w, pc, 1, O))) break;
    }
    // the R tables: pass 1, then every further pass over the store (no network, no PCIe)
    if (rc == 0 && er == hipSuccess) rc = host_wiener_finalize(e, w, 1);
    for (int pass = 2; pass <= iters && rc == 0 && er == hipSuccess; ++pass) {
        for (size_t c = 0; c < l.npieces && rc == 0; ++c) rc = host_wiener_stats(e, w, host_wiener_piece(e->cfg, l, h.d_wstore, rows, c), pass, O);
        if (rc == 0) rc = host_wiener_finalize(e, w, pass);
    }
    // sweep B: filter, inverse transforms, seam, pack, download
    for (size_t c = 0; c < l.npieces && er == hipSuccess && rc == 0; ++c) {
        const int b = (int)(c & 1);
        const HostWienerPiece pc = host_wiener_piece(e->cfg, l, h.d_wstore, rows, c);
        const size_t s0 = pc.row0 * SRT_HOP, clen = srtIstftLength(pc.rows);
        const bool last = c + 1 == l.npieces;
        if (c >= 2) STEP(hipStreamWaitEvent(e->stream, h.ev_out[b], 0));    // the output buffer is free once the download of two pieces ago has drained it
        if (er != hipSuccess) break;
        if ((rc = host_wiener_render(e, w, o, pc, h.d_out[b]))) break;
        if (srt_launch_carry(h.d_out[b], clen, NP, pc.rows * SRT_HOP, h.d_carry, c == 0, last, e->stream)) { rc = fail(-2, "carry launch failed"); break; }
        const size_t take = last ? clen : pc.rows * SRT_HOP;
        if (outq && (rc = host_pack(e, f, o, h.d_out[b], clen, NO, take, h.d_outq[b], d_clip, s0))) break;
        STEP(hipEventRecord(h.ev_cmp[b], e->stream));
        STEP(hipStreamWaitEvent(h.s_out, h.ev_cmp[b], 0));
        if (outq) STEP(hipMemcpy2DAsync((char*)h_out_ + ob * s0, total_len * ob, h.d_outq[b], clen * ob, take * ob, NO, hipMemcpyDeviceToHost, h.s_out));
        else STEP(hipMemcpy2DAsync((float*)h_out_ + s0, total_len * sizeof(float), h.d_out[b], clen * sizeof(float), take * sizeof(float), NP, hipMemcpyDeviceToHost, h.s_out));
        STEP(hipEventRecord(h.ev_out[b], h.s_out));
    }
#undef STEP
    hipStreamSynchronize(h.s_in);
    hipStreamSynchronize(e->stream);
    hipStreamSynchronize(h.s_out);
    if (rc == 0 && er == hipSuccess && d_clip) {      // once, after the last piece
        er = hipMemcpyAsync(h_clipped, d_clip, (size_t)NO * sizeof *d_clip, hipMemcpyDeviceToHost, e->stream);
        if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    }
    if (rc == 0 && er != hipSuccess) rc = fail(-2, "HIP error: %s", hipGetErrorString(er));
    if (pinL) hipHostUnregister((void*)h_in);
    if (pinR) hipHostUnregister((void*)h_in2);
    if (pinO) hipHostUnregister(h_out_);
    return rc;
}

int srtSeparateHostWiener(srt_engine* e, const void* h_in, const void* h_in2, size_t n, const srt_wiener_opts* opts, void* h_out, unsigned flags, unsigned long long* h_clipped)
{
    return host_wiener(e, h_in, h_in2, n, opts, h_out, flags, h_clipped, false);
}

int srtSeparateHostWienerOverlap(srt_engine* e, const void* h_in, const void* h_in2, size_t n, const srt_wiener_opts* opts, void* h_out, unsigned flags, unsigned long long* h_clipped)
{
    return host_wiener(e, h_in, h_in2, n, opts, h_out, flags, h_clipped, true);
}
