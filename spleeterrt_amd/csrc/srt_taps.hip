// srt_taps.hip — the debug taps and the per-launch timers of the engine: srtCopyTensor, srtSetTiming, srtGetTiming, srtGetTimingKernels (its private declarations: srt_engine.h).
#include "srt_engine.h"
#include <cxxabi.h>

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
