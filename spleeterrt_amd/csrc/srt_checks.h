// srt_checks.h — the range predicates of the separation options, shared by the engine units (srt_engine.h) and the live streams (srt_stream.hip).
// They decide only; every caller keeps its own error code and text.
#pragma once
#include "../../include/spleeterrt_amd.h"
#include <math.h>

static inline bool overlap_ok(int overlap_rows, int T) { return overlap_rows >= 0 && overlap_rows <= T / 2; }     // rows two consecutive tiles may share
static inline bool mask_ext_ok(int mode) { return mode == SRT_MASK_EXT_CONSTANT || mode == SRT_MASK_EXT_AVERAGE; }
static inline bool gain_finite(const float* g, int n) { for (int i = 0; i < n; ++i) if (!isfinite(g[i])) return false; return true; }
