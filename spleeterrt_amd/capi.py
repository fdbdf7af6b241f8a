"""ctypes binding of include/spleeterrt_amd.h.  Fails loudly if the HIP library is missing — there is no CPU path."""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(PKG, "libspleeterrt_amd.so")
MAX_STEMS = 8
VARIANT_EXE, VARIANT_VST = 0, 1
IMPL_MFMA, IMPL_NAIVE = 0, 1
PREC_F32, PREC_F16, PREC_F16X2 = 0, 1, 2
MASK_EXT_CONSTANT, MASK_EXT_AVERAGE = 0, 1                 # SRT_MASK_EXT_* (srtSetMaskExtension)
HOST_PINNED, HOST_IN_PCM16, HOST_OUT_PCM16 = 1, 2, 4      # SRT_HOST_* (srtSeparateHostStreamIo / srtSeparateCliHostIo)
HOST_IN_PCM24, HOST_OUT_PCM24, HOST_OUT_DITHER = 16, 32, 64   # ... 24-bit packed PCM and the dithered 16-bit output
COEFF_FLOATS = 9822725
SPEC_LD = 2052


class EngineError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("F", C.c_int), ("T", C.c_int), ("n_stems", C.c_int), ("stem_mode", C.c_int * MAX_STEMS),
                ("oob_weight", C.c_float * MAX_STEMS), ("variant", C.c_int), ("max_tiles", C.c_int), ("impl", C.c_int), ("precision", C.c_int),
                ("ratio_mask", C.c_int), ("batch_invariant", C.c_int)]


class _LiveOpts(C.Structure):
    """srt_live_opts (include/spleeterrt_amd.h): the options of srtLiveCreateEx"""
    _fields_ = [("sample_rate", C.c_int), ("max_block", C.c_int), ("n_out", C.c_int), ("h_gain", C.POINTER(C.c_float)), ("mask_extension", C.c_int)]


class _WienerOpts(C.Structure):
    """srt_wiener_opts (include/spleeterrt_amd.h): the per-call options of srtIstftWienerEx / srtSeparateWiener"""
    _fields_ = [("iterations", C.c_int), ("overlap_rows", C.c_int), ("mask_extension", C.c_int), ("n_out", C.c_int), ("h_gain", C.POINTER(C.c_float))]


class _BatchWienerOpts(C.Structure):
    """srt_batch_wiener_opts (include/spleeterrt_amd.h): the per-call options of srtSeparateBatchWienerEx"""
    _fields_ = [("iterations", C.c_int), ("overlap_rows", C.c_int), ("mask_extension", C.c_int), ("n_out", C.c_int), ("h_gain", C.POINTER(C.c_float)),
                ("gain_stride", C.c_size_t)]


class Span(C.Structure):
    """srt_span (include/spleeterrt_amd.h): one rank's share of a stream, as srtRankSpan fills it."""
    _fields_ = [(k, C.c_size_t) for k in ("tile0", "tile1", "sample0", "nsamples", "frames", "rows", "out_offset")]


_lib = None


def load_library():
    """dlopen libspleeterrt_amd.so.  torch is imported first so both share one HIP runtime (same SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    so = os.environ.get("SPLEETERRT_LIB") or SO           # SPLEETERRT_LIB: the -DSRT_TUNING measurement build (scripts/gpu_tune.sh)
    if not os.path.exists(so):
        raise EngineError("%s not built: run `python -m spleeterrt_amd.build` (needs hipcc); no CPU fallback exists" % so)
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    L = C.CDLL(so)
    vp, f32p = C.c_void_p, C.c_void_p
    L.srtCreate.argtypes = [C.POINTER(_Config), vp, C.POINTER(vp)]
    L.srtDestroy.argtypes = [vp]
    L.srtDestroy.restype = None
    L.srtLastError.restype = C.c_char_p
    L.srtCoeffBytes.restype = C.c_size_t
    L.srtSetCoeffHost.argtypes = [vp, C.c_int, vp]
    L.srtSetCoeffDevice.argtypes = [vp, C.c_int, vp]
    L.srtSetCoeffFp16Host.argtypes = [vp, C.c_int, vp]
    L.srtGetCoeffHost.argtypes = [vp, C.c_int, vp]
    L.srtForward.argtypes = [vp, f32p, C.c_int, f32p]
    L.srtForwardStems.argtypes = [vp, f32p, C.c_int, f32p, C.c_int, C.c_int]
    L.srtRatioMask.argtypes = [vp, f32p, C.c_int]
    L.srtSetWiener.argtypes = [vp, C.c_int]
    L.srtSetOverlap.argtypes = [vp, C.c_int]
    L.srtSetMaskExtension.argtypes = [vp, C.c_int]
    L.srtSetMix.argtypes = [vp, C.c_int, vp]
    L.srtMixOutputs.argtypes = [vp]
    L.srtOverlapTiles.restype = C.c_size_t
    L.srtOverlapTiles.argtypes = [C.c_size_t, C.c_int, C.c_int]
    L.srtIstftWiener.argtypes = [vp, f32p, C.c_size_t, f32p, C.c_int, f32p]
    L.srtIstftWienerEx.argtypes = [vp, f32p, C.c_size_t, f32p, C.POINTER(_WienerOpts), f32p]
    L.srtSeparateWiener.argtypes = [vp, f32p, f32p, C.c_size_t, C.POINTER(_WienerOpts), f32p]
    L.srtSeparateHostWiener.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(_WienerOpts), vp, C.c_uint, vp]
    L.srtHostWienerBytes.restype = C.c_size_t
    L.srtHostWienerBytes.argtypes = [C.POINTER(_Config), C.c_size_t]
    L.srtSeparateHostWienerOverlap.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(_WienerOpts), vp, C.c_uint, vp]
    L.srtHostWienerOverlapBytes.restype = C.c_size_t
    L.srtHostWienerOverlapBytes.argtypes = [C.POINTER(_Config), C.c_size_t, C.c_int]
    L.srtSeparateCli.argtypes = [vp, f32p, f32p, C.c_size_t, C.c_int, f32p]
    L.srtSeparateCliHost.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp]
    L.srtSeparateHostStream.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp]
    L.srtSeparateHostStreamEx.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.c_uint]
    L.srtSeparateHostStreamIo.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.c_uint, vp]
    L.srtSeparateCliHostIo.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp, C.c_uint, vp]
    L.srtSeparateHostStreamOverlap.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp, C.c_uint, vp]
    L.srtHostOverlapPieces.restype = C.c_size_t
    L.srtHostOverlapPieces.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_size_t]
    L.srtSeparateHostStreamRate.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_uint, vp]
    L.srtHostRateLength.restype = C.c_size_t
    L.srtHostRateLength.argtypes = [C.c_size_t, C.c_int, C.c_int]
    L.srtHostRatePieces.restype = C.c_size_t
    L.srtHostRatePieces.argtypes = [C.POINTER(_Config), C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_size_t]
    L.srtPcm16Unpack.argtypes = [vp, vp, C.c_size_t, vp, vp]
    L.srtPcm16Pack.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_size_t, vp, C.c_size_t, vp]
    L.srtPcm24Unpack.argtypes = [vp, vp, C.c_size_t, vp, vp]
    L.srtPcm24Pack.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_size_t, vp, C.c_size_t, vp]
    L.srtPcm16PackDither.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_size_t, vp, C.c_size_t, vp, C.c_uint64, C.c_int, C.c_uint64]
    L.srtSetDitherSeed.argtypes = [vp, C.c_uint64]
    for fn in (L.srtStftRows, L.srtStftFrames, L.srtIstftLength):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_size_t]
    L.srtStft.argtypes = [vp, f32p, f32p, C.c_size_t, f32p, f32p]
    L.srtIstft.argtypes = [vp, f32p, C.c_size_t, f32p, f32p]
    L.srtSeparate.argtypes = [vp, f32p, f32p, C.c_size_t, f32p]
    L.srtStftEx.argtypes = [vp, f32p, f32p, C.c_size_t, C.c_size_t, C.c_size_t, f32p, f32p]
    L.srtSeparateEx.argtypes = [vp, f32p, f32p, C.c_size_t, C.c_size_t, C.c_size_t, f32p]
    L.srtCopyTensor.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, vp, C.c_size_t]
    L.srtBatchPlan.argtypes = [C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.srtSeparateBatch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]
    L.srtSeparateBatchWiener.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp), C.c_int]
    L.srtBatchPlanOverlap.argtypes = [C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.srtSeparateBatchOverlap.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp), C.c_int]
    L.srtSeparateBatchWienerEx.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(_BatchWienerOpts)]
    L.srtSeparateBatchMix.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_size_t]
    L.srtSetGraphMode.argtypes = [vp, C.c_int]
    L.srtPrepareForward.argtypes = [vp, f32p, C.c_int, f32p]
    L.srtReleaseStaging.argtypes = [vp]
    L.srtSetTiming.argtypes = [vp, C.c_int]
    L.srtGetTiming.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_float), C.c_int]
    L.srtGetTimingKernels.argtypes = [vp, C.c_char_p, C.c_size_t]
    # multi-device host driver (csrc/srt_multi.hip)
    L.srtRankSpan.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(Span)]
    L.srtMultiCreate.argtypes = [C.POINTER(_Config), C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.srtMultiDestroy.argtypes = [vp]
    L.srtMultiDestroy.restype = None
    L.srtMultiSetCoeffHost.argtypes = [vp, C.c_int, vp]
    L.srtMultiSetCoeffFp16Host.argtypes = [vp, C.c_int, vp]
    L.srtMultiSeparateHost.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_uint]
    L.srtMultiSeparateCliHost.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp]
    L.srtMultiInfo.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.srtMultiEngine.argtypes = [vp, C.c_int]
    L.srtMultiEngine.restype = vp
    L.srtMultiBenchResident.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    # live separation with a sliding network window (csrc/srt_stream.hip)
    L.srtLiveCreate.argtypes = [C.POINTER(_Config), C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.srtLiveProcess.argtypes = [vp, vp, vp, C.c_int, C.POINTER(vp)]
    L.srtLiveLatency.argtypes = [vp]
    L.srtLiveDestroy.argtypes = [vp]
    L.srtLiveDestroy.restype = None
    L.srtLiveCreateRate.argtypes = [C.POINTER(_Config), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.srtLiveRateLatency.argtypes = [C.c_int, C.c_int, C.c_int]
    L.srtLiveCreateEx.argtypes = [C.POINTER(_Config), C.c_int, C.c_int, C.POINTER(_LiveOpts), C.POINTER(vp), C.POINTER(vp)]
    L.srtLiveSetMix.argtypes = [vp, vp]
    L.srtLiveOutputs.argtypes = [vp]
    L.srtLiveCreateWiener.argtypes = [C.POINTER(_Config), C.c_int, C.c_int, C.POINTER(_LiveOpts), C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.srtLiveWiener.argtypes = [vp]
    L.srtLiveCopyTensor.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_longlong)]
    # sample-rate converter (csrc/srt_resample.hip)
    L.srtResampleLength.restype = C.c_size_t
    L.srtResampleLength.argtypes = [C.c_size_t, C.c_int, C.c_int]
    L.srtResamplerCreate.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.srtResamplerDestroy.argtypes = [vp]
    L.srtResample.argtypes = [vp, f32p, f32p, C.c_size_t, C.c_size_t, C.c_size_t, f32p, f32p]
    L.srtResampleHost.argtypes = [vp, vp, vp, C.c_size_t, vp, vp]
    L.srtResampleSpans.argtypes = [vp, C.c_int, f32p, C.c_size_t, C.c_longlong, C.c_size_t, f32p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, f32p, C.c_size_t]
    # the converter as a stream (csrc/srt_rsstream.hip)
    L.srtResampleHorizon.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.srtResampleComputable.restype = C.c_longlong
    L.srtResampleComputable.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong]
    L.srtResamplerStreamCreate.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.srtResamplerStreamProcess.argtypes = [vp, f32p, C.c_size_t, C.c_int, f32p, C.c_size_t]
    L.srtResamplerStreamFlush.argtypes = [vp, f32p, C.c_size_t]
    L.srtResamplerStreamReset.argtypes = [vp]
    L.srtResamplerStreamHorizon.argtypes = [vp]
    L.srtResamplerStreamDestroy.argtypes = [vp]
    _lib = L
    return L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Engine:
    """One engine per (device, stream): nstems sub-networks evaluated over batches of T x F spectrogram tiles."""

    def __init__(self, F=1024, T=256, stem_modes=(1, 1, 1, 1), oob_weights=None, variant=VARIANT_EXE, max_tiles=1,
                 impl=IMPL_MFMA, device=None, precision=PREC_F32, ratio_mask=False, batch_invariant=False, wiener=0, overlap=0,
                 mask_extension="constant"):
        import torch
        if not torch.cuda.is_available():
            raise EngineError("no GPU visible: spleeterrt_amd has no CPU path")
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        torch.cuda.set_device(self.device)
        self.L = load_library()
        self.F, self.T, self.S, self.max_tiles, self.variant = F, T, len(stem_modes), max_tiles, variant
        cfg = _Config()
        cfg.F, cfg.T, cfg.n_stems, cfg.variant, cfg.max_tiles, cfg.impl = F, T, self.S, variant, max_tiles, impl
        cfg.precision = precision
        cfg.ratio_mask = int(bool(ratio_mask))
        cfg.batch_invariant = int(bool(batch_invariant))
        for i, m in enumerate(stem_modes):
            cfg.stem_mode[i] = int(m)
            cfg.oob_weight[i] = 0.1 if oob_weights is None else float(oob_weights[i])
        self.stream = torch.cuda.current_stream(self.device)
        h = C.c_void_p()
        self._chk(self.L.srtCreate(C.byref(cfg), C.c_void_p(self.stream.cuda_stream), C.byref(h)))
        self.h = h
        self._cfg = cfg
        self.wiener = 0
        self.overlap = 0
        if wiener:
            self.set_wiener(wiener)
        if overlap:
            self.set_overlap(overlap)
        self.mask_extension = MASK_EXT_CONSTANT
        if mask_extension not in ("constant", MASK_EXT_CONSTANT):
            self.set_mask_extension(mask_extension)

    def _chk(self, rc):
        if rc < 0:
            raise EngineError("libspleeterrt_amd: %s (rc=%d)" % (self.L.srtLastError().decode(), rc))
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.srtDestroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights
    def set_coeff(self, stem, coeff):
        """coeff: numpy float32[9822725] (host) or a CUDA float32 tensor (device), spleeterCoeff layout."""
        import numpy as np
        if isinstance(coeff, np.ndarray):
            a = np.ascontiguousarray(coeff, np.float32)
            assert a.size == COEFF_FLOATS
            self._chk(self.L.srtSetCoeffHost(self.h, stem, C.c_void_p(a.ctypes.data)))
        else:
            assert coeff.is_cuda and coeff.numel() == COEFF_FLOATS and coeff.dtype == self.torch.float32
            self._chk(self.L.srtSetCoeffDevice(self.h, stem, _ptr(coeff.contiguous())))

    def set_coeff_fp16(self, stem, halfs):
        import numpy as np
        a = np.ascontiguousarray(halfs, np.uint16)
        assert a.size == COEFF_FLOATS
        self._chk(self.L.srtSetCoeffFp16Host(self.h, stem, C.c_void_p(a.ctypes.data)))

    def get_coeff(self, stem):
        """the fp32 blob the engine holds for a sub-network (after set_coeff_fp16: the expanded container)"""
        import numpy as np
        a = np.empty(COEFF_FLOATS, np.float32)
        self._chk(self.L.srtGetCoeffHost(self.h, stem, C.c_void_p(a.ctypes.data)))
        return a

    # ---- stages (all tensors live on self.device)
    def forward(self, mag, masks=None):
        """mag [ntiles,2,T,F] -> masks [S,ntiles,2,T,F]"""
        t = self.torch
        nt = mag.shape[0]
        assert mag.is_cuda and mag.dtype == t.float32 and tuple(mag.shape[1:]) == (2, self.T, self.F)
        mag = mag.contiguous()
        if masks is None:
            masks = t.empty((self.S, nt, 2, self.T, self.F), device=self.device, dtype=t.float32)
        self._chk(self.L.srtForward(self.h, _ptr(mag), nt, _ptr(masks)))
        return masks

    def forward_stems(self, mag, masks, stem0, nstems):
        """sub-networks [stem0, stem0+nstems) only; masks keeps the all-stem shape [S,ntiles,2,T,F]"""
        self._chk(self.L.srtForwardStems(self.h, _ptr(mag.contiguous()), mag.shape[0], _ptr(masks), stem0, nstems))
        return masks

    def ratio_mask(self, masks):
        """in place: m_s <- (m_s^2 + eps/S) / (sum_j m_j^2 + eps) across the stem axis"""
        assert masks.is_contiguous() and masks.shape[0] == self.S
        self._chk(self.L.srtRatioMask(self.h, _ptr(masks), masks.shape[1]))
        return masks

    def set_dither_seed(self, seed):
        """the seed of the dithered 16-bit output of the host paths (dither=True; srtSetDitherSeed): any 64-bit value, default 0"""
        self._chk(self.L.srtSetDitherSeed(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_wiener(self, iterations):
        """multichannel Wiener filter (Spleeter's --mwf) inside separate / separate_ex: 0 = off, 1..3 EM iterations (srtSetWiener)"""
        self._chk(self.L.srtSetWiener(self.h, int(iterations)))
        self.wiener = int(iterations)

    def set_overlap(self, rows):
        """overlapped network tiles with cross-faded masks (srtSetOverlap): consecutive tiles of a signal share `rows` rows, 0 <= rows <= T/2
        (0 = off, back-to-back tiles).  stft() then returns mag in the overlapped layout [tiles(rows), 2, T, F] and istft() expects masks in it."""
        self._chk(self.L.srtSetOverlap(self.h, int(rows)))
        self.overlap = int(rows)

    def set_mask_extension(self, mode):
        """the gain of bins >= F (srtSetMaskExtension): "constant" (oob_weights, the default) or "average" (each row's upper bins get the mean of
        that row's in-band gain, per stem and channel: official Spleeter's mask_extension = "average"; oob_weights are ignored).  Also takes MASK_EXT_*."""
        m = {"constant": MASK_EXT_CONSTANT, "average": MASK_EXT_AVERAGE}.get(mode, mode)
        if isinstance(m, str):
            raise EngineError("mask_extension must be \"constant\" or \"average\", not %r" % (mode,))
        self._chk(self.L.srtSetMaskExtension(self.h, int(m)))
        self.mask_extension = int(m)

    def set_mix(self, matrix):
        """stem remix inside the inverse transform (srtSetMix): matrix [n_out, S + 1] - G[m][s] the gain of stem s in output m, G[m][S] the gain of
        the unmasked input - or None / an empty matrix for off.  While it is on istft, separate, separate_ex and separate_host_stream[_io] return n_out pairs
        instead of S."""
        import numpy as np
        if matrix is None or np.size(matrix) == 0:
            self._chk(self.L.srtSetMix(self.h, 0, None))
            return
        g = np.ascontiguousarray(matrix, np.float32)
        if g.ndim != 2 or g.shape[1] != self.S + 1:
            raise EngineError("set_mix: the matrix must be [n_out, n_stems + 1] = [*, %d], not %r" % (self.S + 1, tuple(g.shape)))
        self._chk(self.L.srtSetMix(self.h, int(g.shape[0]), C.c_void_p(g.ctypes.data)))

    @property
    def mix_outputs(self):
        """outputs of the stem remix (srtMixOutputs): n_out while set_mix is on, 0 while it is off"""
        return int(self.L.srtMixOutputs(self.h)) if getattr(self, "h", None) else 0

    @property
    def outputs(self):
        """stereo pairs istft / separate / separate_ex / separate_host_stream[_io] write: mix_outputs while the remix is on, else the stems"""
        return self.mix_outputs or self.S

    def mask_ext(self, stem, rows):
        """the gains of bins >= F the last inverse transform with mask_extension = "average" applied to one stem: numpy [rows, 2] (L, R)"""
        import numpy as np
        a = np.empty((int(rows), 2), np.float32)
        self._chk(self.L.srtCopyTensor(self.h, b"mask_ext", stem, 0, C.c_void_p(a.ctypes.data), a.size))
        return a

    def tiles(self, rows):
        """network tiles of a signal of `rows` spectrum rows at the engine's overlap (stream.overlap_tiles)"""
        from . import stream
        return stream.overlap_tiles(rows, self.T, self.overlap)

    def _wiener_opts(self, who, iterations, overlap, mask_extension, mix):
        """the per-call options of istft_wiener / separate_wiener as (srt_wiener_opts, the matrix it points into, outputs); shape and type errors raise here,
        before any library call.  None: every option is off (the caller takes the entry point without options)."""
        import numpy as np
        m = {"constant": MASK_EXT_CONSTANT, "average": MASK_EXT_AVERAGE}.get(mask_extension, mask_extension) if isinstance(mask_extension, (str, int)) else None
        if isinstance(m, bool) or m not in (MASK_EXT_CONSTANT, MASK_EXT_AVERAGE):
            raise EngineError("%s: mask_extension must be \"constant\" or \"average\", not %r" % (who, mask_extension))
        try:
            it, ov = int(iterations), int(overlap)
        except (TypeError, ValueError):
            raise EngineError("%s: iterations and overlap must be integers, not %r and %r" % (who, iterations, overlap))
        if not 1 <= it <= 3:
            raise EngineError("%s: iterations must be 1..3, not %d" % (who, it))
        if not 0 <= ov <= self.T // 2:
            raise EngineError("%s: overlap must be 0 .. T / 2 = %d rows, not %d" % (who, self.T // 2, ov))
        g = None
        if mix is not None:
            try:
                g = np.ascontiguousarray(mix, np.float32)
            except (TypeError, ValueError):
                raise EngineError("%s: mix must be a real matrix [n_out, n_stems + 1]" % who)
            if g.ndim != 2 or g.shape[1] != self.S + 1 or not 1 <= g.shape[0] <= self.S:
                raise EngineError("%s: mix must be [n_out, n_stems + 1] = [1..%d, %d], not %r" % (who, self.S, self.S + 1, tuple(g.shape)))
            if not np.isfinite(g).all():
                raise EngineError("%s: every gain of mix must be finite" % who)
        if ov == 0 and m == MASK_EXT_CONSTANT and g is None:
            return None
        o = _WienerOpts(it, ov, m, 0 if g is None else g.shape[0], None if g is None else g.ctypes.data_as(C.POINTER(C.c_float)))
        return o, g, (self.S if g is None else g.shape[0])

    def istft_wiener(self, spec, masks, iterations=1, overlap=0, mask_extension="constant", mix=None):
        """spec [2,rows,2052,2], fp32 masks [S,ntiles,2,T,F] -> Wiener-filtered stems [S,2,rows*1024+3072] (srtIstftWiener).
        overlap / mask_extension / mix: options of this call alone, whatever set_overlap / set_mask_extension / set_mix say (srtIstftWienerEx):
        masks in the overlapped layout [S, tiles(rows, overlap), 2, T, F]; "average": bins >= F follow the (blended) masks' row means; mix [n_out, S + 1]
        (set_mix's layout, n_out <= S): the result is [n_out, 2, ..], only those spectra are filtered out and inverted."""
        opts = Engine._wiener_opts(self, "istft_wiener", iterations, overlap, mask_extension, mix)
        t = self.torch
        rows = spec.shape[1]
        assert masks.is_cuda and masks.dtype == t.float32 and masks.is_contiguous() and masks.shape[0] == self.S
        if opts is None:
            out = t.empty((self.S, 2, self.L.srtIstftLength(rows)), device=self.device, dtype=t.float32)
            self._chk(self.L.srtIstftWiener(self.h, _ptr(spec.contiguous()), rows, _ptr(masks), int(iterations), _ptr(out)))
            return out
        o, _keep, planes = opts
        out = t.empty((planes, 2, self.L.srtIstftLength(rows)), device=self.device, dtype=t.float32)
        self._chk(self.L.srtIstftWienerEx(self.h, _ptr(spec.contiguous()), rows, _ptr(masks), C.byref(o), _ptr(out)))
        return out

    def separate_wiener(self, L, R, iterations=1, overlap=0, mask_extension="constant", mix=None, out=None):
        """whole path with the Wiener filter and this call's own options (srtSeparateWiener; the options as istft_wiener's): planar PCM [n] x2 ->
        [S, 2, rows*1024+3072], or [n_out, 2, ..] with a mix.  The engine's set_wiener / set_overlap / set_mask_extension / set_mix are neither read nor changed."""
        opts = Engine._wiener_opts(self, "separate_wiener", iterations, overlap, mask_extension, mix)
        t = self.torch
        if opts is None:
            opts = (_WienerOpts(int(iterations), 0, MASK_EXT_CONSTANT, 0, None), None, self.S)
        o, _keep, planes = opts
        n = L.numel()
        if out is None:
            out = t.empty((planes, 2, self.L.srtIstftLength(self.L.srtStftRows(n))), device=self.device, dtype=t.float32)
        self._chk(self.L.srtSeparateWiener(self.h, _ptr(L), _ptr(R), n, C.byref(o), _ptr(out)))
        return out

    def wiener_cov(self, stem, iteration, track=0):
        """(R [F,4] = R00, R11, Re R01, Im R01; weight sums [F]; a) of one stem and iteration of the last filtered call; after a filtered batch call
        (separate_batch with wiener), of track `track` of that call"""
        import numpy as np
        if not 1 <= int(iteration) <= 3 or int(track) < 0:
            raise EngineError("wiener_cov: iteration must be 1..3 and track >= 0")
        a = np.empty(5 * self.F + 1, np.float32)
        self._chk(self.L.srtCopyTensor(self.h, b"wiener_cov", stem, 4 * int(track) + int(iteration), C.c_void_p(a.ctypes.data), a.size))
        return a[:4 * self.F].reshape(self.F, 4), a[4 * self.F:5 * self.F], float(a[5 * self.F])

    def stft(self, L, R, want_mag=True):
        """planar PCM -> (spec [2,rows,2052,2], mag [ntiles,2,T,F] or None)"""
        t = self.torch
        n = L.numel()
        rows = self.L.srtStftRows(n)
        nt = self.tiles(rows)
        spec = t.empty((2, rows, SPEC_LD, 2), device=self.device, dtype=t.float32)
        mag = t.empty((nt, 2, self.T, self.F), device=self.device, dtype=t.float32) if want_mag else None
        self._chk(self.L.srtStft(self.h, _ptr(L.contiguous()), _ptr(R.contiguous()), n, _ptr(spec), _ptr(mag)))
        return spec, mag

    def istft(self, spec, masks=None):
        """spec [2,rows,2052,2], masks [S,ntiles,2,T,F] or None -> out [S,2,rows*1024+3072] (set_mix on: [n_out,2,..])"""
        t = self.torch
        rows = spec.shape[1]
        out = t.empty((self.outputs, 2, self.L.srtIstftLength(rows)), device=self.device, dtype=t.float32)
        self._chk(self.L.srtIstft(self.h, _ptr(spec), rows, _ptr(masks), _ptr(out)))
        return out

    def separate(self, L, R, out=None):
        """whole path: planar PCM [n] x2 -> stems [S,2,rows*1024+3072] (set_mix on: the mixes [n_out,2,..])"""
        t = self.torch
        n = L.numel()
        rows = self.L.srtStftRows(n)
        if out is None:
            out = t.empty((self.outputs, 2, self.L.srtIstftLength(rows)), device=self.device, dtype=t.float32)
        self._chk(self.L.srtSeparate(self.h, _ptr(L), _ptr(R), n, _ptr(out)))
        return out

    def separate_batch(self, tracks, outs=None, wiener=None, overlap=None, mix=None):
        """many independent tracks: [(L, R)] CUDA float32 tensors -> [stems [S,2,rows_k*1024+3072]], each equal to separate(L, R) of that track.
        The list is cut in order into calls of at most max_tiles packed tiles (stream.pack_tracks); one srtSeparateBatch per call.
        wiener: None = the engine's own setting (set_wiener), 0 = no filter, 1..3 = the multichannel Wiener filter per track with that many iterations
        (one srtSeparateBatchWiener per call): each track as separate(L, R) on an engine with set_wiener(wiener).
        overlap: None = the engine's own setting (set_overlap), 0 = back-to-back tiles, 1..T/2 = overlapped tiles with cross-faded masks inside every track
        (one srtSeparateBatchOverlap per call, the list cut by overlapped tiles): each track as separate(L, R) on an engine with set_overlap(overlap).  The
        filter and an overlap exclude each other.
        mix: None = the stems (the engine's set_mix is not read: the batch calls refuse while it is on); one [n_out, S + 1] matrix for all tracks, or a list of
        one such matrix per track, all with the same n_out (set_mix's layout: the last column is the unmasked input) -> [mixes [n_out,2,rows_k*1024+3072]],
        each equal to separate(L, R) of that track after set_mix(its matrix) and set_overlap(overlap) (one srtSeparateBatchMix per call, each with its own
        tracks' matrices).  Not with the filter."""
        from . import stream
        import numpy as np
        t = self.torch
        ns = [L.numel() for L, _ in tracks]
        G, n_planes = None, self.S
        if mix is not None:
            try:
                G = np.ascontiguousarray(mix, dtype=np.float32)
            except ValueError:                                           # matrices of different shapes
                G = np.zeros(0, np.float32)
            if G.ndim == 2:
                G = np.ascontiguousarray(np.broadcast_to(G, (len(tracks),) + G.shape))
            if G.ndim != 3 or G.shape[0] != len(tracks) or G.shape[2] != self.S + 1 or not 1 <= G.shape[1] <= MAX_STEMS:
                raise EngineError("separate_batch: mix must be [n_out, S + 1] or one such matrix per track with the same n_out (1 <= n_out <= %d)" % MAX_STEMS)
            n_planes = G.shape[1]
        for L, R in tracks:
            assert L.is_cuda and R.is_cuda and L.dtype == t.float32 and R.dtype == t.float32 and R.numel() == L.numel()
        wiener = self.wiener if wiener is None else int(wiener)
        overlap = self.overlap if overlap is None else int(overlap)
        if overlap > 0 and wiener:
            raise EngineError("separate_batch: the Wiener filter is not available with overlapped tiles (overlap = %d, wiener = %d): pass overlap=0 or wiener=0" % (overlap, wiener))
        if G is not None and wiener:
            raise EngineError("separate_batch: the stem mix is not available with the Wiener filter (wiener = %d): pass wiener=0 or mix=None" % wiener)
        if outs is None:
            outs = [t.empty((n_planes, 2, self.L.srtIstftLength(self.L.srtStftRows(n))), device=self.device, dtype=t.float32) for n in ns]
        assert len(outs) == len(tracks)
        for o, n in zip(outs, ns):
            assert o.is_cuda and o.is_contiguous() and o.numel() >= n_planes * 2 * self.L.srtIstftLength(self.L.srtStftRows(n))
        src = [(L.contiguous(), R.contiguous()) for L, R in tracks]      # (kept alive until the calls are issued; the stream orders any reuse)
        own, own_ov = self.wiener, self.overlap
        if own and not wiener:                                           # srtSeparateBatch refuses while the engine's filter is on: off for these calls
            self.set_wiener(0)
        if own_ov and not overlap:                                       # ... and while its overlap is on (srtSeparateBatchOverlap never reads the setting)
            self.set_overlap(0)
        try:
            for g in stream.pack_tracks(ns, self.T, self.max_tiles, overlap):
                k = len(g.tracks)
                P = C.c_void_p * k
                args = (self.h, k, P(*[src[i][0].data_ptr() for i in g.tracks]), P(*[src[i][1].data_ptr() for i in g.tracks]),
                        (C.c_size_t * k)(*[ns[i] for i in g.tracks]), P(*[outs[i].data_ptr() for i in g.tracks]))
                if G is not None:
                    Gk = np.ascontiguousarray(G[list(g.tracks)])
                    self._chk(self.L.srtSeparateBatchMix(*args, overlap, n_planes, Gk.ctypes.data_as(C.POINTER(C.c_float)), n_planes * (self.S + 1)))
                elif overlap > 0:
                    self._chk(self.L.srtSeparateBatchOverlap(*args, overlap))
                else:
                    self._chk(self.L.srtSeparateBatchWiener(*args, wiener) if wiener else self.L.srtSeparateBatch(*args))
        finally:
            if own and not wiener:
                self.set_wiener(own)
            if own_ov and not overlap:
                self.set_overlap(own_ov)
        return outs

    def separate_batch_wiener(self, tracks, outs=None, iterations=1, overlap=0, mask_extension="constant", mix=None):
        """many independent tracks through the Wiener filter with this call's own options (one srtSeparateBatchWienerEx per call):
        [(L, R)] CUDA float32 tensors -> [stems [S,2,rows_k*1024+3072]] (with a mix: [n_out,2,..]), each equal to separate_wiener(L, R, iterations, overlap,
        mask_extension, its matrix) of that track.  The list is cut in order by stream.pack_tracks(ns, T, max_tiles, overlap).  mix: one [n_out, S + 1]
        matrix for all tracks, or one such matrix per track with the same n_out <= S; each call gets its own tracks' matrices.  The engine's set_wiener /
        set_overlap / set_mask_extension / set_mix are neither read nor changed.  Argument errors raise EngineError before any library call."""
        from . import stream
        import numpy as np
        who = "separate_batch_wiener"
        m = {"constant": MASK_EXT_CONSTANT, "average": MASK_EXT_AVERAGE}.get(mask_extension, mask_extension) if isinstance(mask_extension, (str, int)) else None
        if isinstance(m, bool) or m not in (MASK_EXT_CONSTANT, MASK_EXT_AVERAGE):
            raise EngineError("%s: mask_extension must be \"constant\" or \"average\", not %r" % (who, mask_extension))
        try:
            it, ov = int(iterations), int(overlap)
        except (TypeError, ValueError):
            raise EngineError("%s: iterations and overlap must be integers, not %r and %r" % (who, iterations, overlap))
        if not 1 <= it <= 3:
            raise EngineError("%s: iterations must be 1..3, not %d" % (who, it))
        if not 0 <= ov <= self.T // 2:
            raise EngineError("%s: overlap must be 0 .. T / 2 = %d rows, not %d" % (who, self.T // 2, ov))
        G, n_out = None, 0
        if mix is not None:
            shape = "%s: mix must be [n_out, n_stems + 1] or one such matrix per track with the same n_out (1 <= n_out <= %d)" % (who, self.S)
            try:
                G = np.ascontiguousarray(mix, dtype=np.float32)
            except (TypeError, ValueError):                              # matrices of different shapes (two n_out), or no numbers at all
                raise EngineError(shape)
            if G.ndim == 2:
                G = np.ascontiguousarray(np.broadcast_to(G, (len(tracks),) + G.shape))
            if G.ndim != 3 or G.shape[0] != len(tracks) or G.shape[2] != self.S + 1 or not 1 <= G.shape[1] <= self.S:
                raise EngineError(shape)
            if not np.isfinite(G).all():
                raise EngineError("%s: every gain of mix must be finite" % who)
            n_out = G.shape[1]
        t = self.torch
        n_planes = n_out if n_out else self.S
        ns = [L.numel() for L, _ in tracks]
        for L, R in tracks:
            assert L.is_cuda and R.is_cuda and L.dtype == t.float32 and R.dtype == t.float32 and R.numel() == L.numel()
        if outs is None:
            outs = [t.empty((n_planes, 2, self.L.srtIstftLength(self.L.srtStftRows(n))), device=self.device, dtype=t.float32) for n in ns]
        assert len(outs) == len(tracks)
        for o, n in zip(outs, ns):
            assert o.is_cuda and o.is_contiguous() and o.numel() >= n_planes * 2 * self.L.srtIstftLength(self.L.srtStftRows(n))
        src = [(L.contiguous(), R.contiguous()) for L, R in tracks]      # (kept alive until the calls are issued; the stream orders any reuse)
        for g in stream.pack_tracks(ns, self.T, self.max_tiles, ov):
            k = len(g.tracks)
            P = C.c_void_p * k
            Gk = None if G is None else np.ascontiguousarray(G[list(g.tracks)])
            opts = _BatchWienerOpts(it, ov, m, n_out, None if Gk is None else Gk.ctypes.data_as(C.POINTER(C.c_float)), n_out * (self.S + 1))
            self._chk(self.L.srtSeparateBatchWienerEx(self.h, k, P(*[src[i][0].data_ptr() for i in g.tracks]), P(*[src[i][1].data_ptr() for i in g.tracks]),
                                                      (C.c_size_t * k)(*[ns[i] for i in g.tracks]), P(*[outs[i].data_ptr() for i in g.tracks]), C.byref(opts)))
        return outs

    def separate_cli(self, L, R, stems):
        """the offline CLI's flow (main.c:776-798 / 845-928): -> [stems,2,len] = (Vocal, Accompaniment) or (Drum, Vocal, Accompaniment)"""
        t = self.torch
        n = L.numel()
        out = t.empty((stems, 2, self.L.srtIstftLength(self.L.srtStftRows(n))), device=self.device, dtype=t.float32)
        self._chk(self.L.srtSeparateCli(self.h, _ptr(L.contiguous()), _ptr(R.contiguous()), n, stems, _ptr(out)))
        return out

    def separate_cli_host(self, L, R, stems, keep_staging=False):
        """the CLI flow from host buffers (numpy float32), any length: one resident batch when the file fits max_tiles tiles, otherwise
        chunk by chunk (srtSeparateCliHost) -> numpy [stems,2,len].  The call's device staging (whole-file PCM + outputs for a file that fits, O(file)
        bytes of HBM) is released afterwards unless keep_staging=True (a caller that separates file after file keeps it to avoid re-allocating)."""
        import numpy as np
        L = np.ascontiguousarray(L, np.float32)
        R = np.ascontiguousarray(R, np.float32)
        assert L.size == R.size
        out = np.empty((stems, 2, self.L.srtIstftLength(self.L.srtStftRows(L.size))), np.float32)
        try:
            self._chk(self.L.srtSeparateCliHost(self.h, C.c_void_p(L.ctypes.data), C.c_void_p(R.ctypes.data), L.size, stems, C.c_void_p(out.ctypes.data)))
        except EngineError:
            if not keep_staging:
                self.L.srtReleaseStaging(self.h)              # best effort: the separation's own error is the one to report
            raise
        if not keep_staging:
            self._chk(self.L.srtReleaseStaging(self.h))
        return out

    def separate_host_stream(self, L, R, frames=None, rows=None, out=None, pinned=False):
        """host PCM of any length -> host stems [S,2,rows*1024+3072]; chunks of max_tiles tiles with the PCIe copies
        overlapped with compute (srtSeparateHostStreamEx).  L, R, out: contiguous float32 numpy arrays or CPU torch
        tensors; pinned=True promises they are page-locked already (torch pin_memory), so nothing is registered per call."""
        import numpy as np

        def host(a):
            if hasattr(a, "data_ptr"):                           # CPU torch tensor (e.g. pin_memory=True)
                assert not a.is_cuda and a.dtype == self.torch.float32 and a.is_contiguous()
                return a, a.data_ptr(), a.numel()
            a = np.ascontiguousarray(a, np.float32)
            return a, a.ctypes.data, a.size
        L, pL, n = host(L)
        R, pR, nR = host(R)
        assert n == nR
        rows = self.L.srtStftRows(n) if rows is None else rows
        frames = self.L.srtStftFrames(n) if frames is None else frames
        shape = (self.outputs, 2, self.L.srtIstftLength(rows))
        ret = None
        if out is None:
            if pinned:                                           # keep the promise for the output too
                out = self.torch.empty(shape, dtype=self.torch.float32, pin_memory=True)
                ret = out.numpy()
            else:
                out = np.empty(shape, np.float32)
        out, pO, no = host(out)
        assert no == shape[0] * shape[1] * shape[2]
        self._chk(self.L.srtSeparateHostStreamEx(self.h, C.c_void_p(pL), C.c_void_p(pR), n, frames, rows, C.c_void_p(pO),
                                                 1 if pinned else 0))
        return out if ret is None else ret

    def _host_io(self, pcm_or_LR, out_pcm16, nstems, rows, out, pinned, length=None, out_bits=None, dither=False):
        """host buffers of the *_io calls -> (keep-alive list, h_in, h_in2, n, h_out, flags, out object, clipped array).  Input by dtype: an int16 array or CPU
        tensor of shape [n, 2] is interleaved 16-bit PCM, a uint8 one of shape [n, 2, 3] packed 24-bit PCM, anything else a pair (L, R) of float32 buffers.
        out_bits: 32 (float32 [S, 2, len]), 24 (uint8 [S, len, 2, 3]) or 16 (int16 [S, len, 2]); out_pcm16=True means 16; dither: TPDF dither, 16-bit output only."""
        if out_bits is None:
            out_bits = 16 if out_pcm16 else 32
        if out_bits not in (16, 24, 32):
            raise ValueError("out_bits must be 16, 24 or 32, not %r" % (out_bits,))
        if out_pcm16 and out_bits != 16:
            raise ValueError("out_pcm16=True means out_bits=16, not %r" % (out_bits,))
        if dither and out_bits != 16:
            raise ValueError("dither=True applies to 16-bit output only (out_bits=16), not out_bits=%r" % (out_bits,))
        import numpy as np
        t = self.torch

        def host(a, dtype):
            if hasattr(a, "data_ptr"):                           # CPU torch tensor (e.g. pin_memory=True)
                assert not a.is_cuda and a.dtype == getattr(t, np.dtype(dtype).name) and a.is_contiguous()
                return a, a.data_ptr(), a.numel()
            a = np.ascontiguousarray(a, dtype)
            return a, a.ctypes.data, a.size
        flags = HOST_PINNED if pinned else 0
        is16 = not isinstance(pcm_or_LR, (tuple, list)) and str(pcm_or_LR.dtype) in ("int16", "torch.int16")
        is24 = not isinstance(pcm_or_LR, (tuple, list)) and str(pcm_or_LR.dtype) in ("uint8", "torch.uint8")
        if is24:
            assert len(pcm_or_LR.shape) == 3 and tuple(pcm_or_LR.shape[1:]) == (2, 3), "24-bit input is packed interleaved stereo [n, 2, 3]"
            a, p_in, cnt = host(pcm_or_LR, np.uint8)
            keep, p_in2, n = [a], None, cnt // 6
            flags |= HOST_IN_PCM24
        elif is16:
            assert len(pcm_or_LR.shape) == 2 and pcm_or_LR.shape[1] == 2, "16-bit input is interleaved stereo [n, 2]"
            a, p_in, cnt = host(pcm_or_LR, np.int16)
            keep, p_in2, n = [a], None, cnt // 2
            flags |= HOST_IN_PCM16
        else:
            (a, p_in, n), (b, p_in2, nb) = host(pcm_or_LR[0], np.float32), host(pcm_or_LR[1], np.float32)
            assert n == nb
            keep = [a, b]
        rows = self.L.srtStftRows(n) if rows is None else rows
        ln = self.L.srtIstftLength(rows) if length is None else length      # length: frames per output plane where the call's rates decide it (separate_host_rate)
        shape, dtype = {16: ((nstems, ln, 2), np.int16), 24: ((nstems, ln, 2, 3), np.uint8), 32: ((nstems, 2, ln), np.float32)}[out_bits]
        flags |= {16: HOST_OUT_PCM16, 24: HOST_OUT_PCM24, 32: 0}[out_bits] | (HOST_OUT_DITHER if dither else 0)
        ret = None
        if out is None:
            if pinned:                                           # keep the promise for the output too
                out = t.empty(shape, dtype=getattr(t, np.dtype(dtype).name), pin_memory=True)
                ret = out.numpy()
            else:
                out = np.empty(shape, dtype)
        o, p_out, no = host(out, dtype)
        assert no == int(np.prod(shape))
        clipped = np.zeros(nstems, np.uint64)
        return keep + [o], p_in, p_in2, n, rows, p_out, flags, (o if ret is None else ret), clipped

    def separate_host_stream_io(self, pcm_or_LR, out_pcm16=False, frames=None, rows=None, out=None, pinned=False, out_bits=None, dither=False):
        """separate_host_stream with 16-bit PCM on either side (srtSeparateHostStreamIo; the conversion runs on the GPU, half the bytes cross the bus).
        pcm_or_LR: int16 [n, 2] interleaved stereo, or (L, R) float32; out_pcm16: stems as int16 [S, len, 2] (a WAV data chunk per stem) instead of float32
        [S, 2, len].  -> (out, clipped): clipped uint64 [S], the samples per stem whose value before clamping lay outside [-32768, 32767] (zeros for float output).
        24 bits: a uint8 [n, 2, 3] input is packed 24-bit PCM; out_bits=24 gives uint8 [S, len, 2, 3]; out_bits=16 is out_pcm16=True, and dither=True
        adds the TPDF dither of set_dither_seed to it (the noise does not depend on max_tiles)."""
        keep, p_in, p_in2, n, rows, p_out, flags, out, clipped = self._host_io(pcm_or_LR, out_pcm16, self.outputs, rows, out, pinned, out_bits=out_bits, dither=dither)
        frames = self.L.srtStftFrames(n) if frames is None else frames
        self._chk(self.L.srtSeparateHostStreamIo(self.h, C.c_void_p(p_in), C.c_void_p(p_in2), n, frames, rows, C.c_void_p(p_out), flags, C.c_void_p(clipped.ctypes.data)))
        return out, clipped

    def separate_host_overlap(self, pcm_or_LR, overlap, out_pcm16=False, out=None, pinned=False, out_bits=None, dither=False):
        """separate() under set_overlap(overlap) for host PCM of any length (srtSeparateHostStreamOverlap): the stream is walked in pieces of
        max_tiles overlapped tiles (stream.host_overlap_pieces) and the mask blend crosses the piece seams through a small device carry.  overlap (0 .. T/2 rows)
        holds for this call only - the engine's set_overlap is neither read nor changed; ratio_mask, the mask extension and the mix come from the engine.  Buffers as
        separate_host_stream_io: pcm_or_LR int16 [n, 2] or (L, R) float32; out_pcm16: int16 [outputs, len, 2] instead of float32 [outputs, 2, len]; pinned=True
        promises page-locked buffers; out_bits / dither and a uint8 [n, 2, 3] input as there.  overlap = 0 is separate_host_stream_io.  -> (out, clipped)."""
        try:
            ov = int(overlap)
        except (TypeError, ValueError):
            raise EngineError("separate_host_overlap: overlap must be an integer 0 .. T / 2, not %r" % (overlap,))
        if ov != overlap or ov < 0 or ov > self.T // 2:
            raise EngineError("separate_host_overlap: overlap must be an integer 0 .. T / 2 = %d, not %r" % (self.T // 2, overlap))
        keep, p_in, p_in2, n, rows, p_out, flags, out, clipped = self._host_io(pcm_or_LR, out_pcm16, self.outputs, None, out, pinned, out_bits=out_bits, dither=dither)
        if n < 4096:
            raise EngineError("separate_host_overlap: need at least 4096 samples, not %d" % n)
        self._chk(self.L.srtSeparateHostStreamOverlap(self.h, C.c_void_p(p_in), C.c_void_p(p_in2), n, ov, C.c_void_p(p_out), flags, C.c_void_p(clipped.ctypes.data)))
        return out, clipped

    def host_rate_length(self, n, sample_rate, out_rate=None):
        """srtHostRateLength: frames per output plane of separate_host_rate for n input frames at sample_rate (pure arithmetic).  Raises for bad arguments."""
        ln = self.L.srtHostRateLength(int(n), int(sample_rate), int(sample_rate if out_rate is None else out_rate))
        if not ln:
            raise EngineError("libspleeterrt_amd: %s" % self.L.srtLastError().decode())
        return ln

    def separate_host_rate(self, pcm_or_LR, sample_rate, out_rate=None, overlap=0, out_pcm16=False, out=None, pinned=False, out_bits=None, dither=False):
        """separate_host_stream_io / separate_host_overlap for host PCM at sample_rate with the outputs at out_rate (None: sample_rate; either may be 44100)
        (srtSeparateHostStreamRate): both conversions run on the device inside the chunk pipeline, so every sample crosses the bus once at its own
        rate.  Equals Resampler.resample_host to 44.1 kHz, separate_host_overlap, resample_host per output pair, bit for bit.  overlap (0 .. T/2 rows) holds for the
        call only; ratio_mask, the mask extension and the mix come from the engine.  Buffers as separate_host_stream_io: pcm_or_LR int16 [n, 2] or (L, R) float32;
        out float32 [outputs, 2, host_rate_length(n, ..)] or, with out_pcm16, int16 [outputs, length, 2]; out_bits / dither and a uint8 [n, 2, 3] input as there (the
        dither's sample index runs over the converted output).  -> (out, clipped)."""
        try:
            fs_in, fs_out, ov = int(sample_rate), int(sample_rate if out_rate is None else out_rate), int(overlap)
        except (TypeError, ValueError):
            raise EngineError("separate_host_rate: sample_rate, out_rate and overlap must be integers, not %r, %r, %r" % (sample_rate, out_rate, overlap))
        if ov != overlap or ov < 0 or ov > self.T // 2:
            raise EngineError("separate_host_rate: overlap must be an integer 0 .. T / 2 = %d, not %r" % (self.T // 2, overlap))
        first = pcm_or_LR[0] if isinstance(pcm_or_LR, (tuple, list)) else pcm_or_LR        # (L, R) or int16 [n, 2]: n is the first axis either way
        ln = self.host_rate_length(first.shape[0] if hasattr(first, "shape") else len(first), fs_in, fs_out)
        keep, p_in, p_in2, n, rows, p_out, flags, out, clipped = self._host_io(pcm_or_LR, out_pcm16, self.outputs, 0, out, pinned, length=ln, out_bits=out_bits, dither=dither)
        self._chk(self.L.srtSeparateHostStreamRate(self.h, C.c_void_p(p_in), C.c_void_p(p_in2), n, fs_in, fs_out, ov, C.c_void_p(p_out), flags, C.c_void_p(clipped.ctypes.data)))
        return out, clipped

    def separate_host_wiener(self, pcm_or_LR, iterations=1, mask_extension="constant", mix=None, out_pcm16=False, out=None, pinned=False, overlap=0, out_bits=None, dither=False):
        """separate_wiener for host PCM of any length (srtSeparateHostWiener): the stream is walked in pieces of max_tiles tiles, its spectrum and
        masks are kept in a device store of host_wiener_bytes(n) bytes, and the R tables are those of one separate_wiener call over the whole signal, bit for bit.
        Buffers as separate_host_stream_io: pcm_or_LR int16 [n, 2] or (L, R) float32; out_pcm16: int16 [outputs, len, 2] instead of float32 [outputs, 2, len];
        pinned=True promises page-locked buffers; out_bits / dither and a uint8 [n, 2, 3] input as there.  iterations / mask_extension / mix: options of this call alone, as separate_wiener's; overlap must be 0
        (separate_host_wiener_overlap takes one).  -> (out, clipped).  wiener_cov works afterwards; release_staging frees the store."""
        try:
            ov = int(overlap)
        except (TypeError, ValueError):
            raise EngineError("separate_host_wiener: overlap must be 0, not %r" % (overlap,))
        if ov != 0:
            raise EngineError("separate_host_wiener: overlap must be 0, not %d (separate_host_wiener_overlap takes overlapped tiles)" % ov)
        opts = Engine._wiener_opts(self, "separate_host_wiener", iterations, 0, mask_extension, mix)
        if opts is None:
            opts = (_WienerOpts(int(iterations), 0, MASK_EXT_CONSTANT, 0, None), None, self.S)
        o, _keep_g, planes = opts
        keep, p_in, p_in2, n, rows, p_out, flags, out, clipped = self._host_io(pcm_or_LR, out_pcm16, planes, None, out, pinned, out_bits=out_bits, dither=dither)
        self._chk(self.L.srtSeparateHostWiener(self.h, C.c_void_p(p_in), C.c_void_p(p_in2), n, C.byref(o), C.c_void_p(p_out), flags, C.c_void_p(clipped.ctypes.data)))
        return out, clipped

    def host_wiener_bytes(self, n):
        """bytes of the device store separate_host_wiener keeps for a stream of n samples on this engine (srtHostWienerBytes)"""
        return host_wiener_bytes(n, self.F, self.T, self.S, self.max_tiles)

    def separate_host_wiener_overlap(self, pcm_or_LR, overlap, iterations=1, mask_extension="constant", mix=None, out_pcm16=False, out=None, pinned=False, out_bits=None, dither=False):
        """separate_wiener(..., overlap=overlap) for host PCM of any length (srtSeparateHostWienerOverlap): the stream is walked in pieces of
        max_tiles overlapped tiles (stream.host_overlap_pieces), spectrum, masks and one mask carry per piece boundary are kept in a device store of
        host_wiener_overlap_bytes(n, overlap) bytes, and the R tables are those of one separate_wiener call over the whole signal, bit for bit.  overlap
        (0 .. T/2 rows), iterations, mask_extension and mix are options of this call alone; buffers as separate_host_wiener.  overlap = 0 is
        separate_host_wiener.  -> (out, clipped).  wiener_cov works afterwards; release_staging frees the store."""
        try:
            ov = int(overlap)
        except (TypeError, ValueError):
            raise EngineError("separate_host_wiener_overlap: overlap must be an integer 0 .. T / 2, not %r" % (overlap,))
        if ov != overlap or ov < 0 or ov > self.T // 2:
            raise EngineError("separate_host_wiener_overlap: overlap must be an integer 0 .. T / 2 = %d, not %r" % (self.T // 2, overlap))
        opts = Engine._wiener_opts(self, "separate_host_wiener_overlap", iterations, ov, mask_extension, mix)
        if opts is None:
            opts = (_WienerOpts(int(iterations), 0, MASK_EXT_CONSTANT, 0, None), None, self.S)
        o, _keep_g, planes = opts
        keep, p_in, p_in2, n, rows, p_out, flags, out, clipped = self._host_io(pcm_or_LR, out_pcm16, planes, None, out, pinned, out_bits=out_bits, dither=dither)
        if n < 4096:
            raise EngineError("separate_host_wiener_overlap: need at least 4096 samples, not %d" % n)
        self._chk(self.L.srtSeparateHostWienerOverlap(self.h, C.c_void_p(p_in), C.c_void_p(p_in2), n, C.byref(o), C.c_void_p(p_out), flags, C.c_void_p(clipped.ctypes.data)))
        return out, clipped

    def host_wiener_overlap_bytes(self, n, overlap):
        """bytes of the device store separate_host_wiener_overlap keeps for a stream of n samples at this overlap on this engine (srtHostWienerOverlapBytes)"""
        return host_wiener_overlap_bytes(n, self.F, self.T, self.S, self.max_tiles, overlap)

    def separate_cli_host_io(self, pcm_or_LR, stems, out_pcm16=False, out=None, pinned=False, keep_staging=False, out_bits=None, dither=False):
        """separate_cli_host with 16- or 24-bit PCM on either side (srtSeparateCliHostIo) -> (out, clipped) as separate_host_stream_io, `stems` outputs."""
        keep, p_in, p_in2, n, rows, p_out, flags, out, clipped = self._host_io(pcm_or_LR, out_pcm16, stems, None, out, pinned, out_bits=out_bits, dither=dither)
        try:
            self._chk(self.L.srtSeparateCliHostIo(self.h, C.c_void_p(p_in), C.c_void_p(p_in2), n, stems, C.c_void_p(p_out), flags, C.c_void_p(clipped.ctypes.data)))
        except EngineError:
            if not keep_staging:
                self.L.srtReleaseStaging(self.h)              # best effort: the separation's own error is the one to report
            raise
        if not keep_staging:
            self._chk(self.L.srtReleaseStaging(self.h))
        return out, clipped

    def separate_ex(self, L, R, frames, rows, out=None):
        """explicit-geometry form used by spleeterrt_amd.stream for tile ranges of a longer stream"""
        t = self.torch
        if out is None:
            out = t.empty((self.outputs, 2, self.L.srtIstftLength(rows)), device=self.device, dtype=t.float32)
        self._chk(self.L.srtSeparateEx(self.h, _ptr(L.contiguous()), _ptr(R.contiguous()), L.numel(), frames, rows, _ptr(out)))
        return out

    # ---- debug / measurement
    def tensor(self, name, stem, tile):
        import numpy as np
        lvl = int(name[-1])
        if name.startswith("up"):
            co = (256, 128, 64, 32, 16, 1)[lvl - 1]
            sh = (co, self.T >> (6 - lvl), self.F >> (6 - lvl))
        else:
            co = (16, 32, 64, 128, 256, 512)[lvl - 1]
            sh = (co, self.T >> lvl, self.F >> lvl)
        a = np.empty(sh, np.float32)
        self._chk(self.L.srtCopyTensor(self.h, name.encode(), stem, tile, C.c_void_p(a.ctypes.data), a.size))
        return a

    def set_graph_mode(self, on=True):
        """replay srtForward / srtSeparate as captured hipGraphs when called again with the same tensors (needs a non-default stream)"""
        self._chk(self.L.srtSetGraphMode(self.h, int(on)))

    def prepare_forward(self, mag, masks):
        """allocate / capture everything forward(mag, masks) would do lazily (runs the networks once into masks)"""
        self._chk(self.L.srtPrepareForward(self.h, _ptr(mag), mag.shape[0], _ptr(masks)))

    def release_staging(self):
        self._chk(self.L.srtReleaseStaging(self.h))

    def set_timing(self, on=True):
        self._chk(self.L.srtSetTiming(self.h, int(on)))

    def get_timing(self, max_entries=65536):
        names = C.create_string_buffer(max_entries * 8)
        ms = (C.c_float * max_entries)()
        n = self._chk(self.L.srtGetTiming(self.h, names, len(names), ms, max_entries))
        nm = names.value.decode().split(",")[:n]
        return list(zip(nm, list(ms[:n])))

    def get_timing_kernels(self, max_entries=65536):
        """[(launch name, kernel symbol that ran it)] for the launches recorded since set_timing(True)"""
        tim = self.get_timing(max_entries)
        buf = C.create_string_buffer(len(tim) * 160 + 16)
        n = self._chk(self.L.srtGetTimingKernels(self.h, buf, len(buf)))
        ks = buf.value.decode().split(";")[:n]
        return [(name, k) for (name, _), k in zip(tim, ks)]


class _HostPiece(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("tile0", "tiles", "row0", "own_rows", "stft_rows")]


def host_overlap_pieces(rows, T, overlap, max_tiles):
    """srtHostOverlapPieces: the piece plan of srtSeparateHostStreamOverlap as a list of dicts (tile0, tiles, row0, own_rows, stft_rows), from the library -
    stream.host_overlap_pieces is the same arithmetic in Python.  Pure host arithmetic: works without a device.  Raises for bad arguments."""
    L = load_library()
    n = L.srtHostOverlapPieces(int(rows), int(T), int(overlap), int(max_tiles), None, 0)
    if not n:
        if int(rows) == 0 and int(T) >= 1 and 0 <= int(overlap) <= int(T) // 2 and int(max_tiles) >= 1:
            return []
        raise EngineError("libspleeterrt_amd: %s" % L.srtLastError().decode())
    buf = (_HostPiece * n)()
    L.srtHostOverlapPieces(int(rows), int(T), int(overlap), int(max_tiles), C.cast(buf, C.c_void_p), n)
    return [dict((k, int(getattr(p, k))) for k, _ in _HostPiece._fields_) for p in buf]


class _HostRatePiece(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("src0", "src_len", "s0", "ns", "fin0", "fin1", "out0", "out1")]


def host_rate_pieces(n, in_rate, out_rate, T, overlap, max_tiles, F=1024):
    """srtHostRatePieces: the piece plan of srtSeparateHostStreamRate for n frames at in_rate as a list of dicts (src0, src_len, s0, ns, fin0, fin1, out0, out1), from
    the library - stream.host_rate_pieces is the same arithmetic in Python.  Pure host arithmetic: works without a device.  Raises for bad arguments."""
    L = load_library()
    cfg = _Config()
    cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles = int(F), int(T), 1, int(max_tiles)
    args = (C.byref(cfg), int(n), int(in_rate), int(out_rate), int(overlap))
    cnt = L.srtHostRatePieces(*args, None, 0)
    if not cnt:
        raise EngineError("libspleeterrt_amd: %s" % L.srtLastError().decode())
    buf = (_HostRatePiece * cnt)()
    L.srtHostRatePieces(*args, C.cast(buf, C.c_void_p), cnt)
    return [dict((k, int(getattr(p, k))) for k, _ in _HostRatePiece._fields_) for p in buf]


def host_rate_length(n, in_rate, out_rate):
    """srtHostRateLength without an engine: frames per output plane; raises for bad arguments"""
    L = load_library()
    ln = L.srtHostRateLength(int(n), int(in_rate), int(out_rate))
    if not ln:
        raise EngineError("libspleeterrt_amd: %s" % L.srtLastError().decode())
    return ln


def host_wiener_bytes(n, F, T, n_stems, max_tiles):
    """srtHostWienerBytes: bytes of the device store srtSeparateHostWiener keeps for a stream of n samples - per spectrum row 2 * 2052 * 8 (the complex spectrum)
    + n_stems * 2 * F * 4 (the fp32 masks, padded to the tile boundary).  Pure host arithmetic: works without a device.  Raises for a bad geometry or n < 4096."""
    L = load_library()
    cfg = _Config()
    cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles = int(F), int(T), int(n_stems), int(max_tiles)
    b = L.srtHostWienerBytes(C.byref(cfg), int(n))
    if not b:
        raise EngineError("libspleeterrt_amd: %s" % L.srtLastError().decode())
    return int(b)


def host_wiener_overlap_bytes(n, F, T, n_stems, max_tiles, overlap):
    """srtHostWienerOverlapBytes: bytes of the device store srtSeparateHostWienerOverlap keeps for a stream of n samples.  With S = T - overlap and P = max_tiles
    every piece but the last takes 2 * ((P - 1) S + T) * 2052 * 8 (its spectrum, the look-ahead rows included) + n_stems * P * 2 * T * F * 4 (its fp32 masks)
    + n_stems * 2 * overlap * F * 4 (the mask carry of its boundary); the last one its own rows and tiles and no carry.  overlap = 0: host_wiener_bytes.  Pure host
    arithmetic: works without a device.  Raises for a bad geometry, n < 4096 or an overlap outside 0 .. T / 2."""
    L = load_library()
    cfg = _Config()
    cfg.F, cfg.T, cfg.n_stems, cfg.max_tiles = int(F), int(T), int(n_stems), int(max_tiles)
    b = L.srtHostWienerOverlapBytes(C.byref(cfg), int(n), int(overlap))
    if not b:
        raise EngineError("libspleeterrt_amd: %s" % L.srtLastError().decode())
    return int(b)


def live_latency(hops_per_run, lookahead):
    """srtLiveLatency's arithmetic: the delay in samples of a live stream fed 1024-sample blocks, (L + 2K) * 1024 + 1024"""
    return (int(lookahead) + 2 * int(hops_per_run)) * 1024 + 1024


def live_rate_latency(sample_rate, hops_per_run, lookahead):
    """srtLiveRateLatency: the constant delay in samples of a rate instance (Live(..., sample_rate=fs)); pure host arithmetic, no device"""
    L = load_library()
    rc = L.srtLiveRateLatency(int(sample_rate), int(hops_per_run), int(lookahead))
    if rc < 0:
        raise EngineError("libspleeterrt_amd: %s (rc=%d)" % (L.srtLastError().decode(), rc))
    return rc


class Live:
    """Live separation with a sliding network window (srtLive*, include/spleeterrt_amd.h) on the current device: the networks
    run every hops_per_run hops on the newest T frames, with `lookahead` frames of future context per frame.  hops_per_run = T, lookahead = 0 with
    the plugin's config (VST, stem modes 1, oob 0.25 / 0 / 0.25 / 0.25) is Spleeter4Stems.  coeffs: one float32 spleeterCoeff blob per stem.
    sample_rate=fs makes a rate instance (srtLiveCreateRate): calls take samples at fs, every call writes as many samples as it got and
    the delay is the constant `latency` whatever the call sizes; max_block is the largest slice a call is processed in.
    mix=G ([n_out][S + 1], srtSetMix's layout: the last column is the unmasked input) makes the calls write n_out stereo pairs, the mix of the stems formed
    inside the hop's inverse transform; set_mix replaces the values later.  mask_extension="average" lets the bins above F follow each
    stem's mean mask instead of oob_weights.  Either one creates through srtLiveCreateEx (create_ex=True does so with no option set).
    wiener=n (1..3) creates through srtLiveCreateWiener: the multichannel Wiener filter over each run's network window, applied inside the hop's inverse
    transform; `wiener` returns the count and tensor() reads the last launched run's tables, window and masks back."""

    def __init__(self, F, T, stem_modes, oob_weights, variant, precision, hops_per_run, lookahead, coeffs, impl=IMPL_MFMA,
                 ratio_mask=False, batch_invariant=False, max_tiles=1, sample_rate=None, max_block=4096, mix=None, mask_extension="constant",
                 create_ex=False, wiener=0):
        import numpy as np
        self.L = load_library()
        self.S, self.F, self.T = len(stem_modes), F, T
        self.hops_per_run, self.lookahead = int(hops_per_run), int(lookahead)
        cfg = _Config()
        cfg.F, cfg.T, cfg.n_stems, cfg.variant, cfg.max_tiles, cfg.impl = F, T, self.S, variant, max_tiles, impl
        cfg.precision, cfg.ratio_mask, cfg.batch_invariant = precision, int(bool(ratio_mask)), int(bool(batch_invariant))
        for i, m in enumerate(stem_modes):
            cfg.stem_mode[i] = int(m)
            cfg.oob_weight[i] = float(oob_weights[i])
        blobs = [None if c is None else np.ascontiguousarray(c, np.float32) for c in coeffs]
        for b in blobs:
            assert b is None or b.size == COEFF_FLOATS
        ptrs = (C.c_void_p * max(len(blobs), 1))(*[None if b is None else b.ctypes.data for b in blobs])
        h = C.c_void_p()
        self.sample_rate = None if sample_rate is None else int(sample_rate)
        ext = {"constant": MASK_EXT_CONSTANT, "average": MASK_EXT_AVERAGE}.get(mask_extension, mask_extension)
        if mix is not None or ext != MASK_EXT_CONSTANT or create_ex or int(wiener) > 0:
            o = _LiveOpts()
            if sample_rate is not None:
                o.sample_rate, o.max_block = self.sample_rate, int(max_block)
            if mix is not None:
                g = self._gain(mix, None)
                o.n_out, o.h_gain = g.shape[0], g.ctypes.data_as(C.POINTER(C.c_float))
            o.mask_extension = int(ext)
            if int(wiener) > 0:
                self._chk(self.L.srtLiveCreateWiener(C.byref(cfg), self.hops_per_run, self.lookahead, C.byref(o), int(wiener), ptrs, C.byref(h)))
            else:
                self._chk(self.L.srtLiveCreateEx(C.byref(cfg), self.hops_per_run, self.lookahead, C.byref(o), ptrs, C.byref(h)))
        elif sample_rate is None:
            self._chk(self.L.srtLiveCreate(C.byref(cfg), self.hops_per_run, self.lookahead, ptrs, C.byref(h)))
        else:
            self._chk(self.L.srtLiveCreateRate(C.byref(cfg), self.hops_per_run, self.lookahead, self.sample_rate, int(max_block), ptrs, C.byref(h)))
        self.h = h

    def _chk(self, rc):
        if rc < 0:
            raise EngineError("libspleeterrt_amd: %s (rc=%d)" % (self.L.srtLastError().decode(), rc))
        return rc

    def _gain(self, G, n_out):
        import numpy as np
        g = np.ascontiguousarray(G, np.float32)
        if g.ndim != 2 or g.shape[1] != self.S + 1 or (n_out is not None and g.shape[0] != n_out):
            raise ValueError("the mix matrix must be [%s][%d] (the last column is the unmasked input)" % ("n_out" if n_out is None else n_out, self.S + 1))
        return g

    @property
    def outputs(self):
        """stereo pairs a call writes (srtLiveOutputs): the mix's n_out, or the stem count while it is off"""
        return self.L.srtLiveOutputs(self.h)

    @property
    def wiener(self):
        """iterations of the Wiener filter in the hop path (srtLiveWiener), 0 while off"""
        return self.L.srtLiveWiener(self.h)

    def tensor(self, name, stem=0, index=0):
        """srtLiveCopyTensor: (array, run_hop) of the run launched last - "wiener_cov" (index = iteration 1..n; 5 F + 1 floats: R [F][4], weight sums [F], a),
        "wiener_spec" (complex64 [2][T][2052]) or "masks" (the stem's [2][T][F]); (None, -1) while no run has been launched.  Waits for the instance's streams."""
        import numpy as np
        count = {"wiener_cov": 5 * self.F + 1, "wiener_spec": 2 * self.T * SPEC_LD * 2, "masks": 2 * self.T * self.F}.get(name, 1)
        a = np.empty(count, np.float32)
        hr = C.c_longlong(-2)
        n = self._chk(self.L.srtLiveCopyTensor(self.h, name.encode(), int(stem), int(index), C.c_void_p(a.ctypes.data), a.size, C.byref(hr)))
        if n == 0:
            return None, int(hr.value)
        if name == "wiener_spec":
            return a.view(np.complex64).reshape(2, self.T, SPEC_LD), int(hr.value)
        if name == "masks":
            return a.reshape(2, self.T, self.F), int(hr.value)
        return a, int(hr.value)

    def set_mix(self, G):
        """srtLiveSetMix: replace the matrix values (the same [n_out][S + 1]); holds from the next hop processed"""
        g = self._gain(G, self.outputs)
        self._chk(self.L.srtLiveSetMix(self.h, C.c_void_p(g.ctypes.data)))

    @property
    def latency(self):
        """samples between an input sample and its separated output (srtLiveLatency): for 1024-sample calls, or for any calls on a rate instance"""
        return self._chk(self.L.srtLiveLatency(self.h))

    def process(self, L, R, chunks=(1024,)):
        """Feed planar float32 L, R in calls of the sizes in `chunks` (cycled).  Returns (written [2P][m], timeline [2P][n]), P = outputs: the concatenation of what
        the calls wrote (the counts srtLiveProcess returned) and the same samples placed where each call's output starts in the caller's buffers
        (zero where nothing was written), the form tests/test_stream.py's _run builds for the plugin."""
        import numpy as np
        L = np.ascontiguousarray(L, np.float32)
        R = np.ascontiguousarray(R, np.float32)
        n = L.size
        assert R.size == n
        nc = 2 * self.outputs
        timeline = np.zeros((nc, n), np.float32)
        pieces = []
        pos = i = 0
        P = C.c_void_p * nc
        while pos < n:
            c = min(int(chunks[i % len(chunks)]), n - pos)
            i += 1
            w = self._chk(self.L.srtLiveProcess(self.h, C.c_void_p(L.ctypes.data + 4 * pos), C.c_void_p(R.ctypes.data + 4 * pos), c,
                                                P(*[timeline[j].ctypes.data + 4 * pos for j in range(nc)])))
            if w:
                pieces.append((pos, w))
            pos += c
        written = np.concatenate([timeline[:, p:p + w] for p, w in pieces], axis=1) if pieces else np.zeros((nc, 0), np.float32)
        return written, timeline

    def close(self):
        if getattr(self, "h", None):
            self.L.srtLiveDestroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Resampler:
    """Sample-rate conversion fs_in -> fs_out on the current device (srtResampler*, include/spleeterrt_amd.h): the reference program's
    libsamplerate sinc converter (main.c:264-271) on planar stereo fp32.  table=None: the built-in filter; otherwise a half filter in
    libsamplerate's layout (table_len floats, index_inc points per input sample), e.g. the reference's 22 438-point table."""

    def __init__(self, fs_in, fs_out, table=None, index_inc=491, stream=None):
        import numpy as np
        self.L = load_library()
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self._table = None if table is None else np.ascontiguousarray(table, np.float32)
        import torch
        if stream is None and torch.cuda.is_available():
            stream = torch.cuda.current_stream()
        self.stream = stream
        sp = None if stream is None else C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))
        h = C.c_void_p()
        tp = None if self._table is None else C.c_void_p(self._table.ctypes.data)
        self._chk(self.L.srtResamplerCreate(self.fs_in, self.fs_out, tp, 0 if self._table is None else self._table.size, int(index_inc), sp, C.byref(h)))
        self.h = h

    def _chk(self, rc):
        if rc < 0:
            raise EngineError("libspleeterrt_amd: %s (rc=%d)" % (self.L.srtLastError().decode(), rc))
        return rc

    def length(self, n):
        """output frames of an n-frame input: ceil(n * (fs_out / fs_in)), as main.c:266"""
        return self.L.srtResampleLength(int(n), self.fs_in, self.fs_out)

    def resample(self, L, R, out0=0, n_out=None, Lo=None, Ro=None):
        """CUDA float32 tensors [n] -> (Lo, Ro): output frames [out0, out0 + n_out) (default: all of them).  R may be L (mono)."""
        import torch
        assert L.is_cuda and L.dtype == torch.float32 and R.is_cuda and R.dtype == torch.float32 and L.numel() == R.numel()
        mono = R is L
        L = L.contiguous()
        R = L if mono else R.contiguous()
        n = L.numel()
        if n_out is None:
            n_out = max(self.length(n) - out0, 0)
        if Lo is None:
            Lo = torch.empty(n_out, device=L.device, dtype=torch.float32)
        if Ro is None:
            Ro = torch.empty(n_out, device=L.device, dtype=torch.float32)
        self._chk(self.L.srtResample(self.h, _ptr(L), _ptr(R), n, int(out0), int(n_out), _ptr(Lo), _ptr(Ro)))
        return Lo, Ro

    def resample_spans(self, a, a0, b, n_in, out0, n_out, out=None):
        """srtResampleSpans: output frames [out0, out0 + n_out) of the converted stream of a signal of n_in frames of which the device holds two consecutive spans.
        a: CUDA float32 [2 * pairs, a_len], rows L0, R0, L1, R1, .. holding frames [a0, a0 + a_len) (a0 may be negative); b: the same for the frames behind them, or
        None.  Rows may be views into a larger buffer (any row stride, unit column stride).  -> out [2 * pairs, n_out].  Every frame has resample()'s bits; raises
        when a weighted tap of a requested frame falls on a frame of [0, n_in) that neither span holds."""
        import torch

        def span(t):
            if t is None:
                return None, 0, 0
            assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == planes
            assert t.shape[1] == 0 or t.stride(1) == 1
            return (_ptr(t) if t.shape[1] else None), (t.stride(0) if t.shape[0] > 1 else t.shape[1]), t.shape[1]
        planes = a.shape[0]
        assert planes % 2 == 0 and planes >= 2
        pa, sa, la = span(a)
        pb, sb, lb = span(b)
        if out is None:
            out = torch.empty((planes, int(n_out)), device=a.device, dtype=torch.float32)
        po, so, lo = span(out)
        assert lo == n_out
        self._chk(self.L.srtResampleSpans(self.h, planes // 2, pa, sa, int(a0), la, pb, sb, lb, int(n_in), int(out0), int(n_out), po, so))
        return out

    def resample_host(self, L, R):
        """numpy float32 [n] x2 -> (Lo, Ro) numpy, the whole stream (synchronous)"""
        import numpy as np
        mono = R is L
        L = np.ascontiguousarray(L, np.float32)
        R = L if mono else np.ascontiguousarray(R, np.float32)
        assert L.size == R.size
        m = self.length(L.size)
        Lo, Ro = np.empty(m, np.float32), np.empty(m, np.float32)
        self._chk(self.L.srtResampleHost(self.h, C.c_void_p(L.ctypes.data), C.c_void_p(R.ctypes.data), L.size,
                                         C.c_void_p(Lo.ctypes.data), C.c_void_p(Ro.ctypes.data)))
        return Lo, Ro

    def close(self):
        if getattr(self, "h", None):
            self.L.srtResamplerDestroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResamplerStream:
    """The converter fed block by block (srtResamplerStream*, include/spleeterrt_amd.h): `channels` channels share one history ring on the device, every
    process() returns the frames that became computable, and the concatenation equals Resampler.resample of the whole input bit for bit."""

    def __init__(self, fs_in, fs_out, channels=2, max_block=4096, table=None, index_inc=491, stream=None):
        import numpy as np
        import torch
        self.L = load_library()
        self.fs_in, self.fs_out, self.channels, self.max_block = int(fs_in), int(fs_out), int(channels), int(max_block)
        self._table = None if table is None else np.ascontiguousarray(table, np.float32)
        if stream is None and torch.cuda.is_available():
            stream = torch.cuda.current_stream()
        self.stream = stream
        sp = None if stream is None else C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))
        tp = None if self._table is None else C.c_void_p(self._table.ctypes.data)
        h = C.c_void_p()
        self._chk(self.L.srtResamplerStreamCreate(self.fs_in, self.fs_out, self.channels, self.max_block, tp,
                                                  0 if self._table is None else self._table.size, int(index_inc), sp, C.byref(h)))
        self.h = h
        self.received = 0

    _chk = Resampler._chk

    @property
    def horizon(self):
        """H: output frame j needs the input up to frame floor(j * fs_in / fs_out) + H"""
        return self._chk(self.L.srtResamplerStreamHorizon(self.h))

    def computable(self, n_in):
        """frames a stream that has received n_in input frames can compute (srtResampleComputable)"""
        return self.L.srtResampleComputable(self.fs_in, self.fs_out, self.horizon, int(n_in))

    def process(self, x, interleaved=False):
        """x: CUDA float32 [channels, n] (planar) or [n, channels] (interleaved=True), n <= max_block -> [channels, k] newly computable frames"""
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
        x = x.contiguous()
        n = x.shape[0] if interleaved else x.shape[1]
        assert (x.shape[1] if interleaved else x.shape[0]) == self.channels
        k = self.computable(self.received + n) - self.computable(self.received)
        out = torch.empty((self.channels, k), device=x.device, dtype=torch.float32)
        got = self._chk(self.L.srtResamplerStreamProcess(self.h, _ptr(x), 0 if interleaved else n, n, _ptr(out), k))
        assert got == k, (got, k)
        self.received += n
        return out

    def flush(self):
        """the input has ended: the frames up to Resampler.length(received), zeros after the last input frame"""
        import torch
        k = max(self.L.srtResampleLength(self.received, self.fs_in, self.fs_out) - self.computable(self.received), 0)
        out = torch.empty((self.channels, k), device="cuda", dtype=torch.float32)
        got = self._chk(self.L.srtResamplerStreamFlush(self.h, _ptr(out), k))
        assert got == k, (got, k)
        return out

    def reset(self):
        self._chk(self.L.srtResamplerStreamReset(self.h))
        self.received = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.srtResamplerStreamDestroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pcm16_unpack(t):
    """int16 CUDA tensor [n, 2] (interleaved stereo) -> (L, R) float32 [n], x = q / 32768 (srtPcm16Unpack, on the tensor's device and the current stream)"""
    import torch
    assert t.is_cuda and t.dtype == torch.int16 and t.dim() == 2 and t.shape[1] == 2
    lib = load_library()
    t = t.contiguous()
    with torch.cuda.device(t.device):
        out = torch.empty((2, t.shape[0]), device=t.device, dtype=torch.float32)
        rc = lib.srtPcm16Unpack(C.c_void_p(torch.cuda.current_stream().cuda_stream), _ptr(t), t.shape[0], _ptr(out[0]), _ptr(out[1]))
    if rc < 0:
        raise EngineError("libspleeterrt_amd: %s (rc=%d)" % (lib.srtLastError().decode(), rc))
    return out[0], out[1]


def pcm16_pack(planes, clipped=None):
    """float32 CUDA tensor [pairs, 2, count] (planar stereo pairs) -> (int16 [pairs, count, 2], clipped int64 [pairs]); q = clamp(rint(x * 32768)), NaN -> 0
    (srtPcm16Pack).  clipped: an int64 CUDA tensor [pairs] the counts are ADDED to (default: zeros)."""
    import torch
    assert planes.is_cuda and planes.dtype == torch.float32 and planes.dim() == 3 and planes.shape[1] == 2
    lib = load_library()
    planes = planes.contiguous()
    pairs, count = planes.shape[0], planes.shape[2]
    with torch.cuda.device(planes.device):
        out = torch.empty((pairs, count, 2), device=planes.device, dtype=torch.int16)
        if clipped is None:
            clipped = torch.zeros(pairs, device=planes.device, dtype=torch.int64)
        assert clipped.is_cuda and clipped.dtype == torch.int64 and clipped.is_contiguous() and clipped.numel() == pairs
        rc = lib.srtPcm16Pack(C.c_void_p(torch.cuda.current_stream().cuda_stream), _ptr(planes), count, pairs, count, _ptr(out), count, _ptr(clipped))
    if rc < 0:
        raise EngineError("libspleeterrt_amd: %s (rc=%d)" % (lib.srtLastError().decode(), rc))
    return out, clipped


def pcm24_unpack(t):
    """uint8 CUDA tensor [n, 2, 3] (packed 24-bit interleaved stereo, little-endian) -> (L, R) float32 [n], x = q / 2^23 (srtPcm24Unpack, on the tensor's device
    and the current stream)"""
    import torch
    assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and tuple(t.shape[1:]) == (2, 3)
    lib = load_library()
    t = t.contiguous()
    with torch.cuda.device(t.device):
        out = torch.empty((2, t.shape[0]), device=t.device, dtype=torch.float32)
        rc = lib.srtPcm24Unpack(C.c_void_p(torch.cuda.current_stream().cuda_stream), _ptr(t), t.shape[0], _ptr(out[0]), _ptr(out[1]))
    if rc < 0:
        raise EngineError("libspleeterrt_amd: %s (rc=%d)" % (lib.srtLastError().decode(), rc))
    return out[0], out[1]


def pcm24_pack(planes, clipped=None):
    """float32 CUDA tensor [pairs, 2, count] (planar stereo pairs) -> (uint8 [pairs, count, 2, 3], clipped int64 [pairs]); q = clamp(rint(x * 2^23)), NaN -> 0
    (srtPcm24Pack).  clipped: an int64 CUDA tensor [pairs] the counts are ADDED to (default: zeros)."""
    import torch
    assert planes.is_cuda and planes.dtype == torch.float32 and planes.dim() == 3 and planes.shape[1] == 2
    lib = load_library()
    planes = planes.contiguous()
    pairs, count = planes.shape[0], planes.shape[2]
    with torch.cuda.device(planes.device):
        out = torch.empty((pairs, count, 2, 3), device=planes.device, dtype=torch.uint8)
        if clipped is None:
            clipped = torch.zeros(pairs, device=planes.device, dtype=torch.int64)
        assert clipped.is_cuda and clipped.dtype == torch.int64 and clipped.is_contiguous() and clipped.numel() == pairs
        rc = lib.srtPcm24Pack(C.c_void_p(torch.cuda.current_stream().cuda_stream), _ptr(planes), count, pairs, count, _ptr(out), count, _ptr(clipped))
    if rc < 0:
        raise EngineError("libspleeterrt_amd: %s (rc=%d)" % (lib.srtLastError().decode(), rc))
    return out, clipped


def pcm16_pack_dither(planes, seed=0, first_pair=0, first_index=0, clipped=None):
    """pcm16_pack with TPDF dither: q = clamp(rint(x * 32768 + d)), d of (seed, 2 * (first_pair + pair) + channel, first_index + sample) (srtPcm16PackDither;
    DESIGN.md §14.1) -> (int16 [pairs, count, 2], clipped int64 [pairs])."""
    import torch
    assert planes.is_cuda and planes.dtype == torch.float32 and planes.dim() == 3 and planes.shape[1] == 2
    lib = load_library()
    planes = planes.contiguous()
    pairs, count = planes.shape[0], planes.shape[2]
    with torch.cuda.device(planes.device):
        out = torch.empty((pairs, count, 2), device=planes.device, dtype=torch.int16)
        if clipped is None:
            clipped = torch.zeros(pairs, device=planes.device, dtype=torch.int64)
        assert clipped.is_cuda and clipped.dtype == torch.int64 and clipped.is_contiguous() and clipped.numel() == pairs
        rc = lib.srtPcm16PackDither(C.c_void_p(torch.cuda.current_stream().cuda_stream), _ptr(planes), count, pairs, count, _ptr(out), count, _ptr(clipped),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_pair), int(first_index))
    if rc < 0:
        raise EngineError("libspleeterrt_amd: %s (rc=%d)" % (lib.srtLastError().decode(), rc))
    return out, clipped
