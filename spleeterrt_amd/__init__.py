"""spleeterrt_amd — MI355X-native engine for SpleeterRT's STFT -> U-Net mask -> iSTFT hot path.

The product is the C-ABI shared library `libspleeterrt_amd.so` (hand-written HIP for gfx950, see csrc/ and
include/*.h).  This package only holds the build script and a thin ctypes binding used by tests and bench.py;
PyTorch appears solely as the owner of device memory / streams / torch.distributed.
"""
from .capi import Engine, EngineError, Live, Resampler, ResamplerStream, live_latency, live_rate_latency, load_library, VARIANT_EXE, VARIANT_VST, IMPL_MFMA, IMPL_NAIVE, PREC_F32, PREC_F16, PREC_F16X2, HOST_PINNED, HOST_IN_PCM16, HOST_OUT_PCM16, HOST_IN_PCM24, HOST_OUT_PCM24, HOST_OUT_DITHER, MASK_EXT_CONSTANT, MASK_EXT_AVERAGE, pcm16_pack, pcm16_unpack, pcm24_pack, pcm24_unpack, pcm16_pack_dither  # noqa: F401
