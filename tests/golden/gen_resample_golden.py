"""Regenerate tests/golden/resample_reference.npz from the reference program's own sample-rate converter.

    python tests/golden/gen_resample_golden.py [REFERENCE_TREE]

Run by hand where the reference tree exists (default /root/reference); no test runs it.  It compiles, in a temporary
directory outside the repository:
  * Executable/main.c with -Dmain=ref_program_main, against a stub model.c (the reference's weights are not public) that
    only defines `coeffQuantized`, and a stub openblas_set_num_threads;
  * libsamplerate/samplerate.c and libsamplerate/src_sinc.c;
  * the five hot-path files main.c links against, with -DCPU_GEMM=1 (the in-tree GEMM).
Through ctypes it then rebuilds the 22 438-point sinc table with decompressResamplerMQ (the 701 knots are read out of
main.c's text at run time) and converts seeded stereo clips with JamesDSPOfflineResampling (main.c:264-271).  src_simple
is called once more on the same data to record how many frames the reference generated (it can leave the last one at 0).

The fixture holds only data: the table the reference program computes at start-up, and inputs / outputs of the runs.
"""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resample_reference.npz")
# (fs_in, fs_out, frames, seed): odd lengths of a few thousand frames, every direction the tests need
CASES = [(8000, 44100, 1501, 11), (22050, 44100, 2999, 12), (32000, 44100, 3001, 13), (44056, 44100, 2003, 14),
         (48000, 44100, 4001, 15), (96000, 44100, 3000, 16), (192000, 44100, 4003, 17), (44100, 48000, 3001, 18)]


class SRC_DATA(C.Structure):
    _fields_ = [("data_in", C.c_void_p), ("data_out", C.c_void_p), ("input_frames", C.c_long), ("output_frames", C.c_long),
                ("input_frames_used", C.c_long), ("output_frames_gen", C.c_long), ("end_of_input", C.c_int), ("src_ratio", C.c_double)]


def build(ref, tmp):
    exe = os.path.join(ref, "Executable")
    with open(os.path.join(tmp, "model.c"), "w") as f:
        f.write("static const void *coeffQuantized = 0;\n")
    with open(os.path.join(tmp, "stub.c"), "w") as f:
        f.write("void openblas_set_num_threads(int n) { (void)n; }\n")
    so = os.path.join(tmp, "libref_resample.so")
    srcs = [os.path.join(exe, "main.c"), os.path.join(exe, "libsamplerate", "samplerate.c"), os.path.join(exe, "libsamplerate", "src_sinc.c"),
            os.path.join(tmp, "stub.c")] + [os.path.join(exe, f) for f in ("spleeter.c", "gemm.c", "im2col_dilated.c", "stftFix.c", "codelet.c")]
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-w", "-DCPU_GEMM=1", "-Dmain=ref_program_main", "-I" + tmp, "-I" + exe,
                           "-o", so] + srcs + ["-lm", "-lpthread"])
    return so


def signal(n, fs, seed):
    """seeded noise plus tones, L != R"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    top = min(fs, 44100) * 0.45
    L = 0.25 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 997.0 * t) + 0.2 * np.sin(2 * np.pi * 0.61 * top * t + 1.0)
    R = 0.2 * rng.standard_normal(n) + 0.35 * np.sin(2 * np.pi * 440.0 * t + 0.5) + 0.15 * np.sin(2 * np.pi * 0.93 * top * t)
    return np.stack([L, R], 1).astype(np.float32)


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        L = C.CDLL(build(ref, tmp))
        txt = open(os.path.join(ref, "Executable", "main.c")).read()
        m = re.search(r"compressedCoeffMQ\[701\]\s*=\s*\{([^}]*)\}", txt)
        knots = np.array([float(v) for v in m.group(1).split(",")], np.float64)
        assert knots.size == 701
        table = np.zeros(22438, np.float32)
        L.decompressResamplerMQ(C.c_void_p(knots.ctypes.data), C.c_void_p(table.ctypes.data))
        C.c_void_p.in_dll(L, "decompressedCoefficients").value = table.ctypes.data
        L.JamesDSPOfflineResampling.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_double]
        L.src_simple.argtypes = [C.POINTER(SRC_DATA), C.c_int, C.c_int]
        data = {"table": table, "index_inc": np.int32(491), "rates": np.array([c[:2] for c in CASES], np.int32)}
        for k, (fs_in, fs_out, n, seed) in enumerate(CASES):
            x = signal(n, fs_in, seed)
            ratio = fs_out / float(fs_in)
            nout = int(math.ceil(n * ratio))                       # main.c:266
            y = np.zeros((nout, 2), np.float32)
            L.JamesDSPOfflineResampling(x.ctypes.data, y.ctypes.data, n, nout, 2, ratio)
            y2 = np.zeros((nout, 2), np.float32)
            d = SRC_DATA(x.ctypes.data, y2.ctypes.data, n, nout, 0, 0, 0, ratio)
            assert L.src_simple(C.byref(d), 0, 2) == 0
            assert np.array_equal(y, y2)
            data["in%d" % k], data["out%d" % k], data["gen%d" % k] = x, y, np.int64(d.output_frames_gen)
            print("%6d -> %6d Hz: %d -> %d frames, %d generated" % (fs_in, fs_out, n, nout, d.output_frames_gen))
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
