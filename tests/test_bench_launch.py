"""`bench.py --gpus N` is binding: it starts the N ranks itself when no launcher did, refuses to print a line for fewer
devices than asked, and refuses a launcher world that differs from N.  CPU-only here: the rendezvous half (`--rendezvous-only`, hidden flag)
joins a real gloo world of 2 through the same torch.distributed.run command the GPU path uses; the GPU halves are in tests/test_rccl.py.
Also: what a plain run prints (the headline only; the rest comes with --full) and what --dump-outputs writes."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**extra):
    env = dict(os.environ, **extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    return env


def _cpu_only_env():
    return _env(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # also on a GPU box: no device visible


def test_more_gpus_than_devices_fails_loudly():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0"], cwd=ROOT, env=_cpu_only_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--gpus 2 but 0 GPU(s) visible" in r.stderr, r.stderr[-800:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]                    # and no JSON line at all
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--host", "native", "--steps", "1", "--warmup", "0"], cwd=ROOT, env=_cpu_only_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--gpus 2 --host native but 0 GPU(s) visible" in r.stderr, r.stderr[-800:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_launcher_world_must_equal_gpus():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "8"], cwd=ROOT, env=dict(_env(), RANK="0", WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--gpus 8 but the launcher started WORLD_SIZE=2" in r.stderr, r.stderr[-800:]


def test_gpus_2_without_a_launcher_starts_two_ranks():
    """python bench.py --gpus 2 (no RANK/WORLD_SIZE in the environment) re-launches itself under torch.distributed.run with two ranks, which meet
    in a process group (gloo here) and all-reduce: rank_sum 1 + 2 = 3 proves both were there."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--rendezvous-only"], cwd=ROOT, env=_cpu_only_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d == {"rendezvous": True, "world": 2, "n_gpus": 2, "backend": "gloo", "rank_sum": 3.0}


def test_up6_streamed_f16_kernel_is_priced_against_the_fp16_peak():
    """the fp16 modes run up6 as srt_up6_stream_kernel<.., .., .., true> (v_mfma_f32_32x32x16_f16)."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.is_f16_kernel("srt_up6_stream_kernel<64, 2, 0, true>") and bench.mfma_peak("srt_up6_stream_kernel<64, 2, 0, true>") == 2500.0
    assert not bench.is_f16_kernel("srt_up6_stream_kernel<64, 2, 0, false>") and bench.mfma_peak("srt_up6_stream_kernel<64, 2, 0, false>") == 157.3
    assert bench.layer_bytes("down1", "f32", False, 5) < bench.layer_bytes("down1", "f32", False, 4)      # the magnitudes are shared by the stems


def test_plain_line_is_the_headline_only():
    """Without --full the line is built from the timed steps alone: ms_per_step = wall time / --steps, value = x real-time of the frames the
    steps transformed, and none of the per-kernel / roofline / CPU-baseline fields (they need runs of their own)."""
    sys.path.insert(0, ROOT)
    import bench
    a = SimpleNamespace(stems=4, steps=7, warmup=2, tiles=bench.TILES, impl="mfma", precision="f32", full=False)
    rec = {"dt": 0.07, "dt_ev": None, "tim": [], "kern": [], "world": 1, "rows": 16387, "frames_step": 16384,
           "host": "one process per GPU (torch.distributed)", "distributed": None}
    d = bench.make_line(a, rec)
    assert d["ms_per_step"] == pytest.approx(10.0) and d["steps"] == 7 and d["warmup"] == 2
    assert d["frames_per_s"] == pytest.approx(16384 * 7 / 0.07) and d["value"] == pytest.approx(d["frames_per_s"] * bench.HOP / bench.FS)
    assert d["unit"] == "x real-time" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"].startswith("x_realtime")
    assert not {"roofline", "kernel_ms", "layer_kernels", "cpu_baseline", "ms_per_step_events", "nn_stack"} & set(d)


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    """bench.py --dump-outputs DIR: the stems of the last timed step (a fixed sample, float32, <= 64 MB) as DIR/stems.npy; two runs with the
    same arguments write the same arrays.  The plain line holds the headline only."""
    outs = []
    for i in range(2):
        d = tmp_path / str(i)
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)], cwd=ROOT, env=_env(),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0 and line["dtype"] == "f32"
        assert not {"roofline", "kernel_ms", "cpu_baseline", "ms_per_step_events"} & set(line)
        assert os.listdir(d) == ["stems.npy"]
        outs.append(np.load(d / "stems.npy"))
    a, b = outs
    assert a.dtype == np.float32 and a.shape == (4, 2, 1 << 20) and a.nbytes <= 64 << 20
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a, b)
