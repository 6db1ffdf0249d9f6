"""The RCCL branch of the data-parallel path (val.py:98,135 -> racformer_amd/dp.py, bench.py) on the one GPU of the test box:
a FRESH child process initialises the ``nccl`` (= RCCL) process group with ``device_id`` at world size 1, runs real bench
steps with the all-gather forced (``--force-collective`` bypasses the world-1 short-circuit of dp.all_gather_detections),
checks that the gathered block equals the local one and tears the group down; the parent only reads its exit status and
JSON line.  No scaling number can come from one GPU -- this pins that the code the driver's 8-GPU run will execute first
has executed at all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("graph", [True, False], ids=["captured", "eager"])
def test_bench_step_with_forced_rccl_all_gather(graph, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    # --full: the gathered-block check (`collective`) runs after the timed region, which a plain run leaves out
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
           "--no-stress", "--force-collective", "--dump-outputs", str(tmp_path)] + ([] if graph else ["--no-graph"])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    c = line["collective"]
    assert c["backend"] == "nccl" and c["world"] == 1 and c["forced_at_world_1"] is True
    assert c["gathered_shape"] == [1, 1, 300, 11] and c["own_slot_equals_local"] is True
    assert line["value"] > 0 and line["n_gpus"] == 1
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    # --dump-outputs: the last timed step's outputs, float32, finite, in the shapes a caller receives
    shapes = {"all_cls_scores": (6, 1, 900, 10), "all_bbox_preds": (6, 1, 900, 10), "detections": (1, 1, 300, 11)}
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in shapes)
    for name, shape in shapes.items():
        a = np.load(os.path.join(tmp_path, name + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), (name, a.dtype, a.shape)
