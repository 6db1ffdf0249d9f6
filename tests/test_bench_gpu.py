"""A plain `bench.py --gpus 1` run, the form every change is measured with: the default step (captured plans, four samples in
flight) is warmed up and timed, the last timed step's outputs are dumped, and the one JSON line carries the headline and none
of what only `--full` measures after the timed region."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"collective", "one_sample_in_flight", "lanes_match_single_plan_bitwise", "roofline", "mfma", "roofline_stress",
             "pregrouped_producer_layout", "bev_values_int16_block", "cpu_baseline", "parity_vs_oracle"}


def test_plain_run_times_dumps_and_prints_the_headline_only(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "8", "--warmup", "4",
           "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["metric"] == "samples/sec (6-cam 704x256, 900 queries, f8)" and line["unit"] == "samples/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["n_gpus"] == 1
    assert line["steps"] == 8 and line["warmup"] == 4 and line["config"]["samples_in_flight_per_gpu"] == 4
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6
    assert not FULL_ONLY & set(line), sorted(FULL_ONLY & set(line))
    shapes = {"all_cls_scores": (6, 1, 900, 10), "all_bbox_preds": (6, 1, 900, 10), "detections": (1, 1, 300, 11)}
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in shapes)
    for name, shape in shapes.items():
        a = np.load(os.path.join(tmp_path, name + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), (name, a.dtype, a.shape)
