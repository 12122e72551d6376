"""`bench.py` on one GPU (`-m gpu`): a plain run prints the headline line and nothing of `--full`; `--dump-outputs`
writes what the last timed round computed, and two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    if not th.cuda.is_available():
        pytest.skip("no GPU")
    outs = [_plain_run(tmp_path / f"d{i}") for i in range(2)]
    for out in outs:
        assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
        assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(16384 * 1e3 / out["ms_per_step"], rel=1e-9)
        assert out["roofline"] is None and out["variants"] is None and out["cpu_baseline"] is None
        assert out["value_long"] is None
    names = sorted(os.listdir(tmp_path / "d0"))
    assert names == sorted(os.listdir(tmp_path / "d1"))
    for must in ("disc.mlp.dense0.weight.npy", "policy.action_net.weight.npy", "rollout.rewards.npy",
                 "replay.obs.npy", "reward_train_predict.npy"):
        assert must in names, must
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "d0" / n), np.load(tmp_path / "d1" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape, n
        assert np.isfinite(a).all(), n
        total += a.nbytes
        # same seeds, same inputs: the arrays of two runs agree (measured: bit for bit)
        np.testing.assert_allclose(a, b, rtol=2e-4, atol=5e-5, err_msg=n)
    assert total <= 64 << 20
