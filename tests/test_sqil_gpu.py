"""`SQIL.train` end to end on the device against the fixtures the reference's own SQIL produced
(`tests/golden/make_golden_sqil.py`): every action, branch, ring write, sampled index, exploration rate, target update,
logger key and counter exactly; losses, the Q-values of the greedy rows and the final parameters within the stored
`8 x dref` (dref = the relative L2 deviation of the reference's float32 run from its float64 run, per tensor)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from tests import sqil_golden as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("ring_pos", "ring_obs", "ring_next_obs", "ring_action", "ring_done", "sample_rows", "actions", "branches",
         "exploration_rate", "target_updates", "train_n_calls", "train_lr", "n_dumps")
_runs = {}


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def run(name):
    if name not in _runs:
        _runs[name] = sg.run_case(name, json.loads(str(golden(name)["cfg"]))["seed"])
    return _runs[name]


def expected_exact(g, cfg):
    n_envs = cfg["n_envs"]
    want = {k: g[k] for k in EXACT if k != "sample_rows"}
    want["ring_action"] = g["ring_action"].reshape(len(g["ring_pos"]), n_envs)
    want["sample_rows"] = np.concatenate([g["sample_new_pos"] * n_envs + g["sample_new_env"],
                                          g["sample_expert_pos"] + g["sample_expert_env"]], axis=1)
    return want


def check_exact(got, g, cfg):
    want = expected_exact(g, cfg)
    for k in EXACT:
        assert np.array_equal(np.asarray(got[k]), want[k]), k
    for k in g.files:
        if k.startswith("counter/"):
            assert int(got[k]) == int(g[k]), k
        if k.startswith("init/"):
            assert np.array_equal(got[k], g[k]), k
    # the ring in device memory is what those writes leave behind (reward 0 everywhere)
    n_envs, D = cfg["n_envs"], cfg["obs_dim"]
    ring = {k: np.zeros_like(got[f"table_{k}"]) for k in ("obs", "next_obs", "action", "reward", "done")}
    for i, pos in enumerate(g["ring_pos"]):
        rows = slice(pos * n_envs, (pos + 1) * n_envs)
        ring["obs"][rows], ring["next_obs"][rows] = g["ring_obs"][i], g["ring_next_obs"][i]
        ring["action"][rows], ring["done"][rows] = g["ring_action"][i].reshape(-1), g["ring_done"][i]
        assert np.array_equal(g["ring_reward"][i], np.zeros(n_envs, np.float32))
    for k, v in ring.items():
        assert np.array_equal(got[f"table_{k}"], v), k
    assert ring["obs"].shape == (cfg["buffer_size"], D)
    for j in range(int(g["n_dumps"])):
        assert int(got[f"dump{j}_step"]) == int(g[f"dump{j}_step"])
        keys = [str(k) for k in g[f"dump{j}_keys"]]
        assert [str(k) for k in got[f"dump{j}_keys"]] == keys
        for k, a, b in zip(keys, got[f"dump{j}_vals"], g[f"dump{j}_vals64"]):
            if k not in sg.NOT_COMPARED and k != "train/loss":
                assert a == b, (j, k, a, b)


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("name", list(sg.CASES))
def test_sqil_train_matches_the_reference_run(name):
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    got = run(name)
    pol_fused = len(cfg["net_arch"]) == 2
    # the path `SQIL.train` really took: the one-launch kernel on the fused shapes, the general kernels otherwise
    n_calls = len(np.unique(g["train_n_calls"]))
    assert (int(got["fused_calls"]), int(got["general_calls"])) == ((n_calls, 0) if pol_fused else (0, n_calls))
    check_exact(got, g, cfg)
    worst = []
    for k in (f[len("dref/"):] for f in g.files if f.startswith("dref/")):
        dref, dev = float(g[f"dref/{k}"]), rel(got[k], g[f"f64/{k}"])
        print(f"{name} {k}: dref {dref:.3e}, device {dev:.3e} ({dev / dref:.2f} x; fused kernel: {pol_fused})")
        if dev > 8 * dref:
            worst.append((k, dev, dref))
    assert not worst, worst
    for j in range(int(g["n_dumps"])):   # train/loss of a dump: the mean over the call's steps
        keys = [str(k) for k in g[f"dump{j}_keys"]]
        if "train/loss" in keys:
            i = keys.index("train/loss")
            assert abs(got[f"dump{j}_vals"][i] - g[f"dump{j}_vals64"][i]) <= 8 * float(g["dref/loss"]) * abs(g[f"dump{j}_vals64"][i])


@pytest.mark.parametrize("name", [n for n, c in sg.CASES.items() if len(c["net_arch"]) == 2])
def test_general_path_takes_the_same_decisions(name, tmp_path):
    """The fused-shape cases again with `IA_DQN_FUSED=0`, in a fresh process: identical exact keys."""
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    out = str(tmp_path / "general.npz")
    env = dict(os.environ, IA_DQN_FUSED="0")
    subprocess.run([sys.executable, "-m", "tests.sqil_golden", name, str(cfg["seed"]), out], check=True, cwd=ROOT, env=env,
                   timeout=300)
    general, fused = np.load(out), run(name)
    assert int(general["fused_calls"]) == 0 and int(general["general_calls"]) == int(fused["fused_calls"]) > 0
    check_exact(general, g, cfg)
    for k in EXACT + ("table_obs", "table_next_obs", "table_action", "table_done"):
        assert np.array_equal(general[k], fused[k]), k
    for k in ("loss", "final/q_net.q_net.0.weight"):   # both are the same training run up to float32 rounding
        assert rel(general[k], fused[k]) <= 2 * 8 * float(g[f"dref/{k}"]), k
    assert not np.array_equal(general["final/q_net.q_net.0.weight"], g["init/q_net.q_net.0.weight"])


def test_set_demonstrations_between_train_calls_and_continued_timesteps():
    cfg = dict(sg.COMMON, **sg.CASES["sqil_cartpole_shape"])
    algo, rec = sg.build(cfg, seed=3)
    rl = algo.rl_algo
    algo.train(total_timesteps=40, log_interval=None)   # (a rollout is train_freq * n_envs = 16 timesteps: 48 is reached)
    assert rl.num_timesteps == 48 and rl.replay_buffer.expert.rows == cfg["n_demo"]
    n_rows = len(rec.rows)
    assert max(r[:, 4:].max() for r in rec.rows) < cfg["n_demo"]
    r = np.random.default_rng(0)
    more = p.Transitions(obs=r.normal(size=(500, 4)).astype(np.float32), acts=r.integers(0, 2, 500),
                         next_obs=r.normal(size=(500, 4)).astype(np.float32), dones=np.zeros(500, bool))
    algo.set_demonstrations(more)
    assert rl.replay_buffer.expert.rows == 500
    before = rl.policy.q_net._flat.clone()
    algo.train(total_timesteps=40, log_interval=None, reset_num_timesteps=False)
    assert rl.num_timesteps == 96 and rl._total_timesteps == 88   # ([SB3]: `reset_num_timesteps=False` continues the count)
    new_rows = np.concatenate(rec.rows[n_rows:])
    assert len(rec.rows) > n_rows and new_rows[:, 4:].max() >= cfg["n_demo"]   # the next samples index the new table
    assert new_rows[:, :4].max() < cfg["buffer_size"]
    assert not th.equal(rl.policy.q_net._flat, before) and bool(th.isfinite(rl.policy.q_net._flat).all())
    algo.train(total_timesteps=16, log_interval=None)   # the default resets the count, as SB3's `learn` does
    assert rl.num_timesteps == 16
