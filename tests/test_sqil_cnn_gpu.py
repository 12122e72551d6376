"""`SQIL(policy="CnnPolicy").train` end to end on the device against the fixtures the reference's own SQIL produced over the
torch restatement of SB3's DQN `CnnPolicy` (`tests/golden/make_golden_sqil_cnn.py`): every ring position, the CRCs of
every ring write as the DEVICE ring holds it, actions, branches, sampled rows, exploration rates, target updates, counters
and dump keys exactly; losses, the Q-values of the greedy rows, the final online parameters and the dump values within
`8 x dref` of the float64 run; the final target net equal to the online net at the last target update; plus a plain
`DQN("CnnPolicy")` run whose ring fills and wraps."""
import json
import os

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from tests import sqil_cnn_golden as cg
from tests import sqil_golden as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("ring_pos", "ring_obs_crc", "ring_next_obs_crc", "ring_action", "ring_done", "sample_rows", "actions", "branches",
         "exploration_rate", "target_updates", "train_n_calls", "train_lr", "n_dumps")
_runs = {}


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def run(name):
    if name not in _runs:
        _runs[name] = cg.run_case(name, json.loads(str(golden(name)["cfg"]))["seed"])
    return _runs[name]


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check_exact(got, g, cfg):
    n_envs = cfg["n_envs"]
    assert int(g["demo_crc"]) == cg.demo_crc(cfg, cfg["seed"])   # the regenerated demonstrations are the fixture's
    want = {k: g[k] for k in EXACT if k != "sample_rows"}
    want["ring_action"] = g["ring_action"].reshape(len(g["ring_pos"]), n_envs)
    want["sample_rows"] = np.concatenate([g["sample_new_pos"] * n_envs + g["sample_new_env"],
                                          g["sample_expert_pos"] + g["sample_expert_env"]], axis=1)
    for k in EXACT:
        assert np.array_equal(np.asarray(got[k]), want[k]), k
    for k in g.files:
        if k.startswith("counter/"):
            assert int(got[k]) == int(g[k]), k
        if k.startswith("init/"):   # (the fixture holds the online net; the target starts equal to it)
            assert np.array_equal(got[k], g[k]), k
            assert np.array_equal(got["init/q_net_target." + k[len("init/q_net."):]], g[k]), k
    # what those writes leave in the device ring's small columns (reward 0 everywhere)
    ring = {k: np.zeros_like(got[f"table_{k}"]) for k in ("action", "reward", "done")}
    for i, pos in enumerate(g["ring_pos"]):
        rows = slice(pos * n_envs, (pos + 1) * n_envs)
        ring["action"][rows], ring["done"][rows] = g["ring_action"][i].reshape(-1), g["ring_done"][i]
        assert np.array_equal(g["ring_reward"][i], np.zeros(n_envs, np.float32))
    for k, v in ring.items():
        assert np.array_equal(got[f"table_{k}"], v), k
    for j in range(int(g["n_dumps"])):
        assert int(got[f"dump{j}_step"]) == int(g[f"dump{j}_step"])
        keys = [str(k) for k in g[f"dump{j}_keys"]]
        assert [str(k) for k in got[f"dump{j}_keys"]] == keys
        for k, a, b in zip(keys, got[f"dump{j}_vals"], g[f"dump{j}_vals64"]):
            if k not in sg.NOT_COMPARED and k != "train/loss":
                assert a == b, (j, k, a, b)


@pytest.mark.parametrize("name", list(cg.CASES))
def test_sqil_cnn_train_matches_the_reference_run(name):
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    got = run(name)
    # the path `SQIL.train` really took: `update_frames` every call, the flat-observation routes never
    n_calls = len(np.unique(g["train_n_calls"]))
    assert (int(got["frames_calls"]), int(got["fused_calls"]), int(got["general_calls"])) == (n_calls, 0, 0)
    check_exact(got, g, cfg)
    worst = []
    for k in (f[len("dref/"):] for f in g.files if f.startswith("dref/")):
        dref, dev = float(g[f"dref/{k}"]), rel(got[k], g[f"f64/{k}"])
        print(f"{name} {k}: dref {dref:.3e}, device {dev:.3e} ({dev / dref:.2f} x)")
        if dev > 8 * dref:
            worst.append((k, dev, dref))
    assert not worst, worst
    for j in range(int(g["n_dumps"])):   # train/loss of a dump: the mean over the call's steps
        keys = [str(k) for k in g[f"dump{j}_keys"]]
        if "train/loss" in keys:
            i = keys.index("train/loss")
            assert abs(got[f"dump{j}_vals"][i] - g[f"dump{j}_vals64"][i]) <= 8 * float(g["dref/loss"]) * abs(g[f"dump{j}_vals64"][i])
    # tau = 1: the final target is, bit for bit, the online net as it stood at the last recorded target update
    assert len(g["target_updates"]) > 0
    snap = {k[len("target_snapshot/"):]: v for k, v in got.items() if k.startswith("target_snapshot/")}
    assert len(snap) == 10
    for k, v in snap.items():
        assert np.array_equal(got[f"final/q_net_target.{k}"], v.astype(np.float64)), k
    assert not np.array_equal(got["final/q_net.q_net.0.weight"], g["init/q_net.q_net.0.weight"].astype(np.float64))


def test_plain_dqn_cnn_fills_and_wraps_its_ring():
    """No expert table (`n_new == B`): finite losses, a ring that is full and has wrapped."""
    cfg = dict(sg.COMMON, **cg.CASES["sqil_cnn_min"])
    venv = cg.make_env(cfg, 1)
    cg.seed_everything(venv, 1)
    rl = p.DQN("CnnPolicy", venv, device="cuda", **cg.rl_kwargs_of(cfg))
    rl.set_logger(p.logger.Logger(None, []))
    losses, n_new, frames_calls = [], [], []
    train, update_frames = rl.train, rl.policy.update_frames

    def counted(*a, **k):
        frames_calls.append(1)
        return update_frames(*a, **k)

    def noted(*a, **k):
        train(*a, **k)
        losses.append(rl.last_train_stats.copy())
        n_new.append(rl.last_n_new)

    rl.train, rl.policy.update_frames = noted, counted
    before = rl.policy.q_net._flat.clone()
    rl.learn(total_timesteps=cfg["total_timesteps"], log_interval=None)
    rb = rl.replay_buffer
    assert rl.num_timesteps == 208 and rb.full and rb.buffer_size == 16 and rb.pos == 52 % 16   # 52 writes into 16 positions
    assert rb.expert_table() is None and set(n_new) == {cfg["batch_size"]} and len(frames_calls) == len(losses) > 0
    assert np.isfinite(np.concatenate(losses)).all()
    assert rb.table.obs.dtype == th.uint8 and int(rb.table.obs.max()) > 0
    flat = rl.policy.q_net._flat
    assert bool(th.isfinite(flat).all()) and not th.equal(flat, before)
