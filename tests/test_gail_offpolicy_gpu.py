"""GAIL with an off-policy generator (DQN, TD3) end to end on the device against the fixtures the reference's own GAIL
produced over the restated learners (`tests/golden/make_golden_gail_offpolicy.py`).

Exactly: every ring write position, raw done and time-limit flag, every branch, every sampled index row, exploration
rates, target updates, the trainer's ring positions and dones after every round, counters, the initial parameters, the
logger's dump steps and keys -- and, with Discrete actions, every action and the obs / next_obs / action columns of both
rings. With Box actions those rows follow the actor's float32 output (the warm-up rows, which no net touches, are still
compared exactly). The learner's ring is also read back from device memory and compared bit for bit with the ring the write
positions and rows rebuild (`check_table`), on the fused and on the host path, and the two paths' device rings with each other. Floating values (rewards in the learner ring, losses, Q-values of the greedy rows, logger values, final
parameters of both nets, and with Box actions the rows) by relative L2 against the float64 run within `8 x dref`, dref =
the deviation of the reference's float32 run from its float64 run per key; a key whose dref is 0 within float32 epsilon.
Final parameters are one key per tensor, a one-element tensor keyed together with its layer's weight."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import imitation_amd as p
from tests import gail_offpolicy_golden as gg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX_KEYS = ("ring_pos", "ring_done", "ring_timeout", "branches", "sample_rows", "train_at", "gen_dones", "gen_idx",
              "gen_n_data", "n_dumps", "exploration_rate", "target_updates", "disc_norm_count")
ROW_KEYS = gg.EXACT_DQN
EPS32 = float(np.finfo(np.float32).eps)
_runs = {}


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def run(name):
    if name not in _runs:
        _runs[name] = gg.run_case(name, json.loads(str(golden(name)["cfg"]))["seed"])
    return _runs[name]


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check_exact(got, g, cfg):
    for k in INDEX_KEYS:
        if k in g.files:
            assert np.array_equal(np.asarray(got[k]), g[k]), k
    warm = g["branches"] == gg.BRANCH["warmup"]
    assert warm.any() and not warm.all()
    for k in ROW_KEYS:
        if gg.is_exact(cfg, k):
            assert np.array_equal(np.asarray(got[k]), g[k]), k
        elif k.startswith(("ring_", "actions")):   # Box actions: the warm-up rows, which no net had a hand in
            n_warm = int(warm.sum())
            assert warm[:n_warm].all()
            assert np.array_equal(np.asarray(got[k], np.float32)[:n_warm], np.asarray(g["f32/" + k])[:n_warm]), k
    for k in g.files:
        if k.startswith("counter/"):
            assert int(got[k]) == int(g[k]), k
        if k.startswith(("init/", "disc_init/")):
            assert np.array_equal(got[k], g[k]), k
    for j in range(int(g["n_dumps"])):
        assert int(got[f"dump{j}_step"]) == int(g[f"dump{j}_step"]), j
        assert [str(k) for k in got[f"dump{j}_keys"]] == [str(k) for k in g[f"dump{j}_keys"]], j


def check_table(got, g, cfg):
    """The learner's ring as it lies in DEVICE memory is what the writes leave behind: rebuilt from the write positions and
    the rows (the fixture's with Discrete actions; the run's own tapped rows with Box actions, whose rows are float keys),
    SB3's scaled action in the action column and `done * (1 - timeout)` in the done column, compared bit for bit."""
    n = cfg["n_envs"]
    exact = cfg["algo"] == "DQN"
    rows = {k: np.asarray(g[k] if exact else got[k]) for k in ("ring_obs", "ring_next_obs", "ring_action")}
    want = {k: np.zeros_like(got[f"table_{k}"]) for k in ("obs", "next_obs", "action", "done")}
    rew = np.zeros(want["done"].shape, np.float64)
    for i, pos in enumerate(g["ring_pos"]):
        sl = slice(pos * n, (pos + 1) * n)
        want["obs"][sl], want["next_obs"][sl] = rows["ring_obs"][i], rows["ring_next_obs"][i]
        want["action"][sl] = rows["ring_action"][i].reshape(want["action"][sl].shape)
        want["done"][sl] = g["ring_done"][i] * (1 - g["ring_timeout"][i])
        rew[sl] = got["ring_reward"][i]
    assert (g["ring_done"] * (1 - g["ring_timeout"]) != g["ring_done"]).any()   # the two dones differ somewhere
    assert len(set(g["ring_pos"].tolist())) < len(g["ring_pos"])                 # the ring wrapped: rows were overwritten
    for k, v in want.items():
        assert got[f"table_{k}"].dtype == v.dtype and np.array_equal(got[f"table_{k}"], v), k
    assert np.array_equal(got["table_reward"].astype(np.float64), rew)


def check_floats(got, g, name):
    worst = []
    for k in (f[len("dref/"):] for f in g.files if f.startswith("dref/")):
        dref, dev = float(g[f"dref/{k}"]), rel(got[k], g[f"f64/{k}"])
        print(f"{name} {k}: dref {dref:.3e}, device {dev:.3e}")
        if dev > (8 * dref if dref > 0 else EPS32):
            worst.append((k, dev, dref))
    # logger values, per key over all of its dumps
    per_key = {}
    for j in range(int(g["n_dumps"])):
        for k, a, b in zip(g[f"dump{j}_keys"], got[f"dump{j}_vals"], g[f"dump{j}_vals64"]):
            per_key.setdefault(str(k), ([], []))
            per_key[str(k)][0].append(a)
            per_key[str(k)][1].append(b)
    for k, dref in zip(g["log_keys"], g["log_dref"]):
        dev = rel(*per_key[str(k)])
        print(f"{name} log {k}: dref {float(dref):.3e}, device {dev:.3e}")
        if dev > (8 * float(dref) if float(dref) > 0 else EPS32):
            worst.append((str(k), dev, float(dref)))
    assert not worst, worst


@pytest.mark.parametrize("name", list(gg.CASES))
def test_gail_with_an_offpolicy_generator_matches_the_reference_run(name):
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    got = run(name)
    steps = cfg["rounds"] * cfg["gen_train_timesteps"] // cfg["n_envs"]
    # the fused path: one launch per environment step, no per-step reward prediction with its read-back
    assert len(g["ring_pos"]) == steps
    assert int(got["step_launches"]) == steps and int(got["reward_fn_calls"]) == 0
    check_exact(got, g, cfg)
    check_table(got, g, cfg)
    check_floats(got, g, name)


@pytest.mark.parametrize("name", list(gg.CASES))
def test_host_path_takes_the_same_decisions(name, tmp_path):
    """The same run with `IA_OFFPOLICY_FUSED=0`, in a fresh process: the wrapper's per-step prediction and the ring's
    copies. Identical discrete records and ring contents; rewards to the fixture's tolerance."""
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    out = str(tmp_path / "host.npz")
    env = dict(os.environ, IA_OFFPOLICY_FUSED="0")
    subprocess.run([sys.executable, "-m", "tests.gail_offpolicy_golden", name, str(cfg["seed"]), out], check=True, cwd=ROOT,
                   env=env, timeout=300)
    host, fused = np.load(out), run(name)
    steps = len(g["ring_pos"])
    assert int(host["step_launches"]) == -1 and int(host["reward_fn_calls"]) == steps
    check_exact(host, g, cfg)
    check_table(host, g, cfg)
    for k in INDEX_KEYS + ROW_KEYS + ("table_obs", "table_next_obs", "table_action", "table_done"):
        if k in fused:
            assert np.array_equal(host[k], fused[k]), k
    assert rel(host["ring_reward"], fused["ring_reward"]) <= 8 * float(g["dref/ring_reward"])
    print(f"{name}: host-path and fused rewards bit-equal: {np.array_equal(host['ring_reward'], fused['ring_reward'])}")


def test_airl_refuses_a_deterministic_policy():
    cfg = dict(gg.COMMON, **gg.CASES["gail_dqn"])
    venv = gg.make_env(cfg, 0)
    obs, acts, nxt, dones = gg.make_demos(cfg, 0)
    rl = p.DQN("MlpPolicy", venv, device="cuda", **gg.rl_kwargs_of(cfg))
    net = p.BasicShapedRewardNet(venv.observation_space, venv.action_space)
    with pytest.raises(TypeError, match="AIRL needs a stochastic policy"):
        p.AIRL(demonstrations=p.Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones), demo_batch_size=16, venv=venv,
               gen_algo=rl, reward_net=net, custom_logger=p.configure_logger(None, []))


def test_checkpoint_save_says_that_offpolicy_generators_are_out_of_scope(tmp_path):
    cfg = dict(gg.COMMON, **gg.CASES["gail_dqn"])
    trainer, _ = gg.build(cfg, 0)
    with pytest.raises(NotImplementedError, match="off-policy generator"):
        p.checkpoint.save(trainer, str(tmp_path / "ckpt"))
    assert not os.path.exists(str(tmp_path / "ckpt"))
