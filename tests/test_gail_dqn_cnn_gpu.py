"""GAIL over a DQN `CnnPolicy` generator end to end on the device against the fixtures the reference's own GAIL produced over
the restated learner (`tests/golden/make_golden_gail_dqn_cnn.py`), on the frame path (csrc/offpolicy_frames.hip) and, in a
fresh process with `IA_OFFPOLICY_FUSED=0`, on the generic host path.

Exactly: every ring write position, raw done and time-limit flag, every branch, action and sampled index row, exploration
rates, target updates, the trainer's ring positions, actions and dones after every round, counters, the discriminator's
initial parameters, the learner's (as CRCs), the logger's dump steps and keys, and the CRCs of every frame: each learner-ring
write, the trainer's ring after every round, the demonstrations. The learner's ring is read back from device memory and
compared with what the writes rebuild, and the two paths' device rings, learner and generator, bit for bit with each
other. Floating values by relative L2 against the float64 run within `8 x dref`, dref = the larger deviation of the
reference's two float32 runs from its float64 run per key (printed with the measured deviation)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gail_dqn_cnn_golden as gg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX_KEYS = ("ring_pos", "ring_done", "ring_timeout", "branches", "sample_rows", "train_at", "gen_dones", "gen_idx",
              "gen_n_data", "n_dumps", "exploration_rate", "target_updates")
ROW_KEYS = ("ring_action", "actions", "gen_acts", "ring_obs_crc", "ring_next_obs_crc", "gen_obs_crc", "gen_next_obs_crc")
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
    for k in INDEX_KEYS + ROW_KEYS:
        assert np.array_equal(np.asarray(got[k]), g[k]), k
    warm = g["branches"] == gg.BRANCH["warmup"]
    assert warm.any() and not warm.all() and (g["branches"] == gg.BRANCH["greedy"]).sum() >= 10
    assert gg.demo_crc(cfg, cfg["seed"]) == int(g["demo_crc"])
    for k in g.files:
        if k.startswith("counter/"):
            assert int(got[k]) == int(g[k]), k
        if k.startswith("disc_init/"):
            assert np.array_equal(got[k], g[k]), k
        if k.startswith("init_crc/"):
            assert int(got[k]) == int(g[k]), k
    for j in range(int(g["n_dumps"])):
        assert int(got[f"dump{j}_step"]) == int(g[f"dump{j}_step"]), j
        assert [str(k) for k in got[f"dump{j}_keys"]] == [str(k) for k in g[f"dump{j}_keys"]], j


def check_table(got, g, cfg):
    """The learner's uint8 ring as it lies in DEVICE memory is what the writes leave behind: per write position the CRC of
    its obs rows and of its next_obs rows, the action column, `done * (1 - timeout)` in the done column and the reward the
    write's relabelling left."""
    n = cfg["n_envs"]
    assert got["table_obs"].dtype == np.uint8 and got["table_next_obs"].dtype == np.uint8
    last = {int(pos): i for i, pos in enumerate(g["ring_pos"])}     # the latest write of every position
    assert len(last) < len(g["ring_pos"])                            # the ring wrapped: rows were overwritten
    assert (g["ring_done"] * (1 - g["ring_timeout"]) != g["ring_done"]).any()
    for pos, i in last.items():
        sl = slice(pos * n, (pos + 1) * n)
        assert gg.crc(got["table_obs"][sl]) == int(g["ring_obs_crc"][i]), pos
        assert gg.crc(got["table_next_obs"][sl]) == int(g["ring_next_obs_crc"][i]), pos
        assert np.array_equal(got["table_action"][sl], g["ring_action"][i].reshape(-1)), pos
        assert np.array_equal(got["table_done"][sl], (g["ring_done"][i] * (1 - g["ring_timeout"][i])).astype(np.float32)), pos
        assert np.array_equal(got["table_reward"][sl].astype(np.float64), got["ring_reward"][i]), pos


def check_floats(got, g, name):
    worst = []
    for k in (f[len("dref/"):] for f in g.files if f.startswith("dref/")):
        dref, dev = float(g[f"dref/{k}"]), rel(got[k], g[f"f64/{k}"])
        print(f"{name} {k}: dref {dref:.3e}, device {dev:.3e}")
        if dev > (8 * dref if dref > 0 else EPS32):
            worst.append((k, dev, dref))
    first = gg.COMMON["gen_train_timesteps"] // gg.COMMON["n_envs"]
    print(f"{name} first round's ring_reward: dref {float(g['dref_first_round/ring_reward']):.3e}, device "
          f"{rel(got['ring_reward'][:first], g['f64/ring_reward'][:first]):.3e}")
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
def test_gail_over_a_dqn_cnn_generator_matches_the_reference_run(name):
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    got = run(name)
    steps = cfg["rounds"] * cfg["gen_train_timesteps"] // cfg["n_envs"]
    # the frame path: one step-store and one reward-store launch per environment step, no per-step reward prediction with
    # its read-back; one gather launch per discriminator minibatch
    assert len(g["ring_pos"]) == steps and int(got["frame_path"]) == 1
    assert int(got["step_launches"]) == steps and int(got["reward_launches"]) == steps
    assert int(got["reward_fn_calls"]) == 0
    assert int(got["gather_launches"]) == cfg["rounds"] * cfg["n_disc"]
    check_exact(got, g, cfg)
    check_table(got, g, cfg)
    check_floats(got, g, name)


def test_explicit_samples_take_the_frame_path():
    """`train_disc(expert_samples=..., gen_samples=...)`: the dicts are uploaded as uint8 tables and gathered by row
    number. The logits of the update equal the net's own `forward` on the preprocessed float frames (the same values
    through the same convolution ops: `forward` only adds the layout copy), taken before the optimiser step."""
    import torch as th

    cfg = dict(gg.COMMON, **gg.CASES["gail_dqn_cnn_next_done"])
    trainer, _ = gg.build(cfg, 0)
    assert trainer._frame_path
    B, n_act = cfg["demo_batch_size"], cfg["n_actions"]
    r = np.random.default_rng(3)
    batches = []
    for _ in range(2):
        batches.append(dict(obs=r.integers(0, 256, size=(B,) + tuple(cfg["frames"]), dtype=np.uint8),
                            next_obs=r.integers(0, 256, size=(B,) + tuple(cfg["frames"]), dtype=np.uint8),
                            acts=r.integers(0, n_act, size=B), dones=r.uniform(size=B) < 0.3))
    cat = {k: th.from_numpy(np.concatenate([b[k] for b in batches])).cuda() for k in batches[0]}
    with th.no_grad():
        want = trainer._reward_net(cat["obs"].float() / 255, th.nn.functional.one_hot(cat["acts"], n_act).float(),
                                   cat["next_obs"].float() / 255, cat["dones"].float()).cpu().numpy()
    stats = trainer.train_disc(expert_samples=batches[0], gen_samples=batches[1])
    got = trainer._last_disc_logits.cpu().numpy()
    print("explicit samples: max |logit difference|", float(np.abs(got - want).max()))
    assert np.array_equal(got, want)
    assert stats["n_expert"] == B and stats["n_generated"] == B and np.isfinite(stats["disc_loss"])
    assert trainer.frame_gather_launches == 1 and trainer._disc_step == 1
    with pytest.raises(ValueError, match="uint8"):
        trainer.train_disc(expert_samples=dict(batches[0], obs=batches[0]["obs"].astype(np.float32)), gen_samples=batches[1])


@pytest.mark.parametrize("name", list(gg.CASES))
def test_host_path_takes_the_same_decisions(name, tmp_path):
    """The same run with `IA_OFFPOLICY_FUSED=0`, in a fresh process: the wrapper's per-step prediction, the ring's copies,
    the float32 generator ring and discriminator tables. Identical discrete records and ring contents; floats to the
    fixture's tolerance."""
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    out = str(tmp_path / "host.npz")
    env = dict(os.environ, IA_OFFPOLICY_FUSED="0")
    subprocess.run([sys.executable, "-m", "tests.gail_dqn_cnn_golden", name, str(cfg["seed"]), out], check=True, cwd=ROOT,
                   env=env, timeout=300)
    host, fused = np.load(out), run(name)
    steps = len(g["ring_pos"])
    assert int(host["frame_path"]) == 0 and int(host["step_launches"]) == -1 and int(host["reward_fn_calls"]) == steps
    assert int(host["gather_launches"]) == 0
    check_exact(host, g, cfg)
    check_table(host, g, cfg)
    check_floats(host, g, name + " (host path)")
    # the two paths' device rings: the learner's table, and the trainer's generator ring after every round (CRCs of the
    # frames in the space's dtype, actions, dones, positions)
    for k in INDEX_KEYS + ROW_KEYS + ("table_obs", "table_next_obs", "table_action", "table_done"):
        assert np.array_equal(host[k], fused[k]), k
    print(f"{name}: host-path and fused rewards bit-equal: {np.array_equal(host['ring_reward'], fused['ring_reward'])}")
