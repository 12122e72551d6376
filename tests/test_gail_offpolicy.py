"""GAIL with off-policy generators, host logic (no GPU): `OffPolicyAlgorithm.set_env`, the deferred episode bookkeeping of
`RewardVecEnvWrapper`, and the shape of the fixtures `tests/golden/make_golden_gail_offpolicy.py` writes."""
import json
import os

import numpy as np
import pytest

import imitation_amd as p
from oracle import ref_shim
from tests import gail_offpolicy_golden as gg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def _env(n=4, od=4, n_discrete=2, act_dim=2):
    return p.SyntheticVecEnv(num_envs=n, obs_dim=od, act_dim=act_dim, horizon=8, seed=0, n_discrete=n_discrete,
                             prefetch_noise=False)


@pytest.mark.parametrize("algo", ["DQN", "TD3", "DDPG"])
def test_set_env_checks_spaces_and_envs_and_forces_a_reset(algo):
    nd = 2 if algo == "DQN" else None
    venv = _env(n_discrete=nd)
    rl = getattr(p, algo)("MlpPolicy", venv, buffer_size=64, policy_kwargs=dict(net_arch=[32, 32]), device="cpu")
    rl._last_obs = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError, match="Observation spaces do not match"):
        rl.set_env(_env(od=5, n_discrete=nd))
    with pytest.raises(ValueError, match="Action spaces do not match"):
        rl.set_env(_env(n_discrete=3) if nd else _env(act_dim=3, n_discrete=None))
    with pytest.raises(ValueError, match=r"number of environments to be set is different .*\(2 != 4\)"):
        rl.set_env(_env(n=2, n_discrete=nd))
    assert rl.get_env() is venv and rl._last_obs is not None   # a refused environment changes nothing
    other = p.RewardVecEnvWrapper(p.BufferingWrapper(_env(n_discrete=nd)), reward_fn=lambda s, a, ns, d: np.zeros(len(s)))
    rl.set_env(other, force_reset=False)
    assert rl.get_env() is other and rl.n_envs == 4 and rl._last_obs is not None
    rl.set_env(venv)
    assert rl.get_env() is venv and rl._last_obs is None   # the next `_setup_learn` resets the environment


def test_record_rewards_on_a_tile_equals_the_per_step_calls_bit_for_bit():
    """`flush_rewards` hands `record_rewards` the `[steps, n]` rows of the pinned reward tile: the same additions in the
    same order as one call per step, episode ends included."""
    T, n = 13, 5
    r = np.random.default_rng(3)
    rews = r.normal(size=(T, n)).astype(np.float32)
    dones = r.uniform(size=(T, n)) < 0.3
    dones[4] = False
    dones[7] = True
    obs = r.normal(size=(T, n, 3)).astype(np.float32)
    zero = lambda s, a, ns, d: np.zeros(len(s))
    make = lambda: p.RewardVecEnvWrapper(p.BufferingWrapper(_env(n=n, od=3)), reward_fn=zero, ep_history=7)
    tiled, stepped = make(), make()
    tiled.record_rewards(rews[:6], dones[:6], obs[5])
    tiled.record_rewards(rews[6:], dones[6:], obs[-1])
    for t in range(T):
        stepped.record_rewards(rews[t][None], dones[t][None], obs[t])
    assert len(stepped.episode_rewards) == 7 and dones.sum() > 7   # the deque wrapped
    assert [float(x).hex() for x in tiled.episode_rewards] == [float(x).hex() for x in stepped.episode_rewards]
    assert tiled._cumulative_rew.tobytes() == stepped._cumulative_rew.tobytes()
    assert np.array_equal(tiled._old_obs, stepped._old_obs)
    # without a step source there is nothing deferred: the flush is a no-op
    tiled.flush_rewards(force=True)
    assert tiled._cumulative_rew.tobytes() == stepped._cumulative_rew.tobytes()


@pytest.mark.parametrize("name", list(gg.CASES))
def test_fixtures_carry_both_runs_and_a_dref_for_every_float_key(name):
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    assert cfg["case"] == name and {k: cfg[k] for k in gg.COMMON if k not in gg.CASES[name]} == \
        {k: v for k, v in gg.COMMON.items() if k not in gg.CASES[name]}
    assert (cfg["n_envs"], cfg["horizon"], cfg["rounds"], cfg["gen_train_timesteps"]) == (4, 8, 3, 32)
    assert (cfg["demo_batch_size"], cfg["n_disc"], cfg["learning_starts"], cfg["train_freq"]) == (16, 2, 20, 4)
    f64 = {k[4:] for k in g.files if k.startswith("f64/")}
    assert f64 and f64 == {k[4:] for k in g.files if k.startswith("f32/")} == {k[5:] for k in g.files if k.startswith("dref/")}
    assert {"ring_reward", "loss", "disc_final/mlp.dense0.weight", "disc_final/mlp.dense_final", "disc_norm/running_mean",
            "disc_norm/running_var"} <= f64 and any(k.startswith("final/") for k in f64)
    assert g["f64/disc_final/mlp.dense_final"].size == 33 and int(g["disc_norm_count"]) > 0
    assert all(g[f"f64/{k}"].size > 1 for k in f64 if k.startswith(("final/", "disc_final/")))
    for k in f64:
        assert g[f"f64/{k}"].dtype == np.float64 and g[f"f32/{k}"].shape == g[f"f64/{k}"].shape, k
        assert 0.0 <= float(g[f"dref/{k}"]) < 1e-5, k
    assert len(g["log_keys"]) == len(g["log_dref"]) > 0 and not any("time/" in str(k) for k in g["log_keys"])
    for j in range(int(g["n_dumps"])):
        assert len(g[f"dump{j}_keys"]) == len(g[f"dump{j}_vals"]) == len(g[f"dump{j}_vals64"])
    sqil = [os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
            if f.startswith("sqil_") and f.endswith(".npz")]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= max(sqil)
    steps = cfg["rounds"] * cfg["gen_train_timesteps"] // cfg["n_envs"]
    assert len(g["ring_pos"]) == len(g["branches"]) == steps and g["f64/ring_reward"].shape == (steps, cfg["n_envs"])
    if cfg["algo"] == "DQN":
        assert (g["branches"] == gg.BRANCH["greedy"]).sum() >= 10 and "ring_obs" in g.files
    else:
        assert "ring_obs" in f64


@pytest.mark.reference
def test_the_generator_reproduces_gail_dqn_from_its_seed():
    if not ref_shim.reference_available():
        pytest.skip("reference sources not present")
    import torch as th

    from tests.golden import make_golden_gail_offpolicy as mk

    g = golden("gail_dqn")
    cfg = json.loads(str(g["cfg"]))
    seed = cfg.pop("seed")
    for k in ("gap_margin", "case"):
        cfg.pop(k)
    m = mk.install()
    r32, r64 = mk.run_once(cfg, seed, m, th.float32), mk.run_once(cfg, seed, m, th.float64)
    assert mk.check(cfg, r32, r64) is None
    out = mk.pack("gail_dqn", cfg, seed, r32, r64)
    assert set(out) == set(g.files)
    for k in g.files:
        if k == "cfg" or "time/" in k:
            continue
        a, b = np.asarray(out[k]), g[k]
        if k.startswith("dump") and k.endswith(("_vals", "_vals64")):   # (wall-clock entries aside)
            keep = np.array(["time/" not in str(x) for x in g[k.split("_vals")[0] + "_keys"]])
            a, b = a[keep], b[keep]
        assert np.array_equal(a, b), k
