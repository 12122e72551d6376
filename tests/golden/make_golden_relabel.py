"""Generates `tests/golden/relabel_buffer.npz` and `tests/golden/relabel_sac_two_phase.npz` with the REFERENCE's own
`imitation.policies.replay_buffer_wrapper.ReplayBufferRewardWrapper` and reward nets (imported unmodified under
`oracle.ref_shim` plus `tests.sac_ref.install_sb3_modules()`). Runs only where the reference sources are present.
Usage: `python tests/golden/make_golden_relabel.py [buffer] [two_phase]`.

The reward net is the scripts' `NormalizedRewardNet(BasicRewardNet(..., normalize_input_layer=RunningNorm), RunningNorm)`
with non-trivial frozen statistics, the reward function `functools.partial(net.predict_processed, update_stats=False)`.
Every run is made twice: in float32 through the reference's own `predict_processed`, and in float64, where the reward function
is the same modules converted to double and fed double inputs (the reference's `preprocess` always casts to float32). Floating
values stored are those of the float64 run (`f64/`); per float key `dref/` = the relative L2 deviation of the float32 run from
the float64 run (the device path is allowed 8 x).

`relabel_buffer.npz` (cases `box/`, `discrete/`; the adds are `tests.relabel_golden.buffer_adds`): the net's full state, the
NumPy seed, the sampled positions and env indices of three `sample(7)` calls and their rewards.

`relabel_sac_two_phase.npz`: the restated SAC of `tests/sac_ref.py` under the reference wrapper on `SyntheticVecEnv`;
`learn(K)`, then the reward net's state replaced by a second stored set, then `learn(K, reset_num_timesteps=False)`. A seed is
kept only if the float32 and the float64 run make the same index and `eps` draws, pick the same critics and leave both
generators in the same state, and if in phase 2 at least one sampled row was stored in phase 1 whose rewards under the two
parameter sets differ by more than 100 x that row's float32-to-float64 deviation (`n_rows_that_differ`). Stored: both net
states, per gradient step the sampled rows, `eps`, relabelled rewards, losses and alphas, and -- thinned as in
`td3_golden.thin` -- the initial parameters (float32, exact), the final parameters and Adam's moments.
"""
import copy
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim  # noqa: E402

from tests.relabel_golden import BUFFER, BUFFER_CASES, DIFFER_FACTOR, TWO_PHASE, buffer_adds, reward_net_kwargs  # noqa: E402
from tests.sac_golden import KEEP_MOMENT, make_env, rl_kwargs_of, rng_states, seed_everything, thin  # noqa: E402


def install():
    ref_shim.install()
    from tests import sac_ref
    sac_ref.install_sb3_modules()
    from oracle import sb3_restated as sb
    if not hasattr(sb.Logger, "warn"):
        sb.Logger.warn = lambda self, *args, **kwargs: None
    from imitation.policies import replay_buffer_wrapper as rbw
    from imitation.rewards import reward_nets
    from imitation.util import networks
    from stable_baselines3.common.buffers import ReplayBuffer
    return dict(rbw=rbw, rn=reward_nets, nets=networks, sb=sb, ref=sac_ref, ReplayBuffer=ReplayBuffer)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def make_net(m, obs_space, act_space, flags, seed):
    """The reference's normalised reward net with non-trivial statistics in both running norms."""
    import torch as th
    th.manual_seed(seed)
    base = m["rn"].BasicRewardNet(obs_space, act_space, normalize_input_layer=m["nets"].RunningNorm, **reward_net_kwargs(flags))
    net = m["rn"].NormalizedRewardNet(base, m["nets"].RunningNorm)
    with th.no_grad():
        D = base.mlp.normalize_input.running_mean.numel()
        base.mlp.normalize_input.update_stats(th.randn(50, D) * 1.5 + 0.5)
        net.normalize_output_layer.update_stats(th.randn(50, 1) * 0.4 + 0.2)
    return net.eval()


def state_of(net):
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


class Reward:
    """The reward function of one run, recording every call: float32 = the reference's own
    `partial(net.predict_processed, update_stats=False)`; float64 = the same modules in double on double inputs."""

    def __init__(self, net, act_space, double: bool):
        import torch as th
        self.th, self.net, self.double, self.log = th, net, double, []
        self.n_discrete = getattr(act_space, "n", None)
        self.fn32 = functools.partial(net.predict_processed, update_stats=False)
        self.net64 = copy.deepcopy(net).double().eval() if double else None

    def load(self, state) -> None:
        th = self.th
        self.net.load_state_dict({k: th.as_tensor(v) for k, v in state.items()})
        if self.double:
            self.net64 = copy.deepcopy(self.net).double().eval()

    def predict64(self, state, action, next_state, done, net64=None):
        th = self.th
        net64 = self.net64 if net64 is None else net64
        f = lambda x: th.as_tensor(np.asarray(x), dtype=th.float64)
        if self.n_discrete is not None:
            a = th.nn.functional.one_hot(th.as_tensor(np.asarray(action)).long().reshape(-1), self.n_discrete).double()
        else:
            a = f(action)
        with th.no_grad():
            raw = net64.base(f(state), a, f(next_state), f(done).reshape(-1))
            return net64.normalize_output_layer(raw).numpy().reshape(-1)

    def __call__(self, state, action, next_state, done):
        out = self.predict64(state, action, next_state, done) if self.double else self.fn32(state, action, next_state, done)
        self.log.append(np.asarray(out, np.float64).copy())
        return out


# ---------------------------------------------------------------------------------------------------------- the buffer alone

def buffer_run(m, discrete: bool, double: bool):
    import imitation_amd as p
    cfg = BUFFER
    obs_space = p.Box(-np.inf, np.inf, (cfg["obs_dim"],), np.float32)
    act_space = p.Discrete(cfg["n_discrete"]) if discrete else p.Box(-1.0, 1.0, (cfg["act_dim"],), np.float32)
    net = make_net(m, obs_space, act_space, cfg["flags"], 5 + int(discrete))
    fn = Reward(net, act_space, double)
    buf = m["rbw"].ReplayBufferRewardWrapper(cfg["buffer_size"], obs_space, act_space, replay_buffer_class=m["ReplayBuffer"],
                                            reward_fn=fn, n_envs=cfg["n_envs"], device="cpu")
    for obs, nxt, act, rew, done, infos in buffer_adds(discrete):
        buf.add(obs, nxt, act, rew, done, infos)
    positions = cfg["buffer_size"] // cfg["n_envs"]   # (the ring wraps: 40 adds into 32 positions)
    assert buf.pos == buf.replay_buffer.pos == cfg["n_adds"] - positions and buf.full and buf.replay_buffer.full
    np.random.seed(cfg["np_seed"])
    samples = [buf.sample(cfg["batch"]) for _ in range(cfg["n_samples"])]
    inner = buf.replay_buffer
    for s, (pos, env) in zip(samples, inner.sample_log):
        assert np.array_equal(s.observations.numpy(), inner.observations[pos, env])
        assert s.rewards.shape == (cfg["batch"], 1)
    return dict(state=state_of(net), pos=np.stack([x[0] for x in inner.sample_log]), env=np.stack([x[1] for x in inner.sample_log]),
                rewards=np.stack([s.rewards.numpy().reshape(-1).astype(np.float64) for s in samples]),
                env_rewards=inner.rewards.copy(), rng=rng_states())


def make_buffer():
    m = install()
    out = {"cfg": json.dumps(BUFFER)}
    for name in BUFFER_CASES:
        r32, r64 = buffer_run(m, name == "discrete", False), buffer_run(m, name == "discrete", True)
        assert np.array_equal(r32["pos"], r64["pos"]) and np.array_equal(r32["env"], r64["env"])
        for k, v in r32["state"].items():
            out[f"{name}/net/{k}"] = v
        out[f"{name}/sample_pos"], out[f"{name}/sample_env"] = r32["pos"], r32["env"]
        out[f"{name}/env_rewards"] = r32["env_rewards"]
        out[f"{name}/f64/rewards"] = r64["rewards"]
        out[f"{name}/dref/rewards"] = np.float64(rel_l2(r32["rewards"], r64["rewards"]))
        print(name, "dref", float(out[f"{name}/dref/rewards"]), "rows", (r32["pos"] * BUFFER["n_envs"] + r32["env"]).tolist())
    path = os.path.join(HERE, "relabel_buffer.npz")
    np.savez_compressed(path, **out)
    print("relabel_buffer.npz bytes", os.path.getsize(path))


# ------------------------------------------------------------------------------------------------------------- the learner

def two_phase_run(m, cfg, seed, double: bool):
    import torch as th
    ref, sb = m["ref"], m["sb"]
    venv = make_env(cfg, seed)
    net = make_net(m, venv.observation_space, venv.action_space, cfg["flags"], 1000 + seed)
    second = state_of(make_net(m, venv.observation_space, venv.action_space, cfg["flags"], 2000 + seed))
    first = state_of(net)
    fn = Reward(net, venv.action_space, double)
    seed_everything(venv, seed)
    ref.SAC.dtype = th.float64 if double else th.float32
    try:
        rl = ref.SAC("MlpPolicy", venv, replay_buffer_class=m["rbw"].ReplayBufferRewardWrapper,
                     replay_buffer_kwargs=dict(replay_buffer_class=m["ReplayBuffer"], reward_fn=fn),
                     **rl_kwargs_of(cfg, ref.NormalActionNoise))
    finally:
        ref.SAC.dtype = th.float32
    init = {k: v.detach().numpy().astype(np.float32) for k, v in rl.policy.state_dict().items()}
    rl.set_logger(sb.Logger(None, []))
    K = cfg["phase_timesteps"]
    rl.learn(K, log_interval=cfg["log_interval"])
    steps1 = len(rl.train_log)
    fn.load(second)
    rl.learn(K, reset_num_timesteps=False, log_interval=cfg["log_interval"])
    inner = rl.replay_buffer.replay_buffer
    rows = np.stack([pos.astype(np.int64) * cfg["n_envs"] + env for pos, env in inner.sample_log])
    assert len(rows) == len(fn.log) == len(rl.train_log) > steps1 > 0
    # phase-2 rows stored in phase 1: their reward under the first parameter set, in double
    first_fn = Reward(net, venv.action_space, True)
    first_fn.load(first)
    old = []
    for (pos, env) in inner.sample_log[steps1:]:
        d = (inner.dones[pos, env] * (1 - inner.timeouts[pos, env])).reshape(-1, 1)
        old.append(first_fn.predict64(inner.observations[pos, env], inner.actions[pos, env], inner.next_observations[pos, env], d))
    fn.load(second)   # (`first_fn.load` wrote the shared net)
    moments = {}
    for name, part in (("actor", rl.actor), ("critic", rl.critic)):
        st = part.optimizer.state
        for key in ("exp_avg", "exp_avg_sq"):
            moments[f"{name}.{key}"] = np.concatenate([st[q][key].detach().numpy().reshape(-1) for q in part.parameters()])
    final = {k: v.detach().numpy() for k, v in rl.policy.state_dict().items()}
    if rl.log_ent_coef is not None:
        st = rl.ent_coef_optimizer.state[rl.log_ent_coef]
        moments["ent_coef.exp_avg"], moments["ent_coef.exp_avg_sq"] = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        final["log_ent_coef"] = rl.log_ent_coef.detach().numpy()
    return dict(init=init, first=first, second=second, steps1=steps1, rows=rows, rewards=np.stack(fn.log),
                old_rewards=np.stack(old), phase1_rows=(K // cfg["n_envs"]) * cfg["n_envs"], train=rl.train_log, final=final,
                moments=moments, rng=rng_states(), adds=inner.add_log, env_rewards=inner.rewards[:inner.pos].copy(),
                counters=dict(num_timesteps=rl.num_timesteps, n_updates=rl._n_updates, pos=inner.pos))


def rows_that_differ(r32, r64):
    """Phase-2 sampled rows stored in phase 1 whose rewards under the two parameter sets differ by more than
    DIFFER_FACTOR x the row's float32-to-float64 deviation."""
    s1 = r64["steps1"]
    rows, new64, new32, old64 = r64["rows"][s1:], r64["rewards"][s1:], r32["rewards"][s1:], r64["old_rewards"]
    from_phase1 = rows < r64["phase1_rows"]
    return int((from_phase1 & (np.abs(new64 - old64) > DIFFER_FACTOR * np.abs(new32 - new64))).sum()), int(from_phase1.sum())


def check(r32, r64):
    if r32["steps1"] != r64["steps1"] or len(r32["train"]) != len(r64["train"]):
        return "the runs make different numbers of gradient steps"
    if not np.array_equal(r32["rows"], r64["rows"]):
        return "the sampled rows differ"
    for s, t in zip(r32["train"], r64["train"]):
        if not np.array_equal(s["eps"], t["eps"]):
            return "eps differs"
        if not (np.array_equal(s["argmin_target"], t["argmin_target"]) and np.array_equal(s["argmin_pi"], t["argmin_pi"])):
            return "the runs pick different critics"
    if not all(np.array_equal(r32["rng"][k], r64["rng"][k]) for k in r32["rng"]):
        return "generator post-states differ"
    if [a[0] for a in r32["adds"]] != [a[0] for a in r64["adds"]]:
        return "ring positions differ"
    n, _ = rows_that_differ(r32, r64)
    if n < 1:
        return "no phase-2 row from phase 1 tells the two parameter sets apart"
    return None


def floats_of(r):
    fl = dict(rewards=r["rewards"], critic_loss=np.array([t["critic_loss"] for t in r["train"]]),
              actor_loss=np.array([t["actor_loss"] for t in r["train"]]), ent_coef=np.array([t["ent_coef"] for t in r["train"]]),
              ent_coef_loss=np.array([t["ent_coef_loss"] for t in r["train"]]))
    for k, v in r["final"].items():
        fl[f"final/{k}"] = thin(v)
    for k, v in r["moments"].items():
        fl[f"moment/{k}"] = thin(v, KEEP_MOMENT)
    return {k: np.asarray(v, np.float64) for k, v in fl.items()}


def make_two_phase():
    m = install()
    cfg = dict(TWO_PHASE)
    for seed in range(200):
        r32, r64 = two_phase_run(m, cfg, seed, False), two_phase_run(m, cfg, seed, True)
        why = check(r32, r64)
        if why is None:
            break
        print(f"two_phase: seed {seed} rejected: {why}")
    else:
        raise SystemExit("two_phase: no seed satisfies the conditions")
    out = {"cfg": json.dumps(dict(cfg, seed=seed))}
    for which in ("first", "second"):
        for k, v in r32[which].items():
            out[f"net_{which}/{k}"] = v
    for k, v in r32["init"].items():
        out[f"init/{k}"] = thin(v)
    n_differ, n_phase1 = rows_that_differ(r32, r64)
    out.update(steps_phase1=np.int64(r32["steps1"]), phase1_rows=np.int64(r32["phase1_rows"]), sample_rows=r32["rows"],
               eps=np.stack([t["eps"] for t in r32["train"]]), n_rows_that_differ=np.int64(n_differ),
               n_phase2_rows_from_phase1=np.int64(n_phase1), old_rewards64=r64["old_rewards"],
               argmin=np.stack([np.stack([t["argmin_target"], t["argmin_pi"]]) for t in r32["train"]]),
               env_rewards=r32["env_rewards"], **r32["rng"])
    for k, v in r32["counters"].items():
        out[f"counter/{k}"] = np.int64(v)
    f32, f64 = floats_of(r32), floats_of(r64)
    for k in f64:
        out[f"f64/{k}"] = f64[k]
        out[f"dref/{k}"] = np.float64(rel_l2(f32[k], f64[k]))
    path = os.path.join(HERE, "relabel_sac_two_phase.npz")
    np.savez_compressed(path, **out)
    print("two_phase seed", seed, "steps", len(r32["train"]), "of them phase 1", r32["steps1"], "rows that differ", n_differ,
          "of", n_phase1, "dref", {k[5:]: float(f"{float(v):.2e}") for k, v in out.items() if k.startswith("dref/")},
          "bytes", os.path.getsize(path))


if __name__ == "__main__":
    which = sys.argv[1:] or ["buffer", "two_phase"]
    if "buffer" in which:
        make_buffer()
    if "two_phase" in which:
        make_two_phase()
