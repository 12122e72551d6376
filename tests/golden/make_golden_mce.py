"""Generates `tests/golden/mce_*.npz` by running the REFERENCE's own `imitation.algorithms.mce_irl` (imported unmodified
under `oracle.ref_shim`) on small seeded tabular MDPs. Runs only where the reference sources are present.
Usage: `python tests/golden/make_golden_mce.py [CASE ...]` (no name: every case).

The module imports `seals.base_envs` (for annotations) and `stable_baselines3.common.type_aliases`, neither of which the
shim has: this script adds stubs of both in its own process. Nothing of the reference is imported at module level, so
tests import `CASES`, `make_mdp` and `sample_trajectories` from here.

Each file holds the MDP arrays, the net's initial `state_dict`, `demo_state_om`, the logger's records at every dump, the
iteration count, the final `state_dict`, Adam state, visitations and policy, and the tables of `mce_partition_fh` /
`mce_occupancy_measures` on the true reward. The script asserts that no stopping decision of the recorded run is within
a factor 1.25 of its threshold, so float32 rounding cannot move the iteration count, and that the reference's own run,
restarted one float32 ulp away from the recorded initial parameters, ends within 1e-4 of the recorded final parameters, so
a comparison of final parameters is a comparison of the algorithm and not of one ReLU unit's switching time.
"""
import os
import sys
import types as _types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = {
    # demo: "om" = the occupancy measure of the true linear reward; "trajs" = trajectories sampled from its policy
    "mce_linear": dict(S=24, A=3, H=8, obs_dim=6, hid=[], demo="om", discount=1.0, max_iter=60, lr=1e-2, linf_eps=1e-3,
                       grad_l2_eps=1e-4, early=False, seed=0),
    # (seeds 1, 3, 4, 5, 6 and 8 fail the conditioning check of run_case by percents; 7 passes)
    "mce_mlp_discount": dict(S=37, A=4, H=11, obs_dim=5, hid=[32, 32], demo="trajs", n_traj=20, discount=0.9,
                             max_iter=40, lr=1e-2, linf_eps=1e-3, grad_l2_eps=1e-4, early=False, seed=7),
    # a large step and a loose linf_eps: linf_delta falls 0.029, 0.018, 0.006 and the reference stops at the fifth iteration
    "mce_early_stop": dict(S=12, A=2, H=5, obs_dim=3, hid=[], demo="om", discount=1.0, max_iter=200, lr=0.2,
                           linf_eps=0.012, grad_l2_eps=1e-4, early=True, seed=2),
}
MARGIN_BELOW, MARGIN_ABOVE = 0.8, 1.25
# The output layer's bias has an exactly zero true gradient (the occupancy vectors both sum to H + 1): Adam turns the
# rounding residue of its float32 gradient into steps of up to lr, so its value depends on summation order. It is left
# out of the conditioning check below and compared on its own by the tests.
FINAL_BIAS = "mlp.dense_final.bias"
CONDITION_TRIALS, CONDITION_RTOL = 6, 1e-4


class Env:
    """The attributes of a tabular model that `mce_irl` reads."""

    def __init__(self, mdp):
        from imitation_amd import spaces as sp
        self.transition_matrix = mdp["transition_matrix"]
        self.observation_matrix = mdp["observation_matrix"]
        self.reward_matrix = mdp["reward_matrix"]
        self.initial_state_dist = mdp["initial_state_dist"]
        self.horizon = int(mdp["horizon"])
        self.state_dim, self.action_dim = self.transition_matrix.shape[:2]
        self.obs_dim = self.observation_matrix.shape[1]
        self.state_space, self.action_space = sp.Discrete(self.state_dim), sp.Discrete(self.action_dim)
        self.observation_space = sp.Box(-np.inf, np.inf, (self.obs_dim,), np.float32)


def make_mdp(cfg):
    """A seeded random MDP: row-stochastic transitions with about a third of the entries exactly zero, a random
    observation matrix, an initial distribution with zero entries, and a linear true reward (float32 values, the dtype a
    reward net predicts)."""
    r = np.random.default_rng(7000 + cfg["seed"])
    S, A = cfg["S"], cfg["A"]
    T = r.uniform(0.05, 1.0, size=(S, A, S))
    T[r.uniform(size=T.shape) < 1.0 / 3.0] = 0.0
    T[np.arange(S)[:, None], np.arange(A)[None, :], r.integers(S, size=(S, A))] += 0.5   # no empty row
    T /= T.sum(axis=2, keepdims=True)
    obs = r.normal(size=(S, cfg["obs_dim"])).astype(np.float32)
    init = r.uniform(0.1, 1.0, size=S)
    init[r.uniform(size=S) < 0.4] = 0.0
    init[int(r.integers(S))] += 0.5
    init /= init.sum()
    theta = r.normal(size=cfg["obs_dim"]).astype(np.float32)
    reward = (obs @ theta).astype(np.float32)
    return {"transition_matrix": T, "observation_matrix": obs, "initial_state_dist": init, "true_theta": theta,
            "reward_matrix": reward.astype(np.float64), "horizon": np.int64(cfg["H"])}


def sample_trajectories(mdp, pi, n_traj, seed):
    """`n_traj` state / action sequences of one horizon each under the time-dependent policy `pi[t, s, a]`."""
    r = np.random.default_rng(9000 + seed)
    T, init, H = mdp["transition_matrix"], mdp["initial_state_dist"], int(mdp["horizon"])
    S, A = T.shape[:2]
    states, acts = np.zeros((n_traj, H + 1), np.int64), np.zeros((n_traj, H), np.int64)
    for k in range(n_traj):
        s = r.choice(S, p=init)
        for t in range(H):
            states[k, t] = s
            acts[k, t] = a = r.choice(A, p=pi[t, s] / pi[t, s].sum())
            s = r.choice(S, p=T[s, a])
        states[k, H] = s
    return states, acts


def install():
    from oracle import ref_shim
    ref_shim.install()
    ta = _types.ModuleType("stable_baselines3.common.type_aliases")
    ta.Schedule = ta.PyTorchObs = object
    sys.modules["stable_baselines3.common.type_aliases"] = ta
    sys.modules["stable_baselines3.common"].type_aliases = ta
    seals = _types.ModuleType("seals")
    base_envs = _types.ModuleType("seals.base_envs")
    base_envs.TabularModelPOMDP = type("TabularModelPOMDP", (), {})
    seals.base_envs = base_envs
    sys.modules["seals"], sys.modules["seals.base_envs"] = seals, base_envs
    from imitation.algorithms import mce_irl
    from imitation.data import types
    from imitation.rewards import reward_nets
    from imitation.util import logger as imit_logger
    return mce_irl, types, reward_nets, imit_logger


def check_margins(name, cfg, dumps, n_iters):
    """The stopping iteration is unambiguous: see the module docstring."""
    linf = np.array([d["linf_delta"] for d in dumps])
    grad = np.array([d["grad_norm"] for d in dumps])
    assert len(dumps) == n_iters, (name, len(dumps), n_iters)
    assert (grad >= MARGIN_ABOVE * cfg["grad_l2_eps"]).all(), (name, "grad_norm too close to grad_l2_eps", grad.min())
    if cfg["early"]:
        assert n_iters < cfg["max_iter"], (name, "ran to max_iter")
        assert linf[-1] <= MARGIN_BELOW * cfg["linf_eps"], (name, "stopping linf_delta too close", linf[-1])
        assert (linf[:-1] >= MARGIN_ABOVE * cfg["linf_eps"]).all(), (name, "earlier linf_delta too close", linf[:-1].min())
    else:
        assert n_iters == cfg["max_iter"], (name, "stopped early", n_iters)
        assert (linf >= MARGIN_ABOVE * cfg["linf_eps"]).all(), (name, "linf_delta too close to linf_eps", linf.min())


def run_case(name, cfg, mce_irl, types, reward_nets, imit_logger, tmp):
    import torch as th

    mdp = make_mdp(cfg)
    env = Env(mdp)
    true_r = mdp["reward_matrix"].astype(np.float32)
    out = dict(mdp)
    V, Q, pi = mce_irl.mce_partition_fh(env, reward=true_r, discount=cfg["discount"])
    D, Dcum = mce_irl.mce_occupancy_measures(env, reward=true_r, discount=cfg["discount"])
    out.update({"true_V": V, "true_Q": Q, "true_pi": pi, "true_D": D, "true_Dcum": Dcum})
    # the same with a given policy (the discounted one; the default policy above is planned undiscounted)
    D2, Dcum2 = mce_irl.mce_occupancy_measures(env, reward=true_r, pi=pi, discount=cfg["discount"])
    out.update({"true_D_of_pi": D2, "true_Dcum_of_pi": Dcum2})

    def make_net():
        return reward_nets.BasicRewardNet(env.observation_space, env.action_space, use_action=False, hid_sizes=cfg["hid"])

    if cfg["demo"] == "om":
        demos = Dcum
    else:
        states, acts = sample_trajectories(mdp, pi, cfg["n_traj"], cfg["seed"])
        out["traj_states"], out["traj_acts"] = states, acts
        demos = [types.Trajectory(obs=s, acts=a, infos=None, terminal=True) for s, a in zip(states, acts)]
        # the timeless input forms of the same data (discount 1 only): Transitions, transitions without next_obs, mappings
        trans = types.Transitions(obs=states[:, :-1].reshape(-1), acts=acts.reshape(-1), next_obs=states[:, 1:].reshape(-1),
                                  dones=np.tile(np.arange(cfg["H"]) == cfg["H"] - 1, len(states)),
                                  infos=np.array([{}] * acts.size))
        minimal = types.TransitionsMinimal(obs=trans.obs, acts=trans.acts, infos=trans.infos)
        batches = [{"obs": trans.obs[i:i + 50], "acts": trans.acts[i:i + 50], "next_obs": trans.next_obs[i:i + 50],
                    "dones": trans.dones[i:i + 50]} for i in range(0, len(trans.obs), 50)]
        import warnings
        for key, form in (("transitions", trans), ("minimal", minimal), ("mappings", batches),
                          ("trajectories_undiscounted", demos)):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                algo = mce_irl.MCEIRL(form, env, make_net(), np.random.default_rng(0), discount=1.0)
            out[f"form_om/{key}"] = algo.demo_state_om.copy()

    th.manual_seed(cfg["seed"])
    net = make_net()
    for k, v in net.state_dict().items():
        out[f"init/{k}"] = v.detach().numpy().copy()
    logger = imit_logger.configure(os.path.join(tmp, name), ["log"])
    dumps, steps = [], []
    orig_dump = logger.dump

    def dump(step=0):
        dumps.append({k: float(v) for k, v in logger.default_logger.name_to_value.items()})
        steps.append(int(step))
        orig_dump(step)

    logger.dump = dump
    algo = mce_irl.MCEIRL(demos, env, net, np.random.default_rng(cfg["seed"]), optimizer_kwargs={"lr": cfg["lr"]},
                          discount=cfg["discount"], linf_eps=cfg["linf_eps"], grad_l2_eps=cfg["grad_l2_eps"],
                          log_interval=1, custom_logger=logger)
    out["demo_state_om"] = np.asarray(algo.demo_state_om, np.float64).copy()
    visitations = algo.train(max_iter=cfg["max_iter"])
    n_iters = len(dumps)
    check_margins(name, cfg, dumps, n_iters)

    # the run is well conditioned: the reference itself, started one float32 ulp away (random signs on every initial
    # parameter), must end within CONDITION_RTOL of the recorded parameters. A ReLU unit that switches on a state within
    # rounding of an iteration boundary fails this (final parameters then move by percents): change the seed.
    flat = lambda sd: np.concatenate([v.detach().numpy().reshape(-1) for k, v in sd.items() if k != FINAL_BIAS])
    base = flat(net.state_dict())
    for trial in range(CONDITION_TRIALS):
        r = np.random.default_rng(trial)
        net2 = make_net()
        net2.load_state_dict({k: th.as_tensor(out[f"init/{k}"] * (1 + 2.0 ** -23 * r.choice([-1.0, 1.0], size=out[f"init/{k}"].shape))
                                              ).float() for k in net.state_dict()})
        quiet = imit_logger.configure(os.path.join(tmp, f"{name}_c{trial}"), ["log"])
        mce_irl.MCEIRL(demos, env, net2, np.random.default_rng(cfg["seed"]), optimizer_kwargs={"lr": cfg["lr"]},
                       discount=cfg["discount"], linf_eps=cfg["linf_eps"], grad_l2_eps=cfg["grad_l2_eps"],
                       log_interval=None, custom_logger=quiet).train(max_iter=cfg["max_iter"])
        moved = float(np.max(np.abs(flat(net2.state_dict()) - base)) / np.max(np.abs(base)))
        assert moved <= CONDITION_RTOL, (name, "ill-conditioned run: change the seed", trial, moved)

    keys = sorted(dumps[0])
    assert all(sorted(d) == keys for d in dumps)
    out["log_keys"] = np.array(keys)
    out["log_vals"] = np.array([[d[k] for k in keys] for d in dumps], np.float64)
    out["dump_steps"] = np.array(steps, np.int64)
    out["n_iters"] = np.int64(n_iters)
    for k, v in net.state_dict().items():
        out[f"final/{k}"] = v.detach().numpy().copy()
    ps = list(algo.optimizer.param_groups[0]["params"])
    st = algo.optimizer.state
    out["adam/step"] = np.int64(int(st[ps[0]]["step"]))
    out["adam/exp_avg"] = np.concatenate([st[p]["exp_avg"].reshape(-1).numpy() for p in ps])
    out["adam/exp_avg_sq"] = np.concatenate([st[p]["exp_avg_sq"].reshape(-1).numpy() for p in ps])
    out["visitations"] = np.asarray(visitations, np.float64)
    out["final_pi"] = algo.policy.pi.copy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "iterations", n_iters, "linf first/last", out["log_vals"][0, keys.index("linf_delta")],
          out["log_vals"][-1, keys.index("linf_delta")], "bytes", os.path.getsize(path))


def main():
    import tempfile
    names = sys.argv[1:] or list(CASES)
    unknown = [n for n in names if n not in CASES]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {list(CASES)}")
    mods = install()
    tmp = tempfile.mkdtemp()
    for name in names:
        run_case(name, CASES[name], *mods, tmp)


if __name__ == "__main__":
    main()
