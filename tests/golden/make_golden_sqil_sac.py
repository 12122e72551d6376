"""Generates `tests/golden/sqil_sac_*.npz` by running the REFERENCE's own SQIL (`imitation.algorithms.sqil`, imported
unmodified under `oracle.ref_shim`) with `rl_algo_class` = the restated SAC of `tests/sac_ref.py` on this package's
`SyntheticVecEnv` with Box actions. Runs only where the reference sources are present.
Usage: `python tests/golden/make_golden_sqil_sac.py [case ...]`.

Every case runs twice from the same seeds, in float32 and in float64, and a seed is kept only if, in BOTH runs,

* training starts before the run ends;
* at least one `done = 1` row is sampled;
* each critic attains the target's minimum on some row, and each attains the actor's minimum on some row;
* with `target_update_interval=2`, some steps update the target and some do not;
* a learned alpha ends away from its initial value (by more than 1e-3);

and the two runs pick the same critic on every row of every step, make the same index and `eps` draws, leave both generators
in the same state, and the smallest |Q1 - Q2| over all rows of both minima of all steps is at least 100 x the largest
float32-to-float64 deviation of those Q-values (a near tie flips the gradient's route, and no tolerance holds then). The gap and
the deviation are stored in the fixture (`min_q_gap`, `q_dev`), as is the kept seed (`cfg`).

Each file holds the settings, the demonstrations, every ring write, every sampled index, the `eps` tensors of the gradient
steps and of the environment steps, the argmin records, every action with its branch, the logger dumps, the per-step losses
and alphas, both generators' post-states, the counters and -- thinned as in `td3_golden.thin` -- the initial parameters
(float32, exact), the final parameters and Adam's moments. Floating values are those of the float64 run (`f64/`); per float
key `dref/` = the relative L2 deviation of the float32 run from the float64 run (the device path is allowed 8 x).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim  # noqa: E402

from tests.sac_golden import (BRANCH, CASES, COMMON, KEEP_MOMENT, make_demos, make_env, rl_kwargs_of, rng_states,  # noqa: E402
                               seed_everything, thin)

ALPHA_MOVE, GAP_FACTOR = 1e-3, 100.0


def install():
    ref_shim.install()
    from tests import sac_ref
    sac_ref.install_sb3_modules()
    from oracle import sb3_restated as sb
    if not hasattr(sb.Logger, "warn"):
        sb.Logger.warn = lambda self, *args, **kwargs: None
    from imitation.algorithms import sqil
    from imitation.data import types
    return dict(sqil=sqil, types=types, sb=sb, ref=sac_ref)


def run_once(cfg, seed, m, dtype):
    import torch as th
    ref, sb = m["ref"], m["sb"]
    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = m["types"].Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones, infos=np.array([{}] * len(obs)))
    seed_everything(venv, seed)
    ref.SAC.dtype = dtype
    try:
        algo = m["sqil"].SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy", rl_algo_class=ref.SAC,
                              rl_kwargs=rl_kwargs_of(cfg, ref.NormalActionNoise))
    finally:
        ref.SAC.dtype = th.float32
    rl = algo.rl_algo
    init = {k: v.detach().numpy().astype(np.float32) for k, v in rl.policy.state_dict().items()}
    logger = sb.Logger(None, [])
    rl.set_logger(logger)
    dumps = []
    orig_dump = logger.dump

    def dump(step=0):
        dumps.append((int(step), {k: float(v) for k, v in logger.name_to_value.items()}))
        orig_dump(step)

    logger.dump = dump
    algo.train(total_timesteps=cfg["total_timesteps"], log_interval=cfg["log_interval"])
    rb = rl.replay_buffer
    moments = {}
    for name, net in (("actor", rl.actor), ("critic", rl.critic)):
        st = net.optimizer.state
        for key in ("exp_avg", "exp_avg_sq"):
            moments[f"{name}.{key}"] = np.concatenate([st[p][key].detach().numpy().reshape(-1) for p in net.parameters()])
    final = {k: v.detach().numpy() for k, v in rl.policy.state_dict().items()}
    if rl.log_ent_coef is not None:
        st = rl.ent_coef_optimizer.state[rl.log_ent_coef]
        moments["ent_coef.exp_avg"], moments["ent_coef.exp_avg_sq"] = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        final["log_ent_coef"] = rl.log_ent_coef.detach().numpy()
    return dict(init=init, dumps=dumps, adds=rb.add_log, new_samples=rb.sample_log,
                expert_samples=rb.expert_buffer.sample_log, actions=rl.action_log, act_eps=rl.act_eps_log, train=rl.train_log,
                final=final, moments=moments, rng=rng_states(), learned=rl.log_ent_coef is not None,
                counters=dict(num_timesteps=rl.num_timesteps, n_updates=rl._n_updates, episodes=rl._episode_num, pos=rb.pos,
                              full=bool(rb.full)))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def q_gap(r32, r64):
    """(smallest |Q1 - Q2| of the float64 run, largest float32-to-float64 deviation of those Q-values) over both minima."""
    gap, dev = np.inf, 0.0
    for s, t in zip(r32["train"], r64["train"]):
        for k in ("q_target", "q_pi"):
            gap = min(gap, float(np.abs(t[k][:, 0] - t[k][:, 1]).min()))
            dev = max(dev, float(np.abs(s[k] - t[k]).max()))
    return gap, dev


def check(cfg, r32, r64):
    """None if the pair of runs satisfies the conditions in the module docstring, else the reason."""
    for r in (r32, r64):
        if not r["train"]:
            return "training never starts"
        if not any((t["dones"] == 1).any() for t in r["train"]):
            return "no done row is sampled"
        for k in ("argmin_target", "argmin_pi"):
            am = np.concatenate([t[k] for t in r["train"]])
            if not ((am == 0).any() and (am == 1).any()):
                return f"{k}: not every critic attains the minimum somewhere"
        updated = [t["target_updated"] for t in r["train"]]
        if cfg["target_update_interval"] == 2 and (all(updated) or not any(updated)):
            return "target updates and skipped target updates do not both occur"
        if r["learned"] and abs(r["train"][-1]["ent_coef"] - r["train"][0]["ent_coef"]) <= ALPHA_MOVE:
            return "alpha stays at its initial value"
    if len(r32["train"]) != len(r64["train"]):
        return "the runs make different numbers of gradient steps"
    if len(r32["actions"]) != len(r64["actions"]) or [a[0] for a in r32["actions"]] != [a[0] for a in r64["actions"]]:
        return "the runs take different branches"
    for k in ("new_samples", "expert_samples"):
        for x, y in zip(r32[k], r64[k]):
            if not all(np.array_equal(p, q) for p, q in zip(x, y)):
                return f"{k} differ between the runs"
    if [a[0] for a in r32["adds"]] != [a[0] for a in r64["adds"]]:
        return "ring positions differ"
    for s, t in zip(r32["train"], r64["train"]):
        if not np.array_equal(s["eps"], t["eps"]):
            return "eps differs"
        if not (np.array_equal(s["argmin_target"], t["argmin_target"]) and np.array_equal(s["argmin_pi"], t["argmin_pi"])):
            return "the runs pick different critics"
    if not all(np.array_equal(a, b) for a, b in zip(r32["act_eps"], r64["act_eps"])):
        return "the environment steps' eps differs"
    if not all(np.array_equal(r32["rng"][k], r64["rng"][k]) for k in r32["rng"]):
        return "generator post-states differ"
    gap, dev = q_gap(r32, r64)
    if gap < GAP_FACTOR * dev:
        return f"smallest |Q1 - Q2| {gap:.3e} is below {GAP_FACTOR:.0f} x the Q deviation {dev:.3e}"
    return None


def floats_of(r):
    fl = dict(ring_obs=np.stack([a[1] for a in r["adds"]]), ring_next_obs=np.stack([a[2] for a in r["adds"]]),
              ring_action=np.stack([a[3] for a in r["adds"]]), actions=np.stack([a[1] for a in r["actions"]]),
              buffer_actions=np.stack([a[2] for a in r["actions"]]),
              critic_loss=np.array([t["critic_loss"] for t in r["train"]]),
              actor_loss=np.array([t["actor_loss"] for t in r["train"]]),
              ent_coef=np.array([t["ent_coef"] for t in r["train"]]))
    if r["learned"]:
        fl["ent_coef_loss"] = np.array([t["ent_coef_loss"] for t in r["train"]])
    for k, v in r["final"].items():
        fl[f"final/{k}"] = thin(v)
    for k, v in r["moments"].items():
        fl[f"moment/{k}"] = thin(v, KEEP_MOMENT)
    return {k: np.asarray(v, np.float64) for k, v in fl.items()}


def pack(name, cfg, seed, r32, r64):
    out = {"cfg": json.dumps(dict(cfg, seed=seed, case=name))}
    obs, acts, nxt, dones = make_demos(cfg, seed)
    out.update(demo_obs=obs, demo_acts=acts, demo_next_obs=nxt, demo_dones=dones)
    for k, v in r32["init"].items():
        out[f"init/{k}"] = thin(v)
    adds = r32["adds"]
    out["ring_pos"] = np.array([a[0] for a in adds], np.int64)
    out["ring_reward"] = np.stack([a[4] for a in adds])
    out["ring_done"] = np.stack([a[5] for a in adds])
    out["sample_new_pos"] = np.stack([s[0] for s in r32["new_samples"]])
    out["sample_new_env"] = np.stack([s[1] for s in r32["new_samples"]])
    out["sample_expert_pos"] = np.stack([s[0] for s in r32["expert_samples"]])
    out["sample_expert_env"] = np.stack([s[1] for s in r32["expert_samples"]])
    out["eps"] = np.stack([t["eps"] for t in r32["train"]])
    A = cfg["act_dim"]
    out["act_eps"] = np.stack(r32["act_eps"]) if r32["act_eps"] else np.zeros((0, cfg["n_envs"], A), np.float32)
    out["argmin"] = np.stack([np.stack([t["argmin_target"], t["argmin_pi"]]) for t in r32["train"]])
    out["target_updated"] = np.array([t["target_updated"] for t in r32["train"]])
    out["min_q_gap"], out["q_dev"] = (np.float64(x) for x in q_gap(r32, r64))
    out["branches"] = np.array([BRANCH[a[0]] for a in r32["actions"]], np.int64)
    out["train_n_updates"] = np.array([t["n_updates"] for t in r32["train"]], np.int64)
    out["train_lr"] = np.array([t["lr"] for t in r32["train"]], np.float64)
    out.update(r32["rng"])
    for k, v in r32["counters"].items():
        out[f"counter/{k}"] = np.int64(v)
    out["n_dumps"] = np.int64(len(r32["dumps"]))
    for j, (step, kv) in enumerate(r32["dumps"]):
        keys = sorted(kv)
        out[f"dump{j}_step"] = np.int64(step)
        out[f"dump{j}_keys"] = np.array(keys)
        out[f"dump{j}_vals64"] = np.array([r64["dumps"][j][1][k] for k in keys], np.float64)
    f32, f64 = floats_of(r32), floats_of(r64)
    for k in f64:
        out[f"f64/{k}"] = f64[k]
        out[f"dref/{k}"] = np.float64(rel_l2(f32[k], f64[k]))
    return out


def main(only=None):
    import torch as th
    m = install()
    for name, over in CASES.items():
        if only is not None and name not in only:
            continue
        cfg = dict(COMMON, **over)
        for seed in range(2000):
            r32 = run_once(cfg, seed, m, th.float32)
            r64 = run_once(cfg, seed, m, th.float64)
            why = check(cfg, r32, r64)
            if why is None:
                break
            print(f"{name}: seed {seed} rejected: {why}")
        else:
            raise SystemExit(f"{name}: no seed satisfies the conditions")
        out = pack(name, cfg, seed, r32, r64)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, "seed", seed, "steps", len(out["branches"]), "policy steps", int((out["branches"] == BRANCH["policy"]).sum()),
              "train steps", len(out["train_lr"]), "target updates", int(out["target_updated"].sum()), "dumps", int(out["n_dumps"]),
              "gap", float(out["min_q_gap"]), "q dev", float(out["q_dev"]),
              "dref", {k[5:]: float(f"{float(v):.2e}") for k, v in out.items() if k.startswith("dref/")},
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
