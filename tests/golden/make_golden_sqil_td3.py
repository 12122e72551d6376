"""Generates `tests/golden/sqil_td3_*.npz` by running the REFERENCE's own SQIL (`imitation.algorithms.sqil`, imported
unmodified under `oracle.ref_shim`) with `rl_algo_class` = the restated TD3 / DDPG of `tests/td3_ref.py` on this package's
`SyntheticVecEnv` with Box actions. Runs only where the reference sources are present.
Usage: `python tests/golden/make_golden_sqil_td3.py [case ...]`.

Every case runs twice from the same seeds, in float32 and in float64, and a seed is kept only if, in BOTH runs,

* the target-noise clip binds on some elements and not on others (TD3 only: DDPG's clip of 0 binds on every element);
* the clamp of the next action at +-1 binds somewhere (TD3 only: without noise a tanh output never leaves [-1, 1]);
* at least one `done = 1` row is sampled;
* at least one actor update and one skipped actor update occur (TD3 only: DDPG updates the actor in every step);
* training starts before the run ends;

and the two runs make the same index draws, draw the same noise and leave both generators in the same state.

Each file holds the settings, the demonstrations, every ring write, every sampled index, the noise tensors, every action
with its branch, the logger dumps, the per-step losses, which steps updated the actor, both generators' post-states, the
counters and -- thinned to `td3_golden.KEEP` evenly spaced elements per tensor (`KEEP_MOMENT` per optimiser's moment vector),
since the [400, 300] nets would not fit otherwise -- the initial parameters (float32, exact), the final parameters and
Adam's moments. Floating values are those of
the float64 run (`f64/`); per float key `dref/` = the relative L2 deviation of the float32 run from the float64 run (the
device path is allowed 8 x).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim  # noqa: E402

from tests.td3_golden import (BRANCH, CASES, COMMON, KEEP_MOMENT, make_demos, make_env, rl_kwargs_of, rng_states,  # noqa: E402
                               seed_everything, thin)


def install():
    ref_shim.install()
    from tests import td3_ref
    td3_ref.install_sb3_modules()
    from oracle import sb3_restated as sb
    if not hasattr(sb.Logger, "warn"):
        sb.Logger.warn = lambda self, *args, **kwargs: None
    from imitation.algorithms import sqil
    from imitation.data import types
    return dict(sqil=sqil, types=types, sb=sb, ref=td3_ref)


def run_once(cfg, seed, m, dtype):
    import torch as th
    ref, sb = m["ref"], m["sb"]
    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = m["types"].Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones, infos=np.array([{}] * len(obs)))
    seed_everything(venv, seed)
    ref.TD3.dtype = dtype
    try:
        algo = m["sqil"].SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy", rl_algo_class=getattr(ref, cfg["algo"]),
                              rl_kwargs=rl_kwargs_of(cfg, ref.NormalActionNoise))
    finally:
        ref.TD3.dtype = th.float32
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
    return dict(init=init, dumps=dumps, adds=rb.add_log, new_samples=rb.sample_log,
                expert_samples=rb.expert_buffer.sample_log, actions=rl.action_log, train=rl.train_log,
                final={k: v.detach().numpy() for k, v in rl.policy.state_dict().items()}, moments=moments, rng=rng_states(),
                counters=dict(num_timesteps=rl.num_timesteps, n_updates=rl._n_updates, episodes=rl._episode_num, pos=rb.pos,
                              full=bool(rb.full)))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check(cfg, r32, r64):
    """None if the pair of runs satisfies the conditions in the module docstring, else the reason."""
    td3 = cfg["algo"] == "TD3"
    for r in (r32, r64):
        if not r["train"]:
            return "training never starts"
        clipped, total = sum(t["n_noise_clipped"] for t in r["train"]), sum(t["n_noise"] for t in r["train"])
        if td3 and not 0 < clipped < total:
            return "the noise clip does not both bind and not bind"
        if td3 and not sum(t["n_action_clamped"] for t in r["train"]):
            return "the action clamp never binds"
        if not any((t["dones"] == 1).any() for t in r["train"]):
            return "no done row is sampled"
        updated = [t["actor_loss"] is not None for t in r["train"]]
        if not any(updated) or (td3 and all(updated)):
            return "actor updates and skipped actor updates do not both occur"
    if len(r32["actions"]) != len(r64["actions"]) or [a[0] for a in r32["actions"]] != [a[0] for a in r64["actions"]]:
        return "the runs take different branches"
    for k in ("new_samples", "expert_samples"):
        for x, y in zip(r32[k], r64[k]):
            if not all(np.array_equal(p, q) for p, q in zip(x, y)):
                return f"{k} differ between the runs"
    if [a[0] for a in r32["adds"]] != [a[0] for a in r64["adds"]]:
        return "ring positions differ"
    if not all(np.array_equal(s["noise"], t["noise"]) for s, t in zip(r32["train"], r64["train"])):
        return "noise differs"
    if not all(np.array_equal(r32["rng"][k], r64["rng"][k]) for k in r32["rng"]):
        return "generator post-states differ"
    return None


def floats_of(r):
    fl = dict(ring_obs=np.stack([a[1] for a in r["adds"]]), ring_next_obs=np.stack([a[2] for a in r["adds"]]),
              ring_action=np.stack([a[3] for a in r["adds"]]), actions=np.stack([a[1] for a in r["actions"]]),
              buffer_actions=np.stack([a[2] for a in r["actions"]]),
              critic_loss=np.array([t["critic_loss"] for t in r["train"]]),
              actor_loss=np.array([t["actor_loss"] for t in r["train"] if t["actor_loss"] is not None]))
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
    out["noise"] = np.stack([t["noise"] for t in r32["train"]])
    out["branches"] = np.array([BRANCH[a[0]] for a in r32["actions"]], np.int64)
    out["train_n_updates"] = np.array([t["n_updates"] for t in r32["train"]], np.int64)
    out["train_lr"] = np.array([t["lr"] for t in r32["train"]], np.float64)
    out["actor_steps"] = np.array([t["actor_loss"] is not None for t in r32["train"]])
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
        for seed in range(200):
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
              "train steps", len(out["train_lr"]), "actor updates", int(out["actor_steps"].sum()), "dumps", int(out["n_dumps"]),
              "dref", {k[5:]: float(f"{float(v):.2e}") for k, v in out.items() if k.startswith("dref/")},
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
