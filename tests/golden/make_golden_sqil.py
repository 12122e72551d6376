"""Generates `tests/golden/sqil_*.npz` by running the REFERENCE's own SQIL (`imitation.algorithms.sqil`, imported
unmodified under `oracle.ref_shim`) on this package's `SyntheticVecEnv`. Runs only where the reference sources are present.
Usage: `python tests/golden/make_golden_sqil.py [case ...]`.

The shim has no `stable_baselines3.dqn`, `.common.buffers`, `.common.off_policy_algorithm` or `.common.type_aliases`:
`tests/sqil_ref.py` (a restatement of SB3 2.2.x) supplies them in this process. Every case runs twice from the same seeds,
in float32 and in float64, and a seed is kept only if

* every greedy decision has the same arg-max in both runs, a top-two gap above `GAP_MARGIN` in both, and Q-values that
  differ by less than a tenth of the margin -- so that a test can compare ALL actions and ring contents exactly;
* a case that takes greedy steps takes at least 10; both branches of the Huber loss occur; at least one target update
  falls between two `train` calls.

Each file holds the settings, the demonstrations, the initial parameters, every ring write, every sampled index
quadruple, every action with its branch, the exploration rates, the target updates, every logger dump, the per-step
losses, the Q-values of the greedy rows and the final parameters -- floating values of BOTH runs (`f32/`, `f64/`), and per
float key `dref/` = the relative L2 deviation of the float32 run from the float64 run (the device path is allowed 8 x).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim  # noqa: E402

from tests.sqil_golden import (BRANCH, CASES, COMMON, GAP_MARGIN, make_demos, make_env, rl_kwargs_of,  # noqa: E402
                                seed_everything)


def install():
    ref_shim.install()
    from tests import sqil_ref
    sqil_ref.install_sb3_modules()
    from oracle import sb3_restated as sb
    if not hasattr(sb.Logger, "warn"):
        sb.Logger.warn = lambda self, *args, **kwargs: None
    from imitation.algorithms import sqil
    from imitation.data import types
    return dict(sqil=sqil, types=types, sb=sb, ref=sqil_ref)


def run_once(cfg, seed, m, dtype):
    import torch as th
    ref, sb = m["ref"], m["sb"]
    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = m["types"].Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones, infos=np.array([{}] * len(obs)))
    seed_everything(venv, seed)
    ref.DQN.dtype = dtype
    try:
        algo = m["sqil"].SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy", rl_kwargs=rl_kwargs_of(cfg))
    finally:
        ref.DQN.dtype = th.float32
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
    out = dict(init=init, dumps=dumps, adds=rb.add_log, new_samples=rb.sample_log,
               expert_samples=rb.expert_buffer.sample_log, actions=rl.action_log, eps=rl.eps_log,
               target_updates=rl.target_update_log, train=rl.train_log,
               final={k: v.detach().numpy() for k, v in rl.policy.state_dict().items()},
               counters=dict(num_timesteps=rl.num_timesteps, n_updates=rl._n_updates, n_calls=rl._n_calls,
                             episodes=rl._episode_num, pos=rb.pos, full=bool(rb.full)))
    return out


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check(cfg, r32, r64):
    """None if the pair of runs satisfies the conditions in the module docstring, else the reason."""
    if len(r32["actions"]) != len(r64["actions"]):
        return "different number of steps"
    n_greedy = 0
    for (b32, a32, q32), (b64, a64, q64) in zip(r32["actions"], r64["actions"]):
        if b32 != b64 or not np.array_equal(a32, a64):
            return "the float32 and float64 runs take different actions"
        if b32 == "greedy":
            n_greedy += 1
            for q in (q32, q64):
                top = np.sort(q, axis=1)
                if (top[:, -1] - top[:, -2]).min() <= GAP_MARGIN:
                    return "a greedy row's top-two gap is inside the margin"
            if not np.array_equal(q32.argmax(1), q64.argmax(1)):
                return "arg-max differs"
            if np.abs(q32 - q64).max() >= GAP_MARGIN / 10:
                return "|Q32 - Q64| too large"
    wants_greedy = cfg["exploration_final_eps"] < 1.0
    if wants_greedy and n_greedy < 10:
        return f"only {n_greedy} greedy steps"
    if not wants_greedy and n_greedy:
        return "greedy steps in the all-random case"
    for r in (r32, r64):
        td = np.concatenate([t["abs_td"] for t in r["train"]])
        if not ((td < 1).any() and (td >= 1).any()):
            return "one branch of the Huber loss does not occur"
    calls = sorted({t["n_calls"] for t in r32["train"]})
    if not any(calls[0] < u <= calls[-1] for u in r32["target_updates"]):
        return "no target update between two train calls"
    for k in ("adds", "new_samples", "expert_samples"):
        for x, y in zip(r32[k], r64[k]):
            if not all(np.array_equal(p, q) for p, q in zip(x, y)):
                return f"{k} differ between the runs"
    return None


def pack(name, cfg, seed, r32, r64):
    out = {"cfg": json.dumps(dict(cfg, seed=seed, gap_margin=GAP_MARGIN, case=name))}
    obs, acts, nxt, dones = make_demos(cfg, seed)
    out.update(demo_obs=obs, demo_acts=acts, demo_next_obs=nxt, demo_dones=dones)
    for k, v in r32["init"].items():
        out[f"init/{k}"] = v
    adds = r32["adds"]
    out["ring_pos"] = np.array([a[0] for a in adds], np.int64)
    for i, key in enumerate(("ring_obs", "ring_next_obs", "ring_action", "ring_reward", "ring_done"), start=1):
        out[key] = np.stack([a[i] for a in adds])
    out["sample_new_pos"] = np.stack([s[0] for s in r32["new_samples"]])
    out["sample_new_env"] = np.stack([s[1] for s in r32["new_samples"]])
    out["sample_expert_pos"] = np.stack([s[0] for s in r32["expert_samples"]])
    out["sample_expert_env"] = np.stack([s[1] for s in r32["expert_samples"]])
    out["actions"] = np.stack([a[1] for a in r32["actions"]]).astype(np.int64)
    out["branches"] = np.array([BRANCH[a[0]] for a in r32["actions"]], np.int64)
    out["exploration_rate"] = np.array(r32["eps"], np.float64)
    out["target_updates"] = np.array(r32["target_updates"], np.int64)
    out["train_n_calls"] = np.array([t["n_calls"] for t in r32["train"]], np.int64)
    out["train_lr"] = np.array([t["lr"] for t in r32["train"]], np.float64)
    for k, v in r32["counters"].items():
        out[f"counter/{k}"] = np.int64(v)
    out["n_dumps"] = np.int64(len(r32["dumps"]))
    for j, (step, kv) in enumerate(r32["dumps"]):
        keys = sorted(kv)
        out[f"dump{j}_step"] = np.int64(step)
        out[f"dump{j}_keys"] = np.array(keys)
        out[f"dump{j}_vals"] = np.array([kv[k] for k in keys], np.float64)
        out[f"dump{j}_vals64"] = np.array([r64["dumps"][j][1][k] for k in keys], np.float64)
    floats = {}
    for tag, r in (("f32", r32), ("f64", r64)):
        fl = {"loss": np.array([t["loss"] for t in r["train"]], np.float64)}
        gq = [a[2] for a in r["actions"] if a[0] == "greedy"]
        if gq:
            fl["greedy_q"] = np.concatenate(gq).astype(np.float64)
        for k, v in r["final"].items():
            fl[f"final/{k}"] = np.asarray(v, np.float64)
        floats[tag] = fl
        for k, v in fl.items():
            out[f"{tag}/{k}"] = v if tag == "f64" else v.astype(np.float32)
    for k in floats["f32"]:
        out[f"dref/{k}"] = np.float64(rel_l2(floats["f32"][k], floats["f64"][k]))
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
        n_greedy = int((out["branches"] == BRANCH["greedy"]).sum())
        print(name, "seed", seed, "steps", len(out["branches"]), "greedy", n_greedy, "train steps", len(out["f32/loss"]),
              "dumps", int(out["n_dumps"]), "dref", {k[5:]: float(v) for k, v in out.items() if k.startswith("dref/")},
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
