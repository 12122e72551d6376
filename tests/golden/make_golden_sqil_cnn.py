"""Generates `tests/golden/sqil_cnn_*.npz` by running the REFERENCE's own SQIL (`imitation.algorithms.sqil`, imported
unmodified under `oracle.ref_shim`, over `tests/sqil_ref.py`) with `tests/dqn_cnn_ref.CnnPolicy` on this package's
`SyntheticImageVecEnv`. Runs only where the reference sources are present.
Usage: `python tests/golden/make_golden_sqil_cnn.py [case ...]`.

Every case runs twice from the same seeds, in float32 and in float64, and a seed is kept under exactly the conditions of
`make_golden_sqil.check` (imported). What is stored differs from the flat fixtures only where size demands it (about 82 k
online parameters, frames of 5 - 6 KB):

* `init/` and `f64/final/` (+ `f32/final/`, `dref/final/`) hold the ONLINE net only (`q_net.*`); the generator asserts that
  the initial target equals it. The final target needs no data: with `tau = 1` it is the online net at the last update.
* no frames: per ring write `zlib.crc32` of the `obs` rows and of the `next_obs` rows, with position, actions and dones; one
  CRC over the demonstrations, which the tests regenerate from the seed.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_golden_sqil import check, install, rel_l2  # noqa: E402

from tests.sqil_cnn_golden import CASES, COMMON, crc, demo_crc, make_demos, make_env, rl_kwargs_of  # noqa: E402
from tests.sqil_golden import BRANCH, GAP_MARGIN, seed_everything  # noqa: E402


def run_once(cfg, seed, m, dtype):
    import torch as th
    from tests import dqn_cnn_ref
    ref, sb = m["ref"], m["sb"]
    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = m["types"].Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones, infos=np.array([{}] * len(obs)))
    seed_everything(venv, seed)
    ref.DQN.dtype = dtype
    try:
        algo = m["sqil"].SQIL(venv=venv, demonstrations=demos, policy=dqn_cnn_ref.CnnPolicy, rl_kwargs=rl_kwargs_of(cfg))
    finally:
        ref.DQN.dtype = th.float32
    rl = algo.rl_algo
    sd = rl.policy.state_dict()
    for k, v in sd.items():
        if k.startswith("q_net."):
            assert th.equal(v, sd["q_net_target." + k[len("q_net."):]]), k
    init = {k: v.detach().numpy().astype(np.float32) for k, v in sd.items() if k.startswith("q_net.")}
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
    return dict(init=init, dumps=dumps, adds=rb.add_log, new_samples=rb.sample_log,
                expert_samples=rb.expert_buffer.sample_log, actions=rl.action_log, eps=rl.eps_log,
                target_updates=rl.target_update_log, train=rl.train_log,
                final={k: v.detach().numpy() for k, v in rl.policy.state_dict().items() if k.startswith("q_net.")},
                counters=dict(num_timesteps=rl.num_timesteps, n_updates=rl._n_updates, n_calls=rl._n_calls,
                              episodes=rl._episode_num, pos=rb.pos, full=bool(rb.full)))


def pack(name, cfg, seed, r32, r64):
    out = {"cfg": json.dumps(dict(cfg, seed=seed, gap_margin=GAP_MARGIN, case=name))}
    _, acts, _, dones = make_demos(cfg, seed)
    out.update(demo_crc=np.int64(demo_crc(cfg, seed)), demo_acts=acts, demo_dones=dones)
    for k, v in r32["init"].items():
        out[f"init/{k}"] = v
    adds = r32["adds"]
    out["ring_pos"] = np.array([a[0] for a in adds], np.int64)
    out["ring_obs_crc"] = np.array([crc(a[1]) for a in adds], np.int64)
    out["ring_next_obs_crc"] = np.array([crc(a[2]) for a in adds], np.int64)
    for i, key in ((3, "ring_action"), (4, "ring_reward"), (5, "ring_done")):
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
    for k, v in floats["f64"].items():
        out[f"f64/{k}"] = v
    for k in ("loss", "greedy_q"):   # (the float32 run's parameters are not stored: `dref/` is what a test needs of them)
        if k in floats["f32"]:
            out[f"f32/{k}"] = floats["f32"][k].astype(np.float32)
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
        print(name, "seed", seed, "steps", len(out["branches"]), "greedy", n_greedy, "train steps", len(out["f64/loss"]),
              "dumps", int(out["n_dumps"]), "dref", {k[5:]: float(v) for k, v in out.items() if k.startswith("dref/")},
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
