"""Generates `tests/golden/gail_dqn_cnn_*.npz` by running the REFERENCE's own GAIL (`imitation.algorithms.adversarial.gail`,
imported unmodified under `oracle.ref_shim`) with the restated DQN of `tests/sqil_ref.py` and `tests/dqn_cnn_ref.CnnPolicy` as
`gen_algo`, the reference's `CnnRewardNet(hwc_format=False)` as the discriminator, on this package's
`SyntheticImageVecEnv`. Runs only where the reference sources are present.
Usage: `python tests/golden/make_golden_gail_dqn_cnn.py [case ...]`.

Every case runs THREE times from the same seeds: in float32 as the reference is; in float32 inside
`torch.backends.mkldnn.flags(enabled=False)`, a second summation order of the same convolutions; and in float64, widened as
in `make_golden_gail_offpolicy.run_once` (the learner through the restatement's `dtype` switch, the discriminator by
`reward_net.double()` after its float32 initialisation with a forward pre-hook on `net.cnn` that widens its input, the
BCE's labels widened on their way in). A seed is kept under the conditions of `make_golden_gail_offpolicy.check`, applied
to each float32 run against the float64 run: all three runs make the same index draws, ring writes and branches.

What is stored follows the image-SQIL fixtures: CRCs instead of frames (every learner-ring write, the trainer's ring after
every round, the demonstrations), the learner's ONLINE net only (its initial parameters as one CRC per tensor), all index
records, and per float key `f64/`, `f32/` (the plain float32 run; parameters excepted) and `dref/` = the LARGER of the two
float32 runs' relative L2 deviations from the float64 run (the device path is allowed 8 x).
"""
import contextlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_golden_gail_offpolicy import FLOAT_ALWAYS, _WideLabels, check, install, rel_l2  # noqa: E402

from tests.gail_dqn_cnn_golden import (BRANCH, CASES, COMMON, GAP_MARGIN, NOT_COMPARED_PREFIX, demo_crc,  # noqa: E402
                                        frames_to_crc, make_demos, make_env, rl_kwargs_of, seed_everything)
from tests.gail_offpolicy_golden import Tap, pool_params  # noqa: E402

MODES = ("f32", "f32_plain_conv", "f64")


def run_once(cfg, seed, m, mode):
    import torch as th

    from tests import dqn_cnn_ref
    wide = mode == "f64"
    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = m["types"].Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones, infos=np.array([{}] * len(obs)))
    seed_everything(venv, seed)
    cls = m["DQN"]
    cls.dtype = th.float64 if wide else th.float32
    F_orig = m["common"].F
    conv = th.backends.mkldnn.flags(enabled=False) if mode == "f32_plain_conv" else contextlib.nullcontext()
    try:
        with conv:
            rl = cls(dqn_cnn_ref.CnnPolicy, venv, **rl_kwargs_of(cfg))
            f = cfg["flags"]
            net = m["rn"].CnnRewardNet(venv.observation_space, venv.action_space, use_state=f[0], use_action=f[1],
                                       use_next_state=f[2], use_done=f[3], hwc_format=False)
            if wide:
                net.double()
                net.cnn.register_forward_pre_hook(lambda mod, inp: (inp[0].double(),))
                m["common"].F = _WideLabels(F_orig)
            trainer = m["gail"].GAIL(demonstrations=demos, demo_batch_size=cfg["demo_batch_size"], venv=venv, gen_algo=rl,
                                     reward_net=net, n_disc_updates_per_round=cfg["n_disc"],
                                     gen_train_timesteps=cfg["gen_train_timesteps"],
                                     custom_logger=m["logger"].configure(tempfile.mkdtemp(), []),
                                     allow_variable_horizon=False)
            sd = rl.policy.state_dict()
            for k, v in sd.items():
                if k.startswith("q_net."):
                    assert th.equal(v, sd["q_net_target." + k[len("q_net."):]]), k
            init = {f"init/{k}": v.detach().numpy().astype(np.float32) for k, v in sd.items()}
            init.update({f"disc_init/{k}": v.detach().numpy().astype(np.float32) for k, v in net.state_dict().items()})
            rb, buf = rl.replay_buffer, trainer._gen_replay_buffer
            assert rb.observations.dtype == np.uint8 and buf._buffer._arrays["obs"].dtype == np.uint8
            tap = Tap(trainer, cfg, learner_rewards=lambda: rb.rewards.copy(),
                      gen_ring=lambda: dict({k: np.array(buf._buffer._arrays[k]) for k in ("obs", "acts", "next_obs", "dones")},
                                            idx=buf._buffer._idx, n_data=buf._buffer._n_data))
            trainer.train(cfg["rounds"] * cfg["gen_train_timesteps"], callback=tap.end_of_round)
    finally:
        cls.dtype = th.float32
        m["common"].F = F_orig
    out = tap.record()
    n = cfg["n_envs"]
    out.update(init)
    out["actions"] = np.stack([a[1] for a in rl.action_log])
    out["branches"] = np.array([BRANCH[a[0]] for a in rl.action_log], np.int64)
    out["sample_rows"] = np.stack([s[0] * n + s[1] for s in rb.sample_log])
    out["greedy_q"] = [a[2] for a in rl.action_log if a[0] == "greedy"]
    out["train_at"] = np.array([t["n_calls"] for t in rl.train_log], np.int64)
    out["loss"] = np.array([t["loss"] for t in rl.train_log], np.float64)
    out["exploration_rate"] = np.array(rl.eps_log, np.float64)
    out["target_updates"] = np.array(rl.target_update_log, np.int64)
    for k, v in dict(num_timesteps=rl.num_timesteps, n_updates=rl._n_updates, episodes=rl._episode_num, pos=rb.pos,
                     full=int(rb.full), global_step=trainer._global_step, disc_step=trainer._disc_step).items():
        out[f"counter/{k}"] = np.int64(v)
    for k, v in rl.policy.state_dict().items():
        out[f"final/{k}"] = v.detach().numpy().astype(np.float64)
    for k, v in net.state_dict().items():
        out[f"disc_final/{k}"] = v.detach().numpy().astype(np.float64)
    return pool_params(out)


def first_round_rewards(cfg, rec):
    """The rewards of the first round's ring writes: computed before any optimiser step of either net."""
    return np.asarray(rec["ring_reward"])[:cfg["gen_train_timesteps"] // cfg["n_envs"]]


def pack(name, cfg, seed, runs):
    r32, r32b, r64 = (frames_to_crc(runs[k]) for k in MODES)
    out = {"cfg": json.dumps(dict(cfg, seed=seed, gap_margin=GAP_MARGIN, case=name))}
    _, acts, _, dones = make_demos(cfg, seed)
    out.update(demo_crc=np.int64(demo_crc(cfg, seed)), demo_acts=acts, demo_dones=dones)
    floats = {"f32": {}, "f32b": {}, "f64": {}}
    for k, v in r32.items():
        if k == "greedy_q":
            for tag, r in (("f32", r32), ("f32b", r32b), ("f64", r64)):
                floats[tag][k] = np.concatenate(r[k]).astype(np.float64)
        elif k in FLOAT_ALWAYS or k.startswith(("final/", "disc_final/")):
            for tag, r in (("f32", r32), ("f32b", r32b), ("f64", r64)):
                floats[tag][k] = np.asarray(r[k], np.float64)
        elif k.startswith("dump") and k.endswith("_vals"):
            out[k] = v
            out[k + "64"] = r64[k]
        else:
            out[k] = v
    for k, v in floats["f64"].items():
        out[f"f64/{k}"] = v
    for k, v in floats["f32"].items():
        if not k.startswith(("final/", "disc_final/")):   # (`dref/` is what a test needs of the float32 parameters)
            out[f"f32/{k}"] = v.astype(np.float32)
    for k in floats["f32"]:
        out[f"dref/{k}"] = np.float64(max(rel_l2(floats["f32"][k], floats["f64"][k]), rel_l2(floats["f32b"][k], floats["f64"][k])))
    out["dref_first_round/ring_reward"] = np.float64(max(
        rel_l2(first_round_rewards(cfg, r), first_round_rewards(cfg, r64)) for r in (r32, r32b)))
    # per logger key: the deviation over all of its dumps, the larger of the two float32 runs'
    per_key = {}
    for j in range(int(r32["n_dumps"])):
        for i, k in enumerate(r32[f"dump{j}_keys"]):
            if NOT_COMPARED_PREFIX not in str(k):
                rec = per_key.setdefault(str(k), ([], [], []))
                for dst, r in zip(rec, (r32, r32b, r64)):
                    dst.append(r[f"dump{j}_vals"][i])
    out["log_keys"] = np.array(sorted(per_key))
    out["log_dref"] = np.array([max(rel_l2(per_key[k][0], per_key[k][2]), rel_l2(per_key[k][1], per_key[k][2]))
                                for k in sorted(per_key)], np.float64)
    return out


def main(only=None, first_seed=0):
    m = install()
    for name, over in CASES.items():
        if only is not None and name not in only:
            continue
        cfg = dict(COMMON, **over)
        for seed in range(first_seed, 200):
            runs = {mode: run_once(cfg, seed, m, mode) for mode in MODES}
            why = check(cfg, runs["f32"], runs["f64"]) or check(cfg, runs["f32_plain_conv"], runs["f64"])
            if why is None:
                break
            print(f"{name}: seed {seed} rejected: {why}")
        else:
            raise SystemExit(f"{name}: no seed satisfies the conditions")
        out = pack(name, cfg, seed, runs)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, "seed", seed, "steps", len(out["branches"]), "branches", np.bincount(out["branches"], minlength=4).tolist(),
              "train steps", len(out["f32/loss"]), "dumps", int(out["n_dumps"]),
              "dref", {k[5:]: f"{float(v):.2e}" for k, v in out.items() if k.startswith("dref")},
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    args = sys.argv[1:]
    first = 0
    if args and args[0].startswith("--first-seed="):
        first = int(args.pop(0).split("=")[1])
    main(args or None, first)
