"""Generates `tests/golden/gail_dqn.npz`, `gail_dqn_next_done.npz` and `gail_td3.npz` by running the REFERENCE's own GAIL
(`imitation.algorithms.adversarial.gail`, imported unmodified under `oracle.ref_shim`) with the restated off-policy learners
of `tests/sqil_ref.py` (DQN) and `tests/td3_ref.py` (TD3) as `gen_algo`, on this package's `SyntheticVecEnv`. Runs only where
the reference sources are present. Usage: `python tests/golden/make_golden_gail_offpolicy.py [case ...]`.

The learner half is a restatement of SB3 (SB3 itself is installed nowhere this project runs): that half is parity unpinned,
as for the SQIL fixtures. The trainer, the wrappers, the buffers and the reward nets are the reference's.

Every case runs twice from the same seeds, in float32 (the reference as it is) and in float64. The float64 run widens the
learner through the restatement's `dtype` switch and the discriminator by `reward_net.double()` after its float32
initialisation, a forward pre-hook that widens the stack's input, and labels widened on their way into
`binary_cross_entropy_with_logits`; no line of the reference is changed. A seed is kept only if both runs make the same
index draws and ring writes, and, for DQN, every greedy decision has the same arg-max in both runs, a top-two gap above
`GAP_MARGIN` in both and Q-values that differ by less than a tenth of the margin; at least 10 greedy steps occur.

Each file holds the settings, the initial parameters of both nets, every learner-ring write with the reward the step's
relabelling left there, the trainer's replay ring after every round, every sampled index row, every action with its
branch, exploration rates and target updates (DQN), every logger dump, the per-step losses and the final parameters of
both nets (one float key per tensor, see `gail_offpolicy_golden.pool_params`): floating values of BOTH runs (`f32/`,
`f64/`) and per float key `dref/` = the relative L2 deviation of the float32 run from the float64 run (the device path is
allowed 8 x).
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim  # noqa: E402

from tests.gail_offpolicy_golden import (BRANCH, CASES, COMMON, GAP_MARGIN, NOT_COMPARED_PREFIX, Tap, is_exact,  # noqa: E402
                                          make_demos, make_env, pool_params, rl_kwargs_of, seed_everything)


def install():
    ref_shim.install()
    from tests import sqil_ref, td3_ref
    sqil_ref.install_sb3_modules()
    td3_ref.install_sb3_modules()
    from oracle import sb3_restated as sb
    if not hasattr(sb.Logger, "warn"):
        sb.Logger.warn = lambda self, *args, **kwargs: None
    from imitation.algorithms.adversarial import common as ref_common
    from imitation.algorithms.adversarial import gail
    from imitation.data import types
    from imitation.rewards import reward_nets
    from imitation.util import logger as ref_logger
    from imitation.util import networks
    return dict(gail=gail, common=ref_common, types=types, rn=reward_nets, logger=ref_logger, networks=networks, sb=sb,
                DQN=sqil_ref.DQN, TD3=td3_ref.TD3, noise=td3_ref.NormalActionNoise)


class _WideLabels:
    """`torch.nn.functional` with the labels of the BCE widened to the logits' dtype (float64 run only)."""

    def __init__(self, F):
        self._F = F

    def __getattr__(self, name):
        return getattr(self._F, name)

    def binary_cross_entropy_with_logits(self, input, target, *a, **k):
        return self._F.binary_cross_entropy_with_logits(input, target.to(input.dtype), *a, **k)


def run_once(cfg, seed, m, dtype):
    import torch as th
    wide = dtype is th.float64
    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = m["types"].Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones, infos=np.array([{}] * len(obs)))
    seed_everything(venv, seed)
    cls = m[cfg["algo"]]
    cls.dtype = dtype
    F_orig = m["common"].F
    try:
        rl = cls("MlpPolicy", venv, **rl_kwargs_of(cfg, m["noise"]))
        f = cfg["flags"]
        net = m["rn"].BasicRewardNet(venv.observation_space, venv.action_space, use_state=f[0], use_action=f[1],
                                     use_next_state=f[2], use_done=f[3], normalize_input_layer=m["networks"].RunningNorm)
        if wide:
            net.double()
            net.mlp.register_forward_pre_hook(lambda mod, inp: (inp[0].double(),))
            m["common"].F = _WideLabels(F_orig)
        trainer = m["gail"].GAIL(demonstrations=demos, demo_batch_size=cfg["demo_batch_size"], venv=venv, gen_algo=rl,
                                 reward_net=net, n_disc_updates_per_round=cfg["n_disc"],
                                 gen_train_timesteps=cfg["gen_train_timesteps"],
                                 custom_logger=m["logger"].configure(tempfile.mkdtemp(), []), allow_variable_horizon=False)
        init = {f"init/{k}": v.detach().numpy().astype(np.float32) for k, v in rl.policy.state_dict().items()}
        init.update({f"disc_init/{k}": v.detach().numpy().astype(np.float32) if v.is_floating_point() else v.numpy().copy()
                     for k, v in net.state_dict().items()})
        rb, buf = rl.replay_buffer, trainer._gen_replay_buffer
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
    if cfg["algo"] == "DQN":
        out["greedy_q"] = [a[2] for a in rl.action_log if a[0] == "greedy"]
        out["train_at"] = np.array([t["n_calls"] for t in rl.train_log], np.int64)
        out["loss"] = np.array([t["loss"] for t in rl.train_log], np.float64)
        out["exploration_rate"] = np.array(rl.eps_log, np.float64)
        out["target_updates"] = np.array(rl.target_update_log, np.int64)
    else:
        out["train_at"] = np.array([t["n_updates"] for t in rl.train_log], np.int64)
        out["loss"] = np.array([t["critic_loss"] for t in rl.train_log], np.float64)
        out["actor_loss"] = np.array([t["actor_loss"] for t in rl.train_log if t["actor_loss"] is not None], np.float64)
    for k, v in dict(num_timesteps=rl.num_timesteps, n_updates=rl._n_updates, episodes=rl._episode_num, pos=rb.pos,
                     full=int(rb.full), global_step=trainer._global_step, disc_step=trainer._disc_step).items():
        out[f"counter/{k}"] = np.int64(v)
    for k, v in rl.policy.state_dict().items():
        out[f"final/{k}"] = v.detach().numpy().astype(np.float64)
    for k, v in net.state_dict().items():
        out[f"disc_final/{k}"] = v.detach().numpy().astype(np.float64)
    return pool_params(out)


FLOAT_ALWAYS = ("ring_reward", "loss", "actor_loss", "disc_norm/running_mean", "disc_norm/running_var")
ROW_KEYS = ("ring_obs", "ring_next_obs", "ring_action", "actions", "gen_obs", "gen_acts", "gen_next_obs")
INDEX_KEYS = ("ring_pos", "ring_done", "ring_timeout", "branches", "sample_rows", "train_at", "gen_dones", "gen_idx",
              "gen_n_data", "n_dumps", "exploration_rate", "target_updates", "disc_norm_count")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check(cfg, r32, r64):
    """None if the pair of runs satisfies the conditions in the module docstring, else the reason."""
    for k in INDEX_KEYS + tuple(k for k in ROW_KEYS if is_exact(cfg, k)):
        if k in r32 and not np.array_equal(r32[k], r64[k]):
            return f"{k} differs between the float32 and the float64 run"
    if int(r32["n_dumps"]) == 0:
        return "no logger dump"
    for j in range(int(r32["n_dumps"])):
        if list(r32[f"dump{j}_keys"]) != list(r64[f"dump{j}_keys"]) or r32[f"dump{j}_step"] != r64[f"dump{j}_step"]:
            return "logger dumps differ"
    if cfg["algo"] == "DQN":
        n_greedy = len(r32["greedy_q"])
        if n_greedy < 10:
            return f"only {n_greedy} greedy steps"
        for q32, q64 in zip(r32["greedy_q"], r64["greedy_q"]):
            for q in (q32, q64):
                top = np.sort(q, axis=1)
                if (top[:, -1] - top[:, -2]).min() <= GAP_MARGIN:
                    return "a greedy row's top-two gap is inside the margin"
            if not np.array_equal(q32.argmax(1), q64.argmax(1)):
                return "arg-max differs"
            if np.abs(q32 - q64).max() >= GAP_MARGIN / 10:
                return "|Q32 - Q64| too large"
        if not len(r32["target_updates"]):
            return "no target update"
    if not len(r32["loss"]):
        return "no training step"
    if not r32["ring_done"].any() or not r32["ring_timeout"].any():
        return "no episode end"
    return None


def pack(name, cfg, seed, r32, r64):
    out = {"cfg": json.dumps(dict(cfg, seed=seed, gap_margin=GAP_MARGIN, case=name))}
    obs, acts, nxt, dones = make_demos(cfg, seed)
    out.update(demo_obs=obs, demo_acts=acts, demo_next_obs=nxt, demo_dones=dones)
    floats = {"f32": {}, "f64": {}}
    for k, v in r32.items():
        if k == "greedy_q":
            floats["f32"][k] = np.concatenate(v).astype(np.float64)
            floats["f64"][k] = np.concatenate(r64[k]).astype(np.float64)
        elif k in FLOAT_ALWAYS or k.startswith(("final/", "disc_final/")) or (k in ROW_KEYS and not is_exact(cfg, k)):
            floats["f32"][k], floats["f64"][k] = np.asarray(v, np.float64), np.asarray(r64[k], np.float64)
        elif k.startswith("dump") and k.endswith("_vals"):
            out[k] = v
            out[k + "64"] = r64[k]
        else:
            out[k] = v
    for tag in ("f32", "f64"):
        for k, v in floats[tag].items():
            out[f"{tag}/{k}"] = v if tag == "f64" else v.astype(np.float32)
    for k in floats["f32"]:
        out[f"dref/{k}"] = np.float64(rel_l2(floats["f32"][k], floats["f64"][k]))
    # per logger key: the deviation over all of its dumps
    per_key = {}
    for j in range(int(r32["n_dumps"])):
        for k, a, b in zip(r32[f"dump{j}_keys"], r32[f"dump{j}_vals"], r64[f"dump{j}_vals"]):
            if NOT_COMPARED_PREFIX not in str(k):
                per_key.setdefault(str(k), ([], []))
                per_key[str(k)][0].append(a)
                per_key[str(k)][1].append(b)
    out["log_keys"] = np.array(sorted(per_key))
    out["log_dref"] = np.array([rel_l2(*per_key[k]) for k in sorted(per_key)], np.float64)
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
        print(name, "seed", seed, "steps", len(out["branches"]), "branches", np.bincount(out["branches"], minlength=4).tolist(),
              "train steps", len(out["f32/loss"]), "dumps", int(out["n_dumps"]),
              "dref", {k[5:]: f"{float(v):.2e}" for k, v in out.items() if k.startswith("dref/")},
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
