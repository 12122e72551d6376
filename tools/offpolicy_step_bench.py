"""Microseconds per environment step of `AdversarialTrainer.train_gen` with an off-policy generator on the GPU: the fused
step (`step_source.RewardStepSource`, one `ia_offpolicy_step` launch per step, csrc/offpolicy.hip) against the per-step host path
(`IA_OFFPOLICY_FUSED=0`: the wrapper's `predict_processed` with its read-back, then the ring's copies), alternating in one
process on one box. One JSON line per configuration:

  python tools/offpolicy_step_bench.py      # DQN on a CartPole-shaped env (4 observations, 2 actions) at 8 and 1 024
                                            # environments; TD3 on a 17 / 6 env at 1 environment

Both trainers of a configuration are built from the same seeds and differ in the environment variable only. A timed sample
is one whole `train_gen` call -- environment steps, action selection, the learner's `train` calls, the round's store into
the trainer's replay ring -- bracketed by synchronisations, divided by its environment steps. Each configuration is timed in
two phases: `warmup` (`learning_starts` beyond the run: random actions, no `train`, so the step has no other
synchronisation) and `learning` (greedy / policy actions with their read-back, `train` every `train_freq` steps). Warm-up
calls first, then `--samples` samples per side, interleaved; median and the 10th / 90th percentile are reported, and the
ratio of the medians. The run ends itself after `--limit` seconds.

Copies and synchronisations per step, from the code: the host path makes 4 uploads (`RewardNet.preprocess`), 1 read-back
with its synchronisation (`predict`) and 5 uploads (`_Table.write`); the fused path makes none of them (the launch reads the
step's pinned record) and records one event. Either path adds, in a greedy / policy step, the learner's own upload and
read-back of the action.
"""
import argparse
import json
import os
import signal
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 32   # environment steps per `train_gen` call (= the horizon: every round is one episode per environment)
CONFIGS = [dict(name="dqn_cartpole_8", algo="DQN", n_envs=8, od=4, ad=2),
           dict(name="dqn_cartpole_1024", algo="DQN", n_envs=1024, od=4, ad=2),
           dict(name="td3_17_6_1", algo="TD3", n_envs=1, od=17, ad=6)]
COUNTS = dict(host=dict(uploads=9, readbacks=1, synchronisations=1, launches=2),
              fused=dict(uploads=0, readbacks=0, synchronisations=0, launches=1))


def _stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)))


def make(cfg, fused: bool, learning: bool):
    import torch as th

    import imitation_amd as p
    os.environ["IA_OFFPOLICY_FUSED"] = "1" if fused else "0"
    n, od, ad = cfg["n_envs"], cfg["od"], cfg["ad"]
    discrete = cfg["algo"] == "DQN"
    venv = p.SyntheticVecEnv(num_envs=n, obs_dim=od, act_dim=ad, horizon=STEPS, seed=0, n_discrete=ad if discrete else None,
                             prefetch_noise=False)
    r = np.random.default_rng(0)
    n_demo = 1024
    acts = r.integers(0, ad, n_demo) if discrete else r.uniform(-1, 1, (n_demo, ad)).astype(np.float32)
    dones = np.zeros(n_demo, bool)
    dones[STEPS - 1::STEPS] = True
    demos = p.Transitions(obs=r.normal(size=(n_demo, od)).astype(np.float32), acts=acts,
                          next_obs=r.normal(size=(n_demo, od)).astype(np.float32), dones=dones)
    th.manual_seed(0)
    np.random.seed(0)
    venv.action_space.seed(0)
    starts = 0 if learning else 10 ** 9
    kw = dict(buffer_size=max(4096, 64 * n), learning_starts=starts, batch_size=32, train_freq=4, device="cuda")
    if discrete:
        rl = p.DQN("MlpPolicy", venv, exploration_fraction=0.01, **kw)
    else:
        rl = p.TD3("MlpPolicy", venv, gradient_steps=1, **kw)
    net = p.BasicRewardNet(venv.observation_space, venv.action_space, normalize_input_layer=p.RunningNorm)
    trainer = p.GAIL(demonstrations=demos, demo_batch_size=64, venv=venv, gen_algo=rl, reward_net=net,
                     gen_train_timesteps=STEPS * n, custom_logger=p.configure_logger(tempfile.mkdtemp(), []))
    assert (trainer._step_source is not None) == fused
    return trainer


def sample(trainer) -> float:
    import torch as th
    th.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.train_gen()
    th.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / STEPS


def bench(args):
    for cfg in CONFIGS:
        if args.only and cfg["name"] not in args.only:
            continue
        for phase in ("warmup", "learning"):
            sides = {side: make(cfg, side == "fused", phase == "learning") for side in ("fused", "host")}
            for _ in range(args.warmup):
                for tr in sides.values():
                    sample(tr)
            us = {side: [] for side in sides}
            for _ in range(args.samples):
                for side, tr in sides.items():
                    us[side].append(sample(tr))
            src = sides["fused"]._step_source
            out = dict(config=cfg["name"], phase=phase, n_envs=cfg["n_envs"], steps_per_sample=STEPS, samples=args.samples,
                       fused_us_per_step=_stats(us["fused"]), host_us_per_step=_stats(us["host"]),
                       host_over_fused=float(np.median(us["host"]) / np.median(us["fused"])),
                       in_kernel_reward=src.base is not None, slot_waits=src.event_waits, launches=src.launches,
                       host_reward_calls=sides["host"].venv_wrapped.reward_fn_calls, per_step=COUNTS)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("only", nargs="*")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (print(json.dumps(dict(error="time limit")), flush=True), os._exit(3)))
    signal.alarm(a.limit)
    bench(a)
