"""DAgger collection and dataset hand-over (`imitation_amd/dagger.py`, `csrc/dagger.hip`). One JSON line per measurement.

  python tools/dagger_bench.py step     # environment-free collection step at 8 / 256 / 1 024 environments: the fused
                                        # launch against two `predict` calls (expert deterministic on all rows, learner
                                        # sampled on the masked rows), alternating in one process; steps per second
  python tools/dagger_bench.py round    # one `extend_and_update` hand-over + BC epoch per round over a growing dataset:
                                        # device-resident table against re-upload through `set_demonstrations`

Warm-up first, then `--samples` samples of `--steps` steps each per side, interleaved (`round`: `--reps` whole passes per
side in alternating order after a warm-up pass of each); median and the 10th / 90th percentile are reported. The whole run ends itself after `--limit` seconds.
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

D, A = 17, 6   # BASELINE config P


def _stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)))


def _policies(hidden=32):
    import torch as th
    from imitation_amd import spaces
    from imitation_amd.policies import ActorCriticPolicy
    osp = spaces.Box(-np.inf, np.inf, (D,), np.float32)
    asp = spaces.Box(-1.0, 1.0, (A,), np.float32)
    th.manual_seed(0)
    mk = lambda: ActorCriticPolicy(osp, asp, lambda _: 1e-3, net_arch=[hidden, hidden]).to("cuda")
    return mk(), mk()


def step(args):
    import torch as th
    from imitation_amd import dagger
    expert, learner = _policies()
    rng = np.random.default_rng(0)
    for n in (8, 256, 1024):
        obs = rng.normal(size=(n, D)).astype(np.float32)
        masks = [rng.uniform(size=n) > 0.5 for _ in range(args.steps)]
        fused = dagger._FusedStep(expert, learner, n, None)

        def run_fused():
            for m in masks:
                fused(obs, m)

        def run_predict():
            for m in masks:
                acts = expert.predict(obs, deterministic=True)[0]
                actual = np.array(acts)
                if m.any():
                    actual[m] = learner.predict(obs[m])[0]

        for f in (run_fused, run_predict):
            f()                                      # warm-up (first launches, pinned buffers, allocator)
        t = {"fused": [], "two_predict": []}
        for _ in range(args.samples):
            for name, f in (("fused", run_fused), ("two_predict", run_predict)):
                th.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                t[name].append(args.steps / (time.perf_counter() - t0))
        print(json.dumps(dict(bench="dagger_step", n_envs=n, steps_per_sample=args.steps, samples=args.samples,
                              fused_steps_per_s=_stats(t["fused"]), two_predict_steps_per_s=_stats(t["two_predict"]),
                              speedup_of_medians=float(np.median(t["fused"]) / np.median(t["two_predict"])))), flush=True)


def round_(args):
    import torch as th
    from imitation_amd import bc, dagger, spaces
    from imitation_amd import data_types as dt
    from imitation_amd import logger as imit_logger
    osp = spaces.Box(-np.inf, np.inf, (D,), np.float32)
    asp = spaces.Box(-1.0, 1.0, (A,), np.float32)
    per_round, horizon = 64, 1000      # 64 000 transitions gathered per round

    def one_pass(mode, rounds):
        """-> seconds of the hand-over + BC's first batch, per round. Resident: the new rows are already in the table when
        the clock starts -- the fused step appended them while the environments were stepping (rows that come from files
        instead are uploaded inside `extend_and_update` and would count); re-upload: flatten + upload of everything."""
        rng = np.random.default_rng(0)
        th.manual_seed(0)
        log = imit_logger.configure(tempfile.mkdtemp(), ["log"])
        trainer = bc.BC(observation_space=osp, action_space=asp, rng=np.random.default_rng(0), batch_size=1024,
                        custom_logger=log)
        table = dagger.DeviceDemoTable(D, A, "cuda")
        demos, out = [], []
        for r in range(rounds):
            new = [dt.TrajectoryWithRew(obs=rng.normal(size=(horizon + 1, D)).astype(np.float32),
                                        acts=rng.uniform(-1, 1, size=(horizon, A)).astype(np.float32),
                                        rews=np.zeros(horizon, np.float32), infos=None, terminal=True)
                   for _ in range(per_round)]
            demos += new
            if mode == "resident":
                rows = [table.upload(t) for t in new]
            th.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "resident":
                for x in rows:
                    table.extend_map(x)
                trainer.set_demonstrations_device(table.obs, table.acts, table.row_map)
            else:
                trainer.set_demonstrations(dt.flatten_trajectories(demos))
            trainer.train(n_batches=1, log_interval=10 ** 9)     # first batch: the upload happens here
            th.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out

    for mode in ("resident", "reupload"):
        one_pass(mode, 2)                                        # warm-up: first launches, allocator, pinned staging
    res = {"resident": [], "reupload": []}
    for rep in range(args.reps):
        for mode in (("resident", "reupload") if rep % 2 == 0 else ("reupload", "resident")):
            res[mode].append(one_pass(mode, args.rounds))
    for r in range(args.rounds):
        print(json.dumps(dict(bench="dagger_round_handover", round=r, transitions=(r + 1) * per_round * horizon,
                              reps=args.reps, resident_ms=_stats([1e3 * x[r] for x in res["resident"]]),
                              reupload_ms=_stats([1e3 * x[r] for x in res["reupload"]]))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "round"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240)
    a = ap.parse_args()
    signal.alarm(a.limit)
    {"step": step, "round": round_}[a.what](a)
