"""Helpers of the DAgger tests: the fixtures recorded from the reference (`tests/golden/dagger_*.npz`, written by
`tests/golden/make_golden_dagger.py`) and a run of this package's `SimpleDAggerTrainer` on a fixture's case."""
import importlib.util
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_dagger", os.path.join(HERE, "golden", "make_golden_dagger.py"))
gold = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gold)     # (settings, environment and the callable expert of the cases; imports no reference)

CASES = list(gold.CASES)


def load(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    return z, json.loads(str(z["cfg"]))


def group(z, prefix):
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


class RecordingRng(gold.RecordingRng):
    pass


def dump_recorder(logger):
    """Every `dump` of `logger` -> a dict of its records, appended to the returned list."""
    dumps = []
    orig = logger.dump

    def dump(step=0):
        dumps.append({k: float(v) for k, v in logger.default_logger.name_to_value.items()})
        orig(step)

    logger.dump = dump
    return dumps


def train_kwargs(cfg):
    return dict(rollout_round_min_episodes=cfg["min_episodes"], rollout_round_min_timesteps=cfg["min_timesteps"],
                bc_train_kwargs=dict(n_epochs=cfg["n_epochs"], log_rollouts_venv=None))


def initial_trajs(z):
    from imitation_amd import data_types as dt
    out, i = [], 0
    while f"init{i}_obs" in z.files:
        out.append(dt.TrajectoryWithRew(obs=z[f"init{i}_obs"], acts=z[f"init{i}_acts"], rews=z[f"init{i}_rews"], infos=None,
                                        terminal=True))
        i += 1
    return out or None


def check_host_records(z, cfg, trainer, rng, dumps, masks_by_round):
    """What must equal the reference exactly: rounds, betas, masks, files, draw order, `dagger/*` records."""
    n_rounds = int(z["n_rounds"])
    assert trainer.round_num == n_rounds and len(masks_by_round) == n_rounds
    assert list(rng.kinds) == list(z["draw_kinds"])
    assert len(dumps) == sum(int(z[f"r{r}_n_dumps"]) for r in range(n_rounds))
    j = 0
    for r in range(n_rounds):
        assert trainer.beta_schedule(r) == float(z[f"r{r}_beta"])
        np.testing.assert_array_equal(np.asarray(masks_by_round[r]), z[f"r{r}_masks"])
        files = sorted(f for f in os.listdir(trainer._demo_dir_path_for_round(r)) if f.endswith(".npz"))
        assert files == list(z[f"r{r}_files"])
        for d in range(int(z[f"r{r}_n_dumps"])):
            want = dict(zip(z[f"r{r}_dump{d}_keys"], z[f"r{r}_dump{d}_vals"]))
            got = dumps[j]
            j += 1
            assert {k for k in got if k.startswith("dagger/")} == {k for k in want if k.startswith("dagger/")}
            for k, v in want.items():
                if k.startswith("dagger/"):
                    assert got[k] == v, (r, k, got[k], v)
