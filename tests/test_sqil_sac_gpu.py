"""`SQIL.train` on the SAC learner end to end on the device against the fixtures the reference's own SQIL produced over the
restated SAC (`tests/golden/make_golden_sqil_sac.py`; SB3 itself is installed nowhere: parity unpinned). Exactly: branches,
ring positions, every sampled index, the `eps` tensors of the gradient steps and of the environment steps, which critic
attained each minimum, both generators' post-states, counters, logger keys and dump steps, the initial parameters. Floating
quantities (actions, ring contents, losses, alphas, final parameters, `log_ent_coef`, Adam's moments; parameters and moments
thinned as in the fixture) by relative L2 against the float64 run within `8 x dref`, dref = the deviation of the reference's
float32 run from its float64 run, per key; a key whose dref is 0 within float32 epsilon of its magnitude."""
import json
import os

import numpy as np
import pytest

from tests import sac_golden as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("ring_pos", "ring_done", "sample_rows", "eps", "act_eps", "argmin", "branches", "train_n_updates", "train_lr",
         "n_dumps", "numpy_rng_keys", "numpy_rng_pos", "torch_rng_state")
EPS32 = float(np.finfo(np.float32).eps)


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("name", list(sg.CASES))
def test_sqil_train_on_sac_matches_the_reference_run(name):
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    assert float(g["min_q_gap"]) >= 100 * float(g["q_dev"]) > 0   # no near tie between the critics in the recorded run
    got = sg.run_case(name, cfg["seed"])
    n_envs, B = cfg["n_envs"], cfg["batch_size"]
    want = {k: g[k] for k in EXACT if k != "sample_rows"}
    want["sample_rows"] = np.concatenate([g["sample_new_pos"] * n_envs + g["sample_new_env"],
                                          g["sample_expert_pos"] + g["sample_expert_env"]], axis=1)
    assert want["sample_rows"].shape[1] == B and len(g["train_lr"]) > 0 and len(g["act_eps"]) > 0
    for k in EXACT:
        assert np.array_equal(np.asarray(got[k]), want[k]), k
    assert (g["argmin"] == 0).any() and (g["argmin"] == 1).any()
    assert not g["ring_reward"].any() and not got["table_reward"].any()
    learned = isinstance(cfg["ent_coef"], str)
    assert ("ent_coef_loss" in got) == learned == ("f64/ent_coef_loss" in g.files)
    for k in g.files:
        if k.startswith("counter/"):
            assert int(got[k]) == int(g[k]), k
        if k.startswith("init/"):
            assert np.array_equal(got[k], g[k]), k
    for j in range(int(g["n_dumps"])):
        assert int(got[f"dump{j}_step"]) == int(g[f"dump{j}_step"])
        keys = [str(k) for k in g[f"dump{j}_keys"]]
        assert [str(k) for k in got[f"dump{j}_keys"]] == keys
        assert ("train/ent_coef_loss" in keys) == (learned and "train/ent_coef" in keys)
        for k, a, b in zip(keys, got[f"dump{j}_vals"], g[f"dump{j}_vals64"]):
            if k in sg.LOSS_KEYS:   # the mean over the call's steps
                dref = float(g["dref/" + k[len("train/"):]])
                assert abs(a - b) <= (8 * dref if dref > 0 else EPS32) * abs(b), (j, k, a, b)
            elif k not in sg.NOT_COMPARED:
                assert a == b, (j, k, a, b)
    # the ring in device memory is what the writes left behind
    A = cfg["act_dim"]
    ring = np.zeros_like(got["table_action"])
    for i, pos in enumerate(g["ring_pos"]):
        ring[pos * n_envs:(pos + 1) * n_envs] = got["ring_action"][i].reshape(n_envs, A)
    assert np.array_equal(got["table_action"], ring) and np.abs(ring).max() <= 1.0
    worst = []
    for k in (f[len("dref/"):] for f in g.files if f.startswith("dref/")):
        dref, f64 = float(g[f"dref/{k}"]), g[f"f64/{k}"]
        assert np.shape(got[k]) == f64.shape, k
        dev = rel(got[k], f64)
        bound = 8 * dref if dref > 0 else EPS32
        print(f"{name} {k}: dref {dref:.3e}, device {dev:.3e} ({dev / bound * 8:.2f} x)")
        if not dev <= bound:
            worst.append((k, dev, dref))
    assert not worst, worst
