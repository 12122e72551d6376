"""`imitation_amd.mce_irl` on the device against the reference's own runs (`tests/golden/mce_*.npz`, written by
`make_golden_mce.py` from `imitation.algorithms.mce_irl` unmodified): the planning tables of `mce_partition_fh` /
`mce_occupancy_measures` on the true reward, and `MCEIRL.train` from the recorded initial parameters -- the same number
of iterations, logger keys and dump steps exactly, every logged value, the final parameters, Adam state, visitations and
policy within `TOL`."""
import os

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import data_types as dt
from imitation_amd import mce_irl
from tests.golden.make_golden_mce import CASES
from tests.test_mce_kernels_gpu import bound, restate_backup, restate_forward

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FINAL_BIAS = "mlp.dense_final.bias"

# Worst deviation of each quantity from the reference's recorded run over the three cases, measured once on an MI355X:
# max |x - golden| / max |golden| per array (float32 reward-net training over up to 60 Adam steps against torch on the
# CPU; the planning in between is float64 on both sides). The tests assert 3 x these.
#
# The output layer's bias is compared on its own. Its true gradient is zero -- sum_s (visitations - demo_state_om)[s] =
# (H + 1) - (H + 1), and adding a constant to the reward changes neither the policy nor the visitations -- so what
# reaches Adam is the rounding residue of a float32 sum (the goldens hold exp_avg ~ 1e-10, exp_avg_sq ~ 1e-19 there), and
# Adam's normalised step turns that residue into steps of up to lr: in the reference's own runs the bias wanders by
# 0.02 - 0.11. Its value is determined by summation order, not by the algorithm; `weight_norm`, which includes it,
# inherits that (its 7.6e-3 is the early-stop case, whose bias is a fifth of the norm). `final_bias` is
# |difference| / (lr * iterations). `params` is every other parameter: 7.8e-6, far below the 1e-3 that would mean a bug.
MEASURED = {
    "linf_delta": 6.553e-6, "weight_norm": 7.574e-3, "grad_norm": 1.174e-5, "params": 7.818e-6, "final_bias": 1.476e-1,
    "exp_avg": 1.000e-5, "exp_avg_sq": 1.760e-5, "visitations": 4.400e-7, "pi": 7.735e-6,
}
TOL = {k: 3.0 * v for k, v in MEASURED.items()}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not th.cuda.is_available():
        pytest.skip("no GPU")


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def env_of(g):
    return mce_irl.TabularEnv(transition_matrix=g["transition_matrix"], observation_matrix=g["observation_matrix"],
                              reward_matrix=g["reward_matrix"], horizon=int(g["horizon"]),
                              initial_state_dist=g["initial_state_dist"])


def rel(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    assert np.isfinite(x).all()
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("name", list(CASES))
def test_planning_tables_match_the_reference(name):
    g, cfg = golden(name), CASES[name]
    env = env_of(g)
    T, init, H, gamma = g["transition_matrix"], g["initial_state_dist"], cfg["H"], cfg["discount"]
    r32 = g["reward_matrix"].astype(np.float32)
    got = mce_irl.mce_partition_fh(env, discount=gamma)                    # reward defaults to env.reward_matrix
    ld = restate_backup(T, r32, H, gamma, np.longdouble)
    for key, x, z in zip(("true_V", "true_Q", "true_pi"), got, ld):
        assert x.dtype == np.float64
        err, tol = float(np.max(np.abs(x - g[key]))), bound(g[key], z)
        print(f"{name} {key}: err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (key, err, tol)
    # the default policy of mce_occupancy_measures is planned undiscounted (mce_irl.py:133), the sum over time discounted
    gotD = mce_irl.mce_occupancy_measures(env, reward=r32, discount=gamma)
    pi1_ld = restate_backup(T, r32, H, 1.0, np.longdouble)[2]
    ldD = restate_forward(T, pi1_ld, init, H, gamma, np.longdouble)
    for key, x, z in zip(("true_D", "true_Dcum"), gotD, ldD):
        err, tol = float(np.max(np.abs(x - g[key]))), bound(g[key], z)
        print(f"{name} {key}: err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (key, err, tol)
    # ... and a given policy is taken as it is
    gotD = mce_irl.mce_occupancy_measures(env, reward=r32, pi=g["true_pi"], discount=gamma)
    ldD = restate_forward(T, g["true_pi"], init, H, gamma, np.longdouble)
    for key, x, z in zip(("true_D_of_pi", "true_Dcum_of_pi"), gotD, ldD):
        err, tol = float(np.max(np.abs(x - g[key]))), bound(g[key], z)
        print(f"{name} {key}: err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (key, err, tol)


def _train(name):
    g, cfg = golden(name), CASES[name]
    env = env_of(g)
    net = p.BasicRewardNet(env.observation_space, env.action_space, use_action=False, hid_sizes=cfg["hid"]).to("cuda")
    net.load_state_dict({k[len("init/"):]: th.as_tensor(g[k]) for k in g.files if k.startswith("init/")})
    if cfg["demo"] == "om":
        demos = g["demo_state_om"]
    else:
        demos = [dt.TrajectoryWithRew(obs=s, acts=a, rews=np.zeros(len(a), np.float32), infos=None, terminal=True)
                 for s, a in zip(g["traj_states"], g["traj_acts"])]
    logger = p.configure_logger(format_strs=[])
    dumps, steps, orig_dump = [], [], logger.dump

    def dump(step=0):
        dumps.append({k: float(v) for k, v in logger.default_logger.name_to_value.items()})
        steps.append(int(step))
        orig_dump(step)

    logger.dump = dump
    algo = mce_irl.MCEIRL(demos, env, net, np.random.default_rng(cfg["seed"]), optimizer_kwargs={"lr": cfg["lr"]},
                          discount=cfg["discount"], linf_eps=cfg["linf_eps"], grad_l2_eps=cfg["grad_l2_eps"],
                          log_interval=1, custom_logger=logger)
    assert np.array_equal(algo.demo_state_om, g["demo_state_om"])
    assert (algo.policy.pi == 1.0 / cfg["A"]).all()
    visitations = algo.train(max_iter=cfg["max_iter"])
    return g, cfg, env, net, algo, dumps, steps, visitations


@pytest.mark.parametrize("name", list(CASES))
def test_train_matches_the_reference_run(name):
    g, cfg, env, net, algo, dumps, steps, visitations = _train(name)
    # exact: the iteration count, the logger's keys and the dump steps
    assert len(dumps) == int(g["n_iters"])
    assert steps == g["dump_steps"].tolist()
    keys = g["log_keys"].tolist()
    assert all(sorted(d) == keys for d in dumps)
    assert algo.optimizer.step_count == int(g["adam/step"]) == int(g["n_iters"])
    assert [d["iteration"] for d in dumps] == list(range(len(dumps)))

    dev = {}
    for k in ("linf_delta", "weight_norm", "grad_norm"):
        dev[k] = rel([d[k] for d in dumps], g["log_vals"][:, keys.index(k)])
    sd = net.state_dict()
    final = [k[len("final/"):] for k in g.files if k.startswith("final/")]
    assert sorted(sd) == sorted(final)
    rest = [k for k in final if k != FINAL_BIAS]
    dev["params"] = rel(np.concatenate([sd[k].cpu().numpy().reshape(-1) for k in rest]),
                        np.concatenate([g["final/" + k].reshape(-1) for k in rest]))
    # the output bias, in units of the farthest Adam's steps could have carried it (see FINAL_BIAS)
    dev["final_bias"] = float(abs(sd[FINAL_BIAS].item() - g["final/" + FINAL_BIAS].item()) / (cfg["lr"] * len(dumps)))
    dev["exp_avg"] = rel(algo.optimizer.exp_avg.cpu().numpy(), g["adam/exp_avg"])
    dev["exp_avg_sq"] = rel(algo.optimizer.exp_avg_sq.cpu().numpy(), g["adam/exp_avg_sq"])
    dev["visitations"] = rel(visitations, g["visitations"])
    dev["pi"] = rel(algo.policy.pi, g["final_pi"])
    for k, v in dev.items():
        print(f"{name} {k}: deviation {v:.3e} (asserted {TOL[k]:.3e})")
    for k, v in dev.items():
        assert v <= TOL[k], (k, v, TOL[k])

    # the returned visitations are mce_occupancy_measures of the last predicted reward: the same kernels on the same input
    assert visitations.dtype == np.float64 and algo._predicted_r_np.dtype == np.float32
    _, again = mce_irl.mce_occupancy_measures(env, reward=algo._predicted_r_np, discount=cfg["discount"])
    assert np.array_equal(visitations.view(np.int64), again.view(np.int64))
    _, _, pi = mce_irl.mce_partition_fh(env, reward=algo._predicted_r_np, discount=cfg["discount"])
    assert np.array_equal(algo.policy.pi.view(np.int64), pi.view(np.int64))


def test_train_resumes_and_repeats():
    """A second `train` call goes on from the first (Adam's step count, the cached device tables); two fresh runs agree
    bit for bit."""
    g, cfg, env, net, algo, dumps, _, vis = _train("mce_early_stop")
    _, _, _, net2, algo2, dumps2, _, vis2 = _train("mce_early_stop")
    assert dumps == dumps2 and np.array_equal(vis, vis2)
    assert th.equal(net._store.flat, net2._store.flat)
    planner = algo._dev["planner"]
    algo.train(max_iter=2)
    assert algo._dev["planner"] is planner and algo.optimizer.step_count == int(g["n_iters"]) + 1   # (stops at once)
