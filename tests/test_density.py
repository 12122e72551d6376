"""CPU tests of the density baseline's host layer (`imitation_amd/density.py`): flattening, the demonstration forms,
the reference's error paths, the scaler and the kernel normaliser against sklearn / the committed goldens."""
import glob
import os

import numpy as np
import pytest

from imitation_amd import data_types as dt
from imitation_amd import density as D
from imitation_amd import spaces as sp
from imitation_amd.vec_env import SyntheticVecEnv
from oracle import ref_shim

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _venv(discrete=False, obs_dim=3, act_dim=1):
    return SyntheticVecEnv(num_envs=2, obs_dim=obs_dim, act_dim=act_dim, n_discrete=2 if discrete else None, horizon=5)


def _algo(venv, demos, **kw):
    return D.DensityAlgorithm(demonstrations=demos, venv=venv, rng=np.random.default_rng(0), device="cpu", **kw)


def _trajs(n=3, T=5, obs_dim=3, act_dim=1, discrete=False, seed=0):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        acts = g.integers(0, 2, T) if discrete else g.uniform(-1, 1, (T, act_dim)).astype(np.float32)
        out.append(dt.TrajectoryWithRew(obs=g.standard_normal((T + 1, obs_dim)).astype(np.float32), acts=acts,
                                        rews=np.zeros(T), infos=None, terminal=True))
    return out


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"density_{name}.npz"), allow_pickle=False)


def _golden_demos(g):
    """The demonstrations a golden file was made from, as `imitation_amd` containers."""
    if "demo_obs" in g.files:
        return dt.Transitions(obs=g["demo_obs"], acts=g["demo_acts"], next_obs=g["demo_obs"],
                              dones=np.zeros(len(g["demo_obs"]), bool))
    trajs = dt.trajectories_from_legacy_npz(os.path.join(GOLDEN, "expert_rollouts", str(g["source"]) + ".npz"))
    return trajs[:int(g["n_demo_traj"])]


def _golden_venv(g):
    src = str(g["source"]) if "source" in g.files else ""
    if src == "cartpole_0":
        return SyntheticVecEnv(num_envs=1, obs_dim=4, n_discrete=2, horizon=500)
    if src == "pendulum_0":
        return SyntheticVecEnv(num_envs=1, obs_dim=3, act_dim=1, horizon=200)
    return SyntheticVecEnv(num_envs=1, obs_dim=17, act_dim=6, horizon=16)


GOLDEN_CASES = sorted(os.path.basename(p)[len("density_"):-4] for p in glob.glob(os.path.join(GOLDEN, "density_*.npz")))


def test_golden_files_present():
    assert len(GOLDEN_CASES) == 8, GOLDEN_CASES


@pytest.mark.parametrize("density_type", list(D.DensityType))
@pytest.mark.parametrize("discrete", [False, True])
def test_flatten_per_density_type_and_space(density_type, discrete):
    venv = _venv(discrete)
    algo = _algo(venv, None, density_type=density_type)
    obs = np.arange(6, dtype=np.float32).reshape(2, 3)
    nxt = obs + 10
    acts = np.array([1, 0]) if discrete else np.array([[0.5], [-0.25]], np.float32)
    got = algo._flat_batch(obs, acts, nxt)
    for i in range(2):   # row by row as the reference builds it (`density.py:266-293`)
        parts = [D.flatten(venv.observation_space, obs[i])]
        if density_type == D.DensityType.STATE_ACTION_DENSITY:
            parts.append(D.flatten(venv.action_space, acts[i]))
        elif density_type == D.DensityType.STATE_STATE_DENSITY:
            parts.append(D.flatten(venv.observation_space, nxt[i]))
        want = np.concatenate(parts)
        assert got[i].dtype == want.dtype and np.array_equal(got[i], want)
    if discrete and density_type == D.DensityType.STATE_ACTION_DENSITY:
        assert got.dtype == np.float64 and np.array_equal(got[:, 3:], [[0, 1], [1, 0]])
    with pytest.raises(NotImplementedError):
        D.flatten(sp.Space((2,), np.float32), np.zeros(2))
    with pytest.raises(NotImplementedError):
        algo._flat_batch({"a": obs}, acts, nxt)


def test_three_demonstration_forms():
    venv = _venv()
    trajs = _trajs()
    flat = dt.flatten_trajectories(trajs)
    ns = _algo(venv, trajs, is_stationary=False)
    assert list(ns.transitions) == [0, 1, 2, 3, 4]
    assert np.array_equal(ns.transitions[2][1], np.concatenate([trajs[1].obs[2], trajs[1].acts[2]]))
    st = _algo(venv, trajs)
    assert list(st.transitions) == [None]
    # stationary: the per-timestep groups concatenated in key order (`density.py:231-234`)
    assert np.array_equal(st.transitions[None], np.concatenate([ns.transitions[k] for k in range(5)]))
    tr = _algo(venv, dt.Transitions(obs=flat.obs, acts=flat.acts, next_obs=flat.next_obs, dones=flat.dones))
    assert list(tr.transitions) == [None] and len(tr.transitions[None]) == 15
    assert np.array_equal(tr.transitions[None], np.concatenate([flat.obs, flat.acts], axis=1))
    batches = [{"obs": flat.obs[:8], "acts": flat.acts[:8]}, {"obs": flat.obs[8:], "acts": flat.acts[8:]}]
    mp = _algo(venv, batches)
    # the reference `update`s the None key batch by batch: the last batch is what remains (`density.py:216-219`)
    assert np.array_equal(mp.transitions[None], tr.transitions[None][8:])
    ss = _algo(venv, [{"obs": flat.obs, "acts": flat.acts, "next_obs": flat.next_obs}],
               density_type=D.DensityType.STATE_STATE_DENSITY)
    assert np.array_equal(ss.transitions[None], np.concatenate([flat.obs, flat.next_obs], axis=1))


def test_reference_error_paths():
    venv = _venv()
    trajs = _trajs()
    flat = dt.flatten_trajectories(trajs)
    transitions = dt.Transitions(obs=flat.obs, acts=flat.acts, next_obs=flat.next_obs, dones=flat.dones)
    with pytest.raises(ValueError, match="Non-stationary model incompatible"):
        _algo(venv, transitions, is_stationary=False)
    with pytest.raises(ValueError, match="STATE_STATE_DENSITY requires next_obs_b"):
        _algo(venv, [{"obs": flat.obs, "acts": flat.acts}], density_type=D.DensityType.STATE_STATE_DENSITY)
    with pytest.raises(TypeError, match="Unsupported demonstration type"):
        _algo(venv, 42)
    with pytest.raises(TypeError, match="Unsupported demonstration type"):
        _algo(venv, [1, 2, 3])
    ns = _algo(venv, trajs, is_stationary=False)
    with pytest.raises(ValueError, match="steps must be provided with non-stationary models"):
        ns(flat.obs, flat.acts, flat.next_obs, flat.dones)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ns.train()


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_scaler_matches_goldens(case):
    g = _golden(case)
    algo = _algo(_golden_venv(g), _golden_demos(g), density_type=getattr(D.DensityType, str(g["density_type"])),
                 is_stationary=bool(g["is_stationary"]), standardise_inputs=bool(g["standardise"]))
    sc = D.StandardScaler(bool(g["standardise"])).fit(np.concatenate(list(algo.transitions.values())))
    np.testing.assert_allclose(sc.mean_, g["mean"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(sc.scale_, g["scale"], rtol=1e-12, atol=0)
    assert len(algo.transitions) == int(g["n_models"])


@pytest.mark.parametrize("case", [c for c in GOLDEN_CASES if not c.startswith("cartpole")])
def test_standardised_demo_rows_match_sklearn_bit_for_bit(case):
    preprocessing = pytest.importorskip("sklearn.preprocessing")
    g = _golden(case)
    algo = _algo(_golden_venv(g), _golden_demos(g), density_type=getattr(D.DensityType, str(g["density_type"])),
                 is_stationary=bool(g["is_stationary"]), standardise_inputs=bool(g["standardise"]))
    X = np.concatenate(list(algo.transitions.values()))
    assert X.dtype == np.float32   # Box spaces: float32 rows
    ours = D.StandardScaler(bool(g["standardise"])).fit(X)
    theirs = preprocessing.StandardScaler(with_mean=bool(g["standardise"]), with_std=bool(g["standardise"])).fit(X)
    for v in algo.transitions.values():
        a, b = ours.transform(v), theirs.transform(v)
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the kernel's prologue: (x - mean) then / scale, each in double, rounded to float32
    q = np.asarray(g["q_obs"], np.float32)
    if q.shape[1] == X.shape[1]:
        step = ((q.astype(np.float64) - ours.mean_).astype(np.float32).astype(np.float64) / ours.scale_).astype(np.float32)
        assert np.array_equal(step, theirs.transform(q))


def test_scaler_constant_feature_gets_scale_one():
    X = np.random.default_rng(0).standard_normal((50, 3)).astype(np.float32)
    X[:, 1] = 0.3
    sc = D.StandardScaler().fit(X)
    assert sc.scale_[1] == 1.0 and sc.scale_[0] != 1.0
    preprocessing = pytest.importorskip("sklearn.preprocessing")
    ref = preprocessing.StandardScaler().fit(X)
    np.testing.assert_allclose(sc.scale_, ref.scale_, rtol=1e-12, atol=0)
    np.testing.assert_allclose(sc.mean_, ref.mean_, rtol=1e-12, atol=0)


@pytest.mark.parametrize("kernel", D.KERNELS)
def test_kernel_normaliser_matches_sklearn(kernel):
    kd_tree = pytest.importorskip("sklearn.neighbors._kd_tree")
    for d in (1, 2, 3, 4, 7, 23, 34):
        for h in (0.2, 0.5, 1.7):
            want = kd_tree.kernel_norm(h, d, kernel, return_log=True)
            got = D.log_kernel_norm(h, d, kernel)
            if np.isnan(want):   # sklearn's cosine normaliser is NaN for some d (the reference's density with it)
                assert np.isnan(got), (kernel, d, h, got)
                continue
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (kernel, d, h, got, want)
    with pytest.raises(ValueError):
        D.log_kernel_norm(0.5, 3, "triangle")


@pytest.mark.reference
@pytest.mark.skipif(not ref_shim.reference_available(), reason="/root/reference not present")
def test_golden_reproduces_under_reference():
    """The reference's own DensityAlgorithm, run again, gives the committed rewards of one golden case."""
    pytest.importorskip("sklearn")
    from tests.golden import make_golden_density as mk
    density, types = mk.install()
    g = _golden("pendulum_state_density_nonstationary")
    demo, _ = mk.split_rollouts("pendulum_0")
    algo = density.DensityAlgorithm(demonstrations=mk.ref_trajs(types, demo), venv=_golden_venv(g),
                                    rng=np.random.default_rng(0), density_type=density.DensityType.STATE_DENSITY,
                                    kernel="gaussian", kernel_bandwidth=float(g["bandwidth"]), is_stationary=False)
    algo.train()
    rew = algo(g["q_obs"], g["q_acts"], g["q_next"], np.zeros(len(g["q_obs"]), bool), g["q_steps"])
    assert np.array_equal(rew, g["rew_gaussian"])
