"""DAgger host logic (`imitation_amd.dagger`): beta schedules, the interactive collector's draws and records, the
scratch-directory contract and the device table's row map. Nothing here needs a GPU: the BC trainer is a stand-in that
records what it is handed, the robot is a stub. Expected values restate the reference's definitions
(`algorithms/dagger.py`): `mask = rng.uniform(0, 1, n) > beta` once per step, the robot asked on the masked rows only,
`uuid.UUID(int=int.from_bytes(rng.bytes(16), "big"), version=4).hex` per saved file, files loaded in sorted name order."""
import os
import uuid

import numpy as np
import pytest

from imitation_amd import dagger, serialize
from imitation_amd import data_types as dt
from imitation_amd import spaces
from imitation_amd.vec_env import CountingVecEnv


def test_exported_from_package():
    import imitation_amd

    assert imitation_amd.dagger is dagger
    assert imitation_amd.SimpleDAggerTrainer is dagger.SimpleDAggerTrainer


def test_beta_schedules():
    lin = dagger.LinearBetaSchedule(4)
    assert [lin(i) for i in range(7)] == [1, 0.75, 0.5, 0.25, 0, 0, 0]
    exp = dagger.ExponentialBetaSchedule(0.5)
    assert [exp(i) for i in range(4)] == [1.0, 0.5, 0.25, 0.125]
    assert dagger.ExponentialBetaSchedule(1)(9) == 1
    assert isinstance(lin, dagger.BetaSchedule) and isinstance(exp, dagger.BetaSchedule)
    for bad in (0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r"decay_probability lies outside the range \(0, 1\]\."):
            dagger.ExponentialBetaSchedule(bad)
    with pytest.raises(AssertionError):
        lin(-1)
    with pytest.raises(AssertionError):
        exp(-1)


def _collect(tmp_path, beta, seed, lengths=(3, 5, 2), steps=11):
    """Runs the collector with a stub robot -> (records, mirror of the generator's draws)."""
    venv = CountingVecEnv(lengths, obs_dim=2, act_dim=1)
    calls = []

    def robot(obs):
        calls.append(np.array(obs))
        return -np.ones((len(obs), 1), np.float32)

    col = dagger.InteractiveTrajectoryCollector(venv, robot, beta, tmp_path, np.random.default_rng(seed))
    executed = []
    orig = venv.step_async
    venv.step_async = lambda a: (executed.append(np.array(a)), orig(a))[1]
    mirror = np.random.default_rng(seed)
    obs = col.reset()
    exp_masks, exp_names, given, obs_seen = [], [], [], []
    t = np.zeros(len(lengths), np.int64)
    for s in range(steps):
        acts = np.full((len(lengths), 1), float(s), np.float32)
        given.append(acts)
        obs_seen.append(np.array(obs))
        exp_masks.append(mirror.uniform(0, 1, size=(len(lengths),)) > beta)
        obs, _, dones, _ = col.step(acts)
        t += 1
        for k, i in enumerate(np.flatnonzero(t >= np.asarray(lengths))):
            exp_names.append(f"dagger-demo-{k}-{uuid.UUID(int=int.from_bytes(mirror.bytes(16), 'big'), version=4).hex}.npz")
        t[t >= np.asarray(lengths)] = 0
    return dict(calls=calls, executed=executed, masks=exp_masks, names=exp_names, given=given, obs=obs_seen)


@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0])
def test_collector_masks_robot_rows_files(tmp_path, beta):
    r = _collect(tmp_path, beta, seed=5)
    calls = iter(r["calls"])
    n_calls = 0
    for mask, given, executed, obs in zip(r["masks"], r["given"], r["executed"], r["obs"]):
        want = np.array(given)
        if mask.any():                      # the robot sees the masked rows only, and only when there are any
            np.testing.assert_array_equal(next(calls), obs[mask])
            n_calls += 1
            want[mask] = -1.0
        np.testing.assert_array_equal(executed, want)
    assert n_calls == len(r["calls"])
    if beta == 1.0:
        assert n_calls == 0
    if beta == 0.0:
        assert n_calls == len(r["masks"])
    assert sorted(os.listdir(tmp_path)) == sorted(r["names"])
    # stored actions are the ones passed to `step`, whichever was executed: env 2 has length 2 -> steps (0, 1), (2, 3), ...
    first = [n for n in r["names"] if n.startswith("dagger-demo-0-")][0]   # step index 1: only env 2 finished
    traj = serialize.load(tmp_path / r["names"][0])[0]
    assert first == r["names"][0]
    np.testing.assert_array_equal(np.asarray(traj.acts).reshape(-1), [0.0, 1.0])
    np.testing.assert_array_equal(np.asarray(traj.obs)[:, 0], [0.0, 1.0, 2.0])
    np.testing.assert_array_equal(np.asarray(traj.rews), [10.0, 20.0])
    assert traj.terminal


def test_collector_needs_reset_and_seed(tmp_path):
    venv = CountingVecEnv((2, 2))
    col = dagger.InteractiveTrajectoryCollector(venv, lambda o: o, 0.5, tmp_path, np.random.default_rng(0))
    with pytest.raises(AssertionError, match=r"call \.reset\(\) before \.step\(\)"):
        col.step_async(np.zeros((2, 1), np.float32))
    with pytest.raises(AssertionError):
        dagger.InteractiveTrajectoryCollector(venv, lambda o: o, 1.5, tmp_path, np.random.default_rng(0))
    assert col.seed(3) == [3, 3]
    assert col.rng.uniform() == np.random.default_rng(3).uniform()


class _StubPolicy:
    discrete, obs_dim, act_dim = False, 2, 1


class _StubBC:
    """What `DAggerTrainer` touches of `bc.BC` (no `set_demonstrations_device`: every round hands over everything)."""

    def __init__(self, batch_size=4):
        self.observation_space = spaces.Box(-np.inf, np.inf, (2,), np.float32)
        self.action_space = spaces.Box(-np.inf, np.inf, (1,), np.float32)
        self.batch_size, self.logger, self.policy = batch_size, None, _StubPolicy()
        self.demos, self.train_calls = [], []

    def set_demonstrations(self, d):
        self.demos.append(d)

    def train(self, **kw):
        self.train_calls.append(kw)


def _traj(k, tag):
    obs = np.full((k + 1, 2), tag, np.float32) + np.arange(k + 1, dtype=np.float32)[:, None] / 100
    return dt.TrajectoryWithRew(obs=obs, acts=np.full((k, 1), tag, np.float32), rews=np.zeros(k, np.float32), infos=None,
                                terminal=True)


def test_scratch_dir_contract(tmp_path):
    venv = CountingVecEnv((3, 3), obs_dim=2)
    bc = _StubBC()
    tr = dagger.DAggerTrainer(venv=venv, scratch_dir=tmp_path, rng=np.random.default_rng(0), bc_trainer=bc)
    assert tr.round_num == 0 and tr.batch_size == 4 and tr.policy is bc.policy and bc.logger is tr.logger
    assert isinstance(tr.beta_schedule, dagger.LinearBetaSchedule) and tr.beta_schedule.rampdown_rounds == 15
    assert tr.DEFAULT_N_EPOCHS == 4
    with pytest.raises(dagger.NeedsDemosException, match="No demos found for round 0 in dir"):
        tr.extend_and_update()
    assert tr.round_num == 0
    d0 = tmp_path / "demos" / "round-000"
    assert tr._demo_dir_path_for_round() == d0.resolve()
    os.makedirs(d0)
    serialize.save(d0 / "b.npz", [_traj(2, 1.0)])
    with pytest.raises(ValueError, match=r"Not enough transitions to form a single batch: self\.batch_size=4 > "
                                         r"len\(transitions\)=2"):
        tr.extend_and_update()
    # sorted load order, whatever order the files were written in
    tr = dagger.DAggerTrainer(venv=venv, scratch_dir=tmp_path, rng=np.random.default_rng(0), bc_trainer=bc)
    serialize.save(d0 / "a.npz", [_traj(3, 2.0)])
    serialize.save(d0 / "ignored.txt", [_traj(3, 9.0)])
    assert tr.extend_and_update(dict(n_batches=7)) == 1
    np.testing.assert_array_equal(bc.demos[-1].acts.reshape(-1), [2, 2, 2, 1, 1])
    assert bc.train_calls[-1] == dict(n_batches=7, log_rollouts_venv=venv)
    # the next round needs its own demonstrations; with them, earlier rounds stay in front
    with pytest.raises(dagger.NeedsDemosException):
        tr.extend_and_update()
    col = tr.create_trajectory_collector()
    assert col.beta == tr.beta_schedule(1) and col.save_dir == (tmp_path / "demos" / "round-001").resolve()
    os.makedirs(col.save_dir)
    serialize.save(col.save_dir / "z.npz", [_traj(1, 3.0)])
    assert tr.extend_and_update() == 2
    np.testing.assert_array_equal(bc.demos[-1].acts.reshape(-1), [2, 2, 2, 1, 1, 3])
    assert bc.train_calls[-1] == dict(n_epochs=4, log_rollouts_venv=venv)
    # the logger setter keeps the inner trainer in sync
    tr.logger = "other"
    assert bc.logger == "other"


def test_space_checks_and_initial_data(tmp_path):
    venv = CountingVecEnv((3, 3), obs_dim=2)
    bc = _StubBC()
    bad = _StubBC()
    bad.observation_space = spaces.Box(-np.inf, np.inf, (3,), np.float32)
    with pytest.raises(ValueError, match="Observation spaces do not match"):
        dagger.DAggerTrainer(venv=venv, scratch_dir=tmp_path, rng=np.random.default_rng(0), bc_trainer=bad)

    class Expert:
        def __init__(self, o, a):
            self.observation_space, self.action_space = o, a

    with pytest.raises(ValueError, match="Mismatched observation space between expert_policy and venv"):
        dagger.SimpleDAggerTrainer(venv=venv, scratch_dir=tmp_path, rng=np.random.default_rng(0), bc_trainer=bc,
                                   expert_policy=Expert(bad.observation_space, bc.action_space))
    with pytest.raises(ValueError, match="Mismatched action space between expert_policy and venv"):
        dagger.SimpleDAggerTrainer(venv=venv, scratch_dir=tmp_path, rng=np.random.default_rng(0), bc_trainer=bc,
                                   expert_policy=Expert(bc.observation_space, spaces.Discrete(2)))
    mirror = np.random.default_rng(4)
    tr = dagger.SimpleDAggerTrainer(venv=venv, scratch_dir=tmp_path, rng=np.random.default_rng(4), bc_trainer=bc,
                                    expert_policy=Expert(bc.observation_space, bc.action_space),
                                    expert_trajs=[_traj(2, 1.0), _traj(3, 2.0)])
    want = [f"initial_data-dagger-demo-{i}-{uuid.UUID(int=int.from_bytes(mirror.bytes(16), 'big'), version=4).hex}.npz"
            for i in range(2)]
    assert sorted(os.listdir(tmp_path / "demos" / "round-000")) == sorted(want)
    assert tr.extend_and_update() == 1 and len(bc.demos[-1].acts) == 5


def test_row_map_of_appended_steps():
    """Three environments, one block of three rows appended per step (row = base + env). Env 0 finishes after steps
    {0, 1} and again after {2, 3, 4}; env 1 after {0, 1, 2, 3}; env 2 never. File names sort differently from the order
    the episodes ended in; rows of the unfinished episodes (env 2, env 1's step 4) appear nowhere."""
    tracker = dagger.EpisodeRowTracker(3)
    files = {}
    ends = {1: [(0, "m.npz")], 3: [(1, "a.npz")], 4: [(0, "z.npz")]}
    for step in range(5):
        tracker.step(100 + 3 * step)       # the table already held 100 rows
        for env, name in ends.get(step, []):
            files[name] = tracker.finish(env)
    row_map = dagger.build_row_map(list(files), files)
    want = [100 + 1, 103 + 1, 106 + 1, 109 + 1,          # a.npz: env 1, steps 0..3
            100, 103,                                    # m.npz: env 0, steps 0..1
            106, 109, 112]                               # z.npz: env 0, steps 2..4
    np.testing.assert_array_equal(row_map, want)
    assert row_map.dtype == np.int64
    assert len(set(row_map.tolist())) == len(row_map)
    assert not set(row_map.tolist()) & {102, 105, 108, 111, 114, 113}


# ---- against the records of the reference's own run (tests/golden/dagger_*.npz) -----------------------------------
from imitation_amd import logger as imit_logger  # noqa: E402
from tests import dagger_golden as G  # noqa: E402


def test_beta_schedule_against_fixture():
    for name in G.CASES:
        z, cfg = G.load(name)
        sched = dagger.LinearBetaSchedule(cfg["rampdown"])
        assert [sched(r) for r in range(int(z["n_rounds"]))] == [float(z[f"r{r}_beta"]) for r in range(int(z["n_rounds"]))]


@pytest.mark.parametrize("name", G.CASES)
def test_collection_replays_reference_records(tmp_path, name):
    """`SimpleDAggerTrainer.train` with the recorded labels as the expert and a stub learner that returns the recorded
    executed actions: every mask, the rows the robot is asked on (and no call on an empty mask), the order of the draws,
    the file names, the saved trajectories and the `dagger/*` records equal the reference's run."""
    z, cfg = G.load(name)
    venv = G.gold.make_env(cfg)
    state = dict(t=0, r=-1, steps=[], robot_calls=0)

    def expert(obs, states, dones):
        if trainer.round_num != state["r"]:
            state.update(r=trainer.round_num, t=0)
            state["steps"].append(0)
        r, t = state["r"], state["t"]
        np.testing.assert_array_equal(obs, z[f"r{r}_obs"][t])     # (the environment saw the recorded executed actions)
        state["t"] += 1
        state["steps"][-1] += 1
        return z[f"r{r}_labels"][t].copy(), states

    class Learner:
        discrete, obs_dim, act_dim = cfg["discrete"], cfg["obs_dim"], cfg["act_dim"]

        def predict(self, obs):
            r, t = state["r"], state["t"] - 1
            mask = z[f"r{r}_masks"][t]
            assert mask.any()
            np.testing.assert_array_equal(obs, z[f"r{r}_obs"][t][mask])
            state["robot_calls"] += 1
            return z[f"r{r}_executed"][t][mask], None

    class StubBC(_StubBC):
        def train(self, **kw):
            self.logger.dump(0)

    bc = StubBC(cfg["batch_size"])
    bc.observation_space, bc.action_space, bc.policy = venv.observation_space, venv.action_space, Learner()
    log = imit_logger.configure(str(tmp_path / "log"), ["log"])
    dumps = G.dump_recorder(log)
    rng = G.RecordingRng(np.random.default_rng(cfg["seed"] + 1))
    trainer = dagger.SimpleDAggerTrainer(venv=venv, scratch_dir=tmp_path / "scratch", expert_policy=expert, rng=rng,
                                         expert_trajs=G.initial_trajs(z), bc_trainer=bc, custom_logger=log,
                                         beta_schedule=dagger.LinearBetaSchedule(cfg["rampdown"]))
    trainer.train(cfg["total_timesteps"], **G.train_kwargs(cfg))
    masks, k = [], 0
    for r, n_steps in enumerate(state["steps"]):
        masks.append([u > float(z[f"r{r}_beta"]) for u in rng.uniforms[k:k + n_steps]])
        k += n_steps
    assert k == len(rng.uniforms)
    G.check_host_records(z, cfg, trainer, rng, dumps, masks)
    assert state["robot_calls"] == sum(int(z[f"r{r}_masks"].any(axis=1).sum()) for r in range(int(z["n_rounds"])))
    for r in range(int(z["n_rounds"])):
        for i, f in enumerate(z[f"r{r}_files"]):
            traj = serialize.load(trainer._demo_dir_path_for_round(r) / str(f))[0]
            np.testing.assert_array_equal(np.asarray(traj.obs, np.float32), z[f"r{r}_traj{i}_obs"])
            np.testing.assert_array_equal(np.asarray(traj.acts), z[f"r{r}_traj{i}_acts"])
            np.testing.assert_array_equal(np.asarray(traj.rews, np.float32), z[f"r{r}_traj{i}_rews"])


@pytest.mark.reference
def test_golden_script_reproduces_committed_fixture(tmp_path):
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("reference sources not present")
    name = "dagger_box32"
    m = G.gold.install()
    G.gold.run_case(name, G.gold.CASES[name], m, str(tmp_path), out_dir=str(tmp_path))
    z, _ = G.load(name)
    live = np.load(tmp_path / (name + ".npz"))
    assert sorted(live.files) == sorted(z.files)
    for k in z.files:
        np.testing.assert_array_equal(live[k], z[k], err_msg=k)


def test_fused_collector_with_other_actions_draws_nothing_twice(tmp_path):
    """`step_async` after `expert_actions` with actions that are not the expert's: the step's mask and the robot's
    actions are the ones already drawn (one `uniform` per step, the robot is not asked again), the given actions are what
    is stored, and no table rows are claimed for the files."""
    venv = CountingVecEnv((2, 2), obs_dim=2, act_dim=1)

    class Step:
        table = object()

        def __call__(self, obs, mask):
            return np.zeros((2, 1), np.float32), np.where(mask[:, None], -1.0, 0.0).astype(np.float32), 10

    noted = []
    rng = G.RecordingRng(np.random.default_rng(2))
    col = dagger._FusedCollector(venv=venv, get_robot_acts=lambda o: 1 / 0, beta=0.5, save_dir=tmp_path, rng=rng,
                                 fused_step=Step(), on_file=lambda p, rows: noted.append(rows))
    executed = []
    orig = venv.step_async
    venv.step_async = lambda a: (executed.append(np.array(a)), orig(a))[1]
    obs = col.reset()
    for t in range(2):
        col.expert_actions(obs)
        given = np.full((2, 1), 5.0 + t, np.float32)
        obs, _, _, _ = col.step(given)
        mask = rng.uniforms[-1] > 0.5
        np.testing.assert_array_equal(executed[-1], np.where(mask[:, None], -1.0, 5.0 + t))
    assert rng.kinds.count("uniform") == 2 and not noted
    files = sorted(os.listdir(tmp_path))
    assert len(files) == 2
    np.testing.assert_array_equal(np.asarray(serialize.load(tmp_path / files[0])[0].acts).reshape(-1), [5.0, 6.0])
