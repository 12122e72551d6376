"""Host logic of `imitation_amd.preference_comparisons` (no GPU): query schedule, fragment picks and synthetic
preferences against the reference's goldens (`tests/golden/preference_*.npz`, made by `make_golden_preferences.py`),
the dataset FIFO, constructor errors, out-of-scope components and the DataLoader shuffle draws."""
import json
import os

import numpy as np
import pytest
import torch as th

from imitation_amd import data_types as dt
from imitation_amd import preference_comparisons as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["preference_basic_rn", "preference_plain_disc_noise_accum", "preference_normalized_queue",
         "preference_discrete", "preference_default_sizes"]


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    trajs = []
    for k in range(cfg["n_traj"]):
        trajs.append(dt.TrajectoryWithRew(obs=z[f"traj{k}_obs"], acts=z[f"traj{k}_acts"], rews=z[f"traj{k}_rews"],
                                          infos=None, terminal=True))
    return z, cfg, trajs


class _Stub:
    """A reward-trainer stand-in: the host-side pipeline only (the reward trainer never draws from the numpy rng)."""
    logger = None


@pytest.mark.parametrize("name", CASES)
def test_schedule_picks_and_preferences_match_reference(name):
    z, cfg, trajs = load_case(name)
    rng = np.random.default_rng(cfg["seed"])
    gen = pc.TrajectoryDataset(trajs, rng=rng)
    frag = pc.RandomFragmenter(rng=rng)
    gath = pc.SyntheticGatherer(rng=rng, discount_factor=cfg["gamma"])
    algo = pc.PreferenceComparisons(gen, None, num_iterations=cfg["iters"], fragmenter=frag, preference_gatherer=gath,
                                    reward_trainer=_Stub(), fragment_length=cfg["frag"],
                                    initial_epoch_multiplier=cfg["init_mult"])
    schedule = algo.query_schedule_for(cfg["comparisons"])
    np.testing.assert_array_equal(schedule, z["schedule"])
    by_id = {id(t.obs): k for k, t in enumerate(trajs)}
    for i, num_pairs in enumerate(schedule):
        shuffled = gen.sample(int(np.ceil(2 * num_pairs * cfg["frag"])))
        pairs = frag(shuffled, cfg["frag"], num_pairs)
        picks = np.array([(by_id[id(shuffled[k].obs)], s) for k, s in frag.last_picks], np.int64)
        np.testing.assert_array_equal(picks, z[f"it{i}_picks"], err_msg=f"iteration {i}")
        prefs = gath(pairs)
        assert prefs.dtype == np.float32
        np.testing.assert_array_equal(prefs, z[f"it{i}_prefs"], err_msg=f"iteration {i}")


@pytest.mark.parametrize("sched,expect", [("constant", [10, 30, 30, 30]), ("hyperbolic", [10, 40, 30, 20]),
                                           ("inverse_quadratic", [10, 43, 34, 13])])
def test_query_schedules_and_oric(sched, expect):
    algo = pc.PreferenceComparisons(pc.TrajectoryDataset([], np.random.default_rng(0)), None, num_iterations=3,
                                    rng=None, fragmenter=pc.RandomFragmenter(np.random.default_rng(0)),
                                    preference_gatherer=pc.SyntheticGatherer(sample=False), reward_trainer=_Stub(),
                                    query_schedule=sched)
    got = algo.query_schedule_for(100)
    assert sum(got) == 100 and got[0] == 10
    vec = np.vectorize(pc.QUERY_SCHEDULES[sched])(np.linspace(0, 1, 3))
    exact = vec / vec.sum() * 90
    np.testing.assert_array_equal(got[1:], pc.oric(exact))
    assert np.abs(np.array(got[1:]) - exact).max() < 1


def test_oric_keeps_sum_and_rounds_by_shortfall():
    x = np.array([1.2, 2.7, 3.1, 0.0, 2.0])
    r = pc.oric(x)
    assert r.sum() == 9 and r.tolist() == [1, 3, 3, 0, 2]


def _frag(n, v=0.0):
    return dt.TrajectoryWithRew(obs=np.full((n + 1, 2), v, np.float32), acts=np.zeros((n, 1), np.float32),
                                rews=np.full(n, v, np.float32), infos=None, terminal=False)


def test_dataset_fifo_errors_and_save_load(tmp_path):
    ds = pc.PreferenceDataset(max_size=3)
    ds.push([(_frag(2, 0), _frag(2, 1)), (_frag(2, 2), _frag(2, 3))], np.array([1, 0], np.float32))
    ds.push([(_frag(2, 4), _frag(2, 5)), (_frag(2, 6), _frag(2, 7))], np.array([0.5, 1], np.float32))
    assert len(ds) == 3
    assert [f.rews[0] for f in ds.fragments1] == [2, 4, 6]
    np.testing.assert_array_equal(ds.preferences, [0, 0.5, 1])
    (f1, f2), p = ds[0]
    assert f1.rews[0] == 2 and f2.rews[0] == 3 and p == 0
    with pytest.raises(ValueError, match="Unexpected preferences shape"):
        ds.push([(_frag(2), _frag(2))], np.array([1, 0], np.float32))
    with pytest.raises(ValueError, match="dtype float32"):
        ds.push([(_frag(2), _frag(2))], np.array([1.0]))
    ds._mirror = object()   # a device mirror is never pickled
    path = tmp_path / "ds.pkl"
    ds.save(path)
    back = pc.PreferenceDataset.load(path)
    assert back._mirror is None and back.max_size == 3 and len(back) == 3
    np.testing.assert_array_equal(back.preferences, ds.preferences)
    assert [f.rews[0] for f in back.fragments2] == [5, 7, 3][:0] or [f.rews[0] for f in back.fragments2] == [3, 5, 7]


def test_constructor_errors():
    gen = pc.TrajectoryDataset([], np.random.default_rng(0))
    with pytest.raises(ValueError, match="you must provide your own"):
        pc.PreferenceComparisons(gen, None, num_iterations=1)
    with pytest.raises(ValueError, match="you don't need to provide a random state"):
        pc.PreferenceComparisons(gen, None, num_iterations=1, rng=np.random.default_rng(0),
                                 fragmenter=pc.RandomFragmenter(np.random.default_rng(0)),
                                 preference_gatherer=pc.SyntheticGatherer(sample=False), reward_trainer=_Stub())
    with pytest.raises(ValueError, match="Unknown query schedule"):
        pc.PreferenceComparisons(gen, None, num_iterations=1, fragmenter=pc.RandomFragmenter(np.random.default_rng(0)),
                                 preference_gatherer=pc.SyntheticGatherer(sample=False), reward_trainer=_Stub(),
                                 query_schedule="nope")
    with pytest.raises(ValueError, match="`rng` must be provided"):
        pc.SyntheticGatherer()
    with pytest.raises(ValueError, match="No trajectories are long enough"):
        pc.RandomFragmenter(np.random.default_rng(0))([_frag(3)], 5, 1)
    with pytest.raises(RuntimeError, match="only 3 available"):
        pc._get_trajectories([_frag(3)], 4)


def test_out_of_scope_components_raise():
    with pytest.raises(NotImplementedError, match="ActiveSelectionFragmenter"):
        pc.ActiveSelectionFragmenter()
    with pytest.raises(NotImplementedError, match="EnsembleTrainer"):
        pc.EnsembleTrainer()
    with pytest.raises(NotImplementedError, match="exploration"):
        pc.AgentTrainer(None, None, None, np.random.default_rng(0), exploration_frac=0.1)

    class RewardEnsemble:
        pass

    with pytest.raises(NotImplementedError, match="ensembles"):
        pc.PreferenceModel(RewardEnsemble())
    pm = object.__new__(pc.PreferenceModel)
    with pytest.raises(NotImplementedError, match="regularizers"):
        pc.BasicRewardTrainer(pm, pc.CrossEntropyRewardLoss(), np.random.default_rng(0),
                              regularizer_factory=lambda **k: None)


def test_batch_size_multiple_of_minibatch():
    pm = object.__new__(pc.PreferenceModel)
    with pytest.raises(ValueError, match="multiple of minibatch size"):
        pc.BasicRewardTrainer(pm, pc.CrossEntropyRewardLoss(), np.random.default_rng(0), batch_size=8, minibatch_size=3)


def test_gatherer_temperature_zero_and_no_sample():
    pairs = [(_frag(2, 1.0), _frag(2, 0.0)), (_frag(2, 0.0), _frag(2, 0.0)), (_frag(2, 0.0), _frag(2, 1.0))]
    np.testing.assert_array_equal(pc.SyntheticGatherer(temperature=0, sample=False)(pairs), [1, 0.5, 0])
    p = pc.SyntheticGatherer(sample=False)(pairs)
    np.testing.assert_allclose(p, [1 / (1 + np.exp(-2)), 0.5, 1 / (1 + np.exp(2))], rtol=1e-6)


@pytest.mark.parametrize("n,mb", [(10, 4), (7, 7), (33, 8)])
def test_loader_shuffle_matches_dataloader(n, mb):
    epochs = 4
    th.manual_seed(123)
    loader = th.utils.data.DataLoader(list(range(n)), batch_size=mb, shuffle=True, collate_fn=list)
    want = [np.concatenate([np.array(b) for b in loader]) for _ in range(epochs)]
    state_want = th.get_rng_state()
    th.manual_seed(123)
    got = pc.loader_epoch_permutations(n, epochs)
    for w, g in zip(want, got):
        np.testing.assert_array_equal(w, g)
    assert th.equal(th.get_rng_state(), state_want)


def test_minibatch_schedule_accumulation_and_remainder():
    pm = object.__new__(pc.PreferenceModel)
    tr = object.__new__(pc.BasicRewardTrainer)
    tr.batch_size, tr.minibatch_size = 8, 4
    th.manual_seed(0)
    sched = tr._schedule(10, 2)   # per epoch: 4 (new), 4 (accumulate, step), 2 (new, step: remainder)
    assert [(e, len(mb), s, a, st) for e, mb, s, a, st in sched] == [
        (0, 4, 0.5, False, False), (0, 4, 0.5, True, True), (0, 2, 0.25, False, True),
        (1, 4, 0.5, False, False), (1, 4, 0.5, True, True), (1, 2, 0.25, False, True)]
    del pm


def test_logger_warn_and_accumulate_prefixes():
    from imitation_amd.logger import configure
    lg = configure(format_strs=[])
    lg.warn("x")
    assert lg.get_accumulate_prefixes() == ""
    with lg.add_accumulate_prefix("a"):
        with lg.add_accumulate_prefix("b"):
            assert lg.get_accumulate_prefixes() == "a/b/"
