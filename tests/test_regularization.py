"""`imitation_amd.regularization` on the host: the constructors' checks, `IntervalParamScaler.__call__`, the train /
validation split and the interleaved loader draws against torch's own, the trainer's schedule against the lambda history
of the reference's goldens (`tests/golden/preference_reg_*.npz`), and which factories `BasicRewardTrainer` accepts."""
import json
import os

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import preference_comparisons as pc
from imitation_amd import regularization as rg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["preference_reg_l2", "preference_reg_l3_norm", "preference_reg_l1", "preference_reg_wd", "preference_reg_fixed"]
SCALER = rg.IntervalParamScaler(0.5, (0.77, 2.0))
EPS = np.finfo(float).eps

# (lambda, train_loss, val_loss, expected): shared with the kernel test, which runs the same cases on the device
SCALER_CASES = [
    (0.01, 1.0, 2.5, 0.01 * 1.5),       # above the interval
    (0.01, 1.0, 0.5, 0.01 * 0.5),       # below
    (0.01, 1.0, 1.0, 0.01),             # inside
    (0.01, 1.0, 2.0, 0.01),             # exactly at the upper bound: strict comparison, nothing happens
    (0.01, 100.0, 77.0, 0.01),          # exactly at the lower bound (77 / 100 rounds to the double 0.77)
    (0.3, EPS / 2, EPS / 4, 0.3),       # both losses below eps: lambda stays
    (0.3, EPS / 2, EPS, 0.3 * 1.5),     # train below eps, val at eps: up
    (0.3, 0.0, 1.0, 0.3 * 1.5),         # train zero: the ratio would be infinite
]
SCALER_ERRORS = [
    (0.0, 1.0, 1.0, "must not be zero"),
    (EPS / 2, 1.0, 1.0, "must not be zero"),
    (-0.5, 1.0, 1.0, "non-negative"),
    (0.01, -1.0, 1.0, "losses must be non-negative"),
    (0.01, 1.0, -1.0, "losses must be non-negative"),
]


def _logger():
    return p.configure_logger(format_strs=[])


# ---------------------------------------------------------------------------------------------- constructors

def test_constructor_checks_in_the_reference_order():
    lg = _logger()
    with pytest.raises(ValueError, match="regularization strength must be non-zero"):
        rg.LpRegularizer(None, 0.0, None, lg, p=2)
    for bad in (0.0, 1.0, -0.1, 1, 1.5):
        with pytest.raises(ValueError, match="must be a float strictly between 0 and 1"):
            rg.LpRegularizer(None, 0.1, SCALER, lg, p=2, val_split=bad)
    # lambda 0 is checked before the split
    with pytest.raises(ValueError, match="regularization strength must be non-zero"):
        rg.WeightDecayRegularizer(None, 0.0, None, lg, val_split=2.0)
    with pytest.raises(ValueError, match="you must also specify a validation split"):
        rg.WeightDecayRegularizer(None, 0.1, SCALER, lg)
    with pytest.raises(ValueError, match="you must also pass a regularizer parameter updater"):
        rg.WeightDecayRegularizer(None, 0.1, None, lg, val_split=0.2)
    for bad in (0, -1, 2.0, "2"):
        with pytest.raises(ValueError, match="p must be a positive integer"):
            rg.LpRegularizer(None, 0.1, None, lg, p=bad)
    # the base checks come before p's
    with pytest.raises(ValueError, match="you must also specify a validation split"):
        rg.LpRegularizer(None, 0.1, SCALER, lg, p=0)
    # lambda 0 with an updater is allowed at construction
    assert rg.LpRegularizer(None, 0.0, SCALER, lg, p=1, val_split=0.5).lambda_ == 0.0


def test_create_defaults_val_split_to_zero_like_the_reference():
    lg = _logger()
    factory = rg.LpRegularizer.create(0.1, p=2)
    assert isinstance(factory, rg.RegularizerFactory) and factory.cls is rg.LpRegularizer
    with pytest.raises(ValueError, match=r"val_split = 0.0 must be a float strictly between 0 and 1\."):
        factory(optimizer=None, logger=lg)
    reg = rg.LpRegularizer.create(0.1, val_split=None, p=2)(optimizer=None, logger=lg)
    assert reg.p == 2 and reg.lambda_ == 0.1 and reg.val_split is None and reg.lambda_updater is None
    with pytest.raises(TypeError):
        factory(None, lg)   # keyword-only


def test_construction_records_lambda_and_the_setter_keeps_the_mirror():
    lg = _logger()
    reg = rg.WeightDecayRegularizer.create(0.25, SCALER, val_split=0.5)(optimizer=None, logger=lg)
    assert lg.default_logger.name_to_value["regularization_lambda"] == 0.25
    reg.lambda_ = 0.5
    assert reg.lambda_ == 0.5
    reg.update_params(1.0, 2.5)
    assert reg.lambda_ == 0.75 and lg.default_logger.name_to_value["regularization_lambda"] == 0.75
    assert reg.device_schedule
    assert not rg.LpRegularizer(None, 0.1, lambda l, t, v: SCALER(l, t, v), lg, p=2, val_split=0.5).device_schedule


def test_interval_scaler_constructor_checks():
    for bad in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="scaling_factor must be in"):
            rg.IntervalParamScaler(bad, (0.5, 1.5))
    with pytest.raises(ValueError, match="tuple of length 2"):
        rg.IntervalParamScaler(0.5, (0.5, 1.0, 1.5))
    for bad in ((-0.1, 1.0), (1.0, 1.0), (2.0, 1.0)):
        with pytest.raises(ValueError, match="first element is at least 0"):
            rg.IntervalParamScaler(0.5, bad)


@pytest.mark.parametrize("lam,train,val,want", SCALER_CASES)
def test_interval_scaler_decisions(lam, train, val, want):
    assert SCALER(lam, train, val) == want
    assert SCALER(lam, th.tensor(train, dtype=th.float64), th.tensor(val, dtype=th.float64)) == want


@pytest.mark.parametrize("lam,train,val,msg", SCALER_ERRORS)
def test_interval_scaler_errors(lam, train, val, msg):
    with pytest.raises(ValueError, match=msg):
        SCALER(lam, train, val)


def test_interval_scaler_type_errors():
    with pytest.raises(ValueError, match="lambda_ must be a float"):
        SCALER(1, 1.0, 1.0)
    with pytest.raises(ValueError, match="val_loss must be a scalar"):
        SCALER(0.1, 1.0, th.ones(2))
    with pytest.raises(ValueError, match="train_loss must be a scalar"):
        SCALER(0.1, th.ones(2), 1.0)
    with pytest.raises(ValueError, match="val_loss must be a scalar"):
        SCALER(0.1, 1.0, 1)


# ---------------------------------------------------------------------------------------------- split and loaders

@pytest.mark.parametrize("n,split", [(10, 0.25), (7, 0.5), (33, 0.2)])
def test_split_matches_random_split(n, split):
    val_length = int(n * split)
    seed = pc.make_seeds(np.random.default_rng(n))
    want = th.utils.data.random_split(list(range(n)), lengths=[n - val_length, val_length],
                                      generator=th.Generator().manual_seed(seed))
    train, val = pc.random_split_indices(n, val_length, th.Generator().manual_seed(seed))
    np.testing.assert_array_equal(train, want[0].indices)
    np.testing.assert_array_equal(val, want[1].indices)
    assert len(train) == n - val_length and len(val) == val_length


@pytest.mark.parametrize("n,split,mb", [(10, 0.25, 4), (7, 0.5, 7), (33, 0.2, 8)])
def test_interleaved_loader_shuffle_matches_two_dataloaders(n, split, mb):
    epochs = 3
    val_length = int(n * split)
    parts = th.utils.data.random_split(list(range(100, 100 + n)), lengths=[n - val_length, val_length],
                                       generator=th.Generator().manual_seed(5))
    th.manual_seed(123)
    loaders = [th.utils.data.DataLoader(part, batch_size=mb, shuffle=True, collate_fn=list) for part in parts]
    want = []
    for _ in range(epochs):   # the reference's order: the whole train loader, then the whole validation loader
        want.append([np.concatenate([np.array(b) for b in loader]) for loader in loaders])
    state_want = th.get_rng_state()
    th.manual_seed(123)
    got = pc.loader_epoch_permutations_split(n - val_length, val_length, epochs)
    for (wt, wv), (gt, gv) in zip(want, got):
        np.testing.assert_array_equal(wt, 100 + np.asarray(parts[0].indices)[gt])
        np.testing.assert_array_equal(wv, 100 + np.asarray(parts[1].indices)[gv])
    assert th.equal(th.get_rng_state(), state_want)


# ---------------------------------------------------------------------------------------------- schedule against the goldens

def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(str(z["cfg"]))


@pytest.mark.parametrize("name", [c for c in CASES if c != "preference_reg_fixed"])
def test_schedule_places_validation_and_update_like_the_recorded_history(name):
    z, cfg = _golden(name)
    tr = object.__new__(pc.BasicRewardTrainer)
    tr.batch_size, tr.minibatch_size = cfg["batch"], cfg["mb"] or cfg["batch"]
    th.manual_seed(0)
    n = 0
    for i in range(int(z["n_iters"])):
        n += int(z["schedule"][i])
        train_idx, val_idx = z[f"it{i}_split_train"], z[f"it{i}_split_val"]
        assert len(val_idx) == int(n * cfg["val_split"]) and len(train_idx) + len(val_idx) == n
        epochs = int((z["lambda_hist_call"] == i).sum())
        assert epochs == round(cfg["epochs"] * (cfg["init_mult"] if i == 0 else 1.0))
        sched = tr._schedule_split(train_idx, val_idx, epochs)
        keys = set(str(k) for k in z[f"it{i}_log_keys"])
        for e in range(epochs):
            items = [it for it in sched if it[0] == e]
            kinds = ["update" if it[1] is None else ("val" if it[2] is None else "train") for it in items]
            n_train, n_val = kinds.count("train"), kinds.count("val")
            assert kinds == ["train"] * n_train + ["val"] * n_val + ["update"]
            assert n_train == -(-len(train_idx) // tr.minibatch_size) and n_val == -(-len(val_idx) // tr.minibatch_size)
            np.testing.assert_array_equal(np.sort(np.concatenate([it[1] for it in items[:n_train]])), np.sort(train_idx))
            np.testing.assert_array_equal(np.sort(np.concatenate([it[1] for it in items[n_train:-1]])), np.sort(val_idx))
            assert items[n_train - 1][4] is True   # the epoch's last training minibatch steps
            for key in ("val/loss", "val/accuracy", "val/gt_reward_loss", "train/loss", "regularization_lambda"):
                assert f"mean/reward/epoch-{e}/{key}" in keys
        assert f"mean/reward/epoch-{epochs}/train/loss" not in keys


def test_train_refuses_a_split_with_an_empty_part():
    tr = object.__new__(pc.BasicRewardTrainer)
    tr.regularizer = rg.LpRegularizer(None, 0.1, SCALER, _logger(), p=2, val_split=0.25)
    tr.rng = np.random.default_rng(0)
    assert tr.requires_regularizer_update
    with pytest.raises(ValueError, match="Not enough data samples to split"):
        tr._train([0, 1, 2], 1.0)   # int(3 * 0.25) = 0 validation pairs


@pytest.mark.parametrize("name", CASES)
def test_fixture_log_keys(name):
    z, cfg = _golden(name)
    for i in range(int(z["n_iters"])):
        keys = set(str(k) for k in z[f"it{i}_log_keys"])
        has = lambda part: any(part in k for k in keys)   # noqa: E731
        assert has("reward/final/train/loss")
        assert has("regularized_loss") == (cfg["reg"] == "lp")
        assert has("epoch-0/regularization_lambda") == (cfg["val_split"] is not None)
        assert has("reward/final/val/loss") == has("reward/final/val/accuracy") == has("reward/final/val/gt_reward_loss") \
            == (cfg["val_split"] is not None)
    # constructing the regularizer records lambda: the key is in the first dump with or without a schedule
    assert "regularization_lambda" in set(str(k) for k in z["it0_log_keys"])


# ---------------------------------------------------------------------------------------------- accepted factories

def test_foreign_factories_are_refused():
    pm = object.__new__(pc.PreferenceModel)
    loss, rng = pc.CrossEntropyRewardLoss(), np.random.default_rng(0)

    def bare(*, optimizer, logger):
        return rg.LpRegularizer(optimizer, 0.1, None, logger, p=2)

    class MyLp(rg.LpRegularizer):
        pass

    class MyPenalty(rg.LossRegularizer):
        def launch(self, table, stats_row, loss_scale):
            pass

    for factory in (bare, MyLp.create(0.1, val_split=None, p=2), MyPenalty.create(0.1, val_split=None)):
        with pytest.raises(NotImplementedError, match="regularizers"):
            pc.BasicRewardTrainer(pm, loss, rng, regularizer_factory=factory)
