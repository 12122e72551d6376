"""`regularization/regularizers.py` and `regularization/updaters.py`: regularizers of the preference reward trainer
(`preference_comparisons.BasicRewardTrainer(regularizer_factory=...)`), with lambda resident on the device.

The constructors, their checks (messages and order), `create`, `update_params` and `IntervalParamScaler.__call__` are the
reference's. What differs is where the work runs: the penalty and its gradient (`ia_reg_lp`), the weight decay
(`ia_reg_weight_decay`) and the interval schedule at each epoch end (`ia_reg_lambda_update`) are HIP kernels that read one
device `float64` scalar owned by the regularizer, so a regularised `train()` call stays one enqueue and one read-back.
`Regularizer.lambda_` is the host mirror of that scalar: reading returns the mirror (refreshed at every read-back of the
trainer), setting writes the mirror and the device scalar. Lambda persists across `train()` calls.

The trainer has no autograd on its product path, so a penalty is a kernel, not a Python method: `BasicRewardTrainer`
accepts only a `RegularizerFactory` of `LpRegularizer` or `WeightDecayRegularizer` themselves. A user subclass with its own
`_loss_penalty` / `_weight_penalty` is refused there (`NotImplementedError`): a deliberate cut. A `LambdaUpdater` stays a
protocol: any `f(lambda_, train_loss, val_loss) -> float` is allowed. An `IntervalParamScaler` runs on the device; any other
callable costs one synchronisation per epoch (the trainer calls it on the host and writes its result into the scalar).

Deviation: on the device schedule the `ValueError`s of `IntervalParamScaler.__call__` are raised at the trainer's read-back,
not at the epoch where they arose (the rest of the call is enqueued by then); lambda is left alone from that epoch on.
"""
from __future__ import annotations

import abc
from typing import Callable, Optional, Sequence, Tuple, Type

import numpy as np
import torch as th

from imitation_amd import _lib as L

LambdaUpdater = Callable[[float, float, float], float]
"""`updaters.LambdaUpdater`: `(lambda_, train_loss, val_loss) -> float`, side-effect free."""


LAMBDA_ZERO_MESSAGE = ("lambda_ must not be zero. Make sure that you're not scaling the value of lambda down too quickly "
                       "or passing an initial value of zero to the lambda parameter.")
LAMBDA_NEGATIVE_MESSAGE = "lambda_ must be non-negative"
LOSS_NEGATIVE_MESSAGE = "losses must be non-negative for this updater"
ERROR_MESSAGES = {L.REG_LAMBDA_ZERO: LAMBDA_ZERO_MESSAGE, L.REG_LAMBDA_NEGATIVE: LAMBDA_NEGATIVE_MESSAGE,
                  L.REG_LOSS_NEGATIVE: LOSS_NEGATIVE_MESSAGE}
"""The `ValueError` behind each error code of an `ia_reg_lambda_update` history row."""


class IntervalParamScaler:
    """`updaters.py:28-133`: scales lambda up by `1 + scaling_factor` when `val_loss / train_loss` lies above the tolerable
    interval, down by `1 - scaling_factor` when below, and leaves it inside (bounds included: the comparisons are strict)."""

    def __init__(self, scaling_factor: float, tolerable_interval: Tuple[float, float]):
        eps = np.finfo(float).eps
        if not (eps < scaling_factor < 1 - eps):
            raise ValueError("scaling_factor must be in (0, 1) within machine precision.")
        if len(tolerable_interval) != 2:
            raise ValueError("tolerable_interval must be a tuple of length 2")
        if not (0 <= tolerable_interval[0] < tolerable_interval[1]):
            raise ValueError("tolerable_interval must be a tuple whose first element is at least 0 and the second "
                             "element is greater than the first")
        self.scaling_factor = scaling_factor
        self.tolerable_interval = tolerable_interval

    def __call__(self, lambda_: float, train_loss, val_loss) -> float:
        if not (isinstance(val_loss, float) or (isinstance(val_loss, th.Tensor) and val_loss.dim() == 0)):
            raise ValueError("val_loss must be a scalar")
        if not (isinstance(train_loss, float) or (isinstance(train_loss, th.Tensor) and train_loss.dim() == 0)):
            raise ValueError("train_loss must be a scalar")
        if np.finfo(float).eps > abs(lambda_):
            raise ValueError(LAMBDA_ZERO_MESSAGE)
        elif lambda_ < 0:
            raise ValueError(LAMBDA_NEGATIVE_MESSAGE)
        if not isinstance(lambda_, float):
            raise ValueError("lambda_ must be a float")
        if train_loss < 0 or val_loss < 0:
            raise ValueError(LOSS_NEGATIVE_MESSAGE)
        eps = np.finfo(float).eps
        if train_loss < eps and val_loss < eps:
            return lambda_   # 0 / 0 is undefined: keep lambda
        elif train_loss < eps <= val_loss:
            return lambda_ * (1 + self.scaling_factor)   # the ratio would be infinite
        val_to_train_ratio = val_loss / train_loss
        if val_to_train_ratio > self.tolerable_interval[1]:
            lambda_ *= 1 + self.scaling_factor
        elif val_to_train_ratio < self.tolerable_interval[0]:
            lambda_ *= 1 - self.scaling_factor
        return lambda_


# ---------------------------------------------------------------------------------------------- kernel entries

def segment_table(segments: Sequence[Tuple[th.Tensor, Optional[th.Tensor]]]) -> th.Tensor:
    """The device table `ia_reg_lp` / `ia_reg_weight_decay` walk: one row (parameter pointer, gradient pointer, float
    count) per `(param, grad)` pair of contiguous fp32 device tensors (`grad` None: a null pointer, weight decay only).
    The tensors must outlive every launch that reads the table."""
    rows = []
    for w, g in segments:
        assert w.is_contiguous() and w.dtype == th.float32 and w.is_cuda
        assert g is None or (g.is_contiguous() and g.dtype == th.float32 and g.numel() == w.numel() and g.is_cuda)
        rows.append((w.data_ptr(), 0 if g is None else g.data_ptr(), w.numel()))
    return th.tensor(rows, dtype=th.int64).reshape(-1, 3).to(segments[0][0].device)


def lp_penalty(table: th.Tensor, p: int, lambda_dev: th.Tensor, stats_row: Optional[th.Tensor] = None,
               loss_scale: float = 1.0, s_out: Optional[th.Tensor] = None) -> None:
    """`ia_reg_lp`: adds `float(lambda) * p * sign(w) * |w|^(p-1)` to every gradient of the table; with `stats_row`
    (>= 4 floats, the loss in column 0) writes `loss * loss_scale + float(lambda) * sum |w|^p` into column 3; `s_out`
    (one float) receives the sum."""
    assert lambda_dev.dtype == th.float64 and table.dtype == th.int64
    assert (stats_row is None or (stats_row.dtype == th.float32 and stats_row.numel() >= 4))
    assert s_out is None or s_out.dtype == th.float32
    L.call("ia_reg_lp", L.ptr(table), int(table.shape[0]), int(p), L.ptr(lambda_dev), L.ptr(stats_row), float(loss_scale),
           L.ptr(s_out), L.stream())


def weight_decay(table: th.Tensor, lambda_dev: th.Tensor, lr: float) -> None:
    """`ia_reg_weight_decay`: `w <- w + float(-lambda * lr) * w` on every segment of the table."""
    assert lambda_dev.dtype == th.float64
    L.call("ia_reg_weight_decay", L.ptr(table), int(table.shape[0]), L.ptr(lambda_dev), float(lr), L.stream())


def lambda_update(lambda_dev: th.Tensor, scaler: IntervalParamScaler, train_stats: Optional[th.Tensor],
                  train_scales: Optional[th.Tensor], val_stats: Optional[th.Tensor], row: th.Tensor,
                  prev_row: Optional[th.Tensor] = None) -> None:
    """`ia_reg_lambda_update`: `scaler` applied in place to the device lambda on the summed losses (column 0) of the
    statistics rows `train_stats` `[n, w]` (each times its fp32 scale) and `val_stats` `[m, w]`; `row` (4 doubles) receives
    (lambda after, train_loss, val_loss, error code)."""
    assert lambda_dev.dtype == th.float64 and row.dtype == th.float64 and row.numel() >= 4
    n_t = 0 if train_stats is None else int(train_stats.shape[0])
    n_v = 0 if val_stats is None else int(val_stats.shape[0])
    stride = int((train_stats if n_t else val_stats).stride(0)) if (n_t or n_v) else 1
    assert all(t is None or t.dtype == th.float32 for t in (train_stats, train_scales, val_stats))
    assert not (n_t and n_v) or train_stats.stride(0) == val_stats.stride(0)
    L.call("ia_reg_lambda_update", L.ptr(lambda_dev), train_stats.data_ptr() if n_t else None,
           L.ptr(train_scales) if n_t else None, n_t, val_stats.data_ptr() if n_v else None, n_v, stride,
           float(scaler.scaling_factor), float(scaler.tolerable_interval[0]), float(scaler.tolerable_interval[1]),
           L.ptr(prev_row), L.ptr(row), L.stream())


# ---------------------------------------------------------------------------------------------- regularizers

class RegularizerFactory:
    """What `Regularizer.create` returns (the reference's `RegularizerFactory` protocol as a small callable object, so
    that a trainer can see which class it builds): `factory(optimizer=..., logger=...)` constructs the regularizer."""

    def __init__(self, cls: Type["Regularizer"], initial_lambda: float, lambda_updater: Optional[LambdaUpdater],
                 val_split, kwargs: dict):
        self.cls = cls
        self.initial_lambda = initial_lambda
        self.lambda_updater = lambda_updater
        self.val_split = val_split
        self.kwargs = dict(kwargs)

    def __call__(self, *, optimizer, logger) -> "Regularizer":
        return self.cls(initial_lambda=self.initial_lambda, optimizer=optimizer, lambda_updater=self.lambda_updater,
                        logger=logger, val_split=self.val_split, **self.kwargs)


class Regularizer(abc.ABC):
    """`regularizers.py:59-192`. `optimizer` is the trainer's (`networks.HipAdam` over a product net's flat buffer or
    `ops.HipAdamW` over `nn.Parameter`s); it may be None for a regularizer that only exists for its log record (the
    `EnsembleTrainer`'s own: its members hold the ones that train)."""

    def __init__(self, optimizer, initial_lambda: float, lambda_updater: Optional[LambdaUpdater], logger,
                 val_split: Optional[float] = None) -> None:
        if lambda_updater is None and np.allclose(initial_lambda, 0.0):
            raise ValueError("If you do not pass a regularizer parameter updater your regularization strength must be "
                             "non-zero, as this would result in no regularization.")
        if val_split is not None and (not isinstance(val_split, float) or np.allclose(val_split, 0.0)
                                      or val_split <= 0 or val_split >= 1):
            raise ValueError(f"val_split = {val_split} must be a float strictly between 0 and 1.")
        if lambda_updater is not None and val_split is None:
            raise ValueError("If you pass a regularizer parameter updater, you must also specify a validation split. "
                             "Otherwise the updater won't have any validation data to use for updating.")
        elif lambda_updater is None and val_split is not None:
            raise ValueError("If you pass a validation split, you must also pass a regularizer parameter updater. "
                             "Otherwise you are wasting data into the validation split that will not be used.")
        self.optimizer = optimizer
        self._lambda = initial_lambda
        self._lambda_dev: Optional[th.Tensor] = None
        self.lambda_updater = lambda_updater
        self.logger = logger
        self.val_split = val_split
        self.logger.record("regularization_lambda", self.lambda_)

    @classmethod
    def create(cls, initial_lambda: float, lambda_updater: Optional[LambdaUpdater] = None, val_split: float = 0.0,
               **kwargs) -> RegularizerFactory:
        """`regularizers.py:135-159`. As in the reference `val_split` defaults to 0.0, which the constructor rejects:
        pass `val_split=None` for a regularizer without an updater."""
        return RegularizerFactory(cls, initial_lambda, lambda_updater, val_split, kwargs)

    # -- lambda: a host mirror of one device double
    @property
    def lambda_(self) -> float:
        return self._lambda

    @lambda_.setter
    def lambda_(self, value: float) -> None:
        self._lambda = value
        if self._lambda_dev is not None:
            self._lambda_dev.fill_(float(value))

    def device_lambda(self, device) -> th.Tensor:
        """The device scalar (`float64`, one element), created from the mirror on first use."""
        dev = th.device(device)
        if self._lambda_dev is None or self._lambda_dev.device != dev:
            self._lambda_dev = th.full((1,), float(self._lambda), dtype=th.float64, device=dev)
        return self._lambda_dev

    def refresh_lambda(self, value: float) -> None:
        """The mirror takes a value read back from the device scalar."""
        self._lambda = float(value)

    @property
    def device_schedule(self) -> bool:
        """Whether the lambda schedule runs on the device (`ia_reg_lambda_update`)."""
        return type(self.lambda_updater) is IntervalParamScaler

    @abc.abstractmethod
    def launch(self, table: th.Tensor, stats_row: Optional[th.Tensor], loss_scale: float) -> None:
        """The regularization of one training minibatch, after its backward and before the optimiser step, on the
        segments of `table` (`segment_table`): the device form of the reference's `regularize_and_backward`."""

    def update_params(self, train_loss, val_loss) -> None:
        """`regularizers.py:179-192`."""
        if self.lambda_updater is not None:
            self.lambda_ = self.lambda_updater(self.lambda_, train_loss, val_loss)
            self.logger.record("regularization_lambda", self.lambda_)


class LossRegularizer(Regularizer):
    """`regularizers.py:195-224`: regularizers that add a term to the loss (here: its gradient to the gradient buffer and
    `regularized_loss` to the statistics row)."""

    needs_grads = True


class WeightRegularizer(Regularizer):
    """`regularizers.py:227-250`: regularizers that change the weights after the backward pass."""

    needs_grads = False


class LpRegularizer(LossRegularizer):
    """`regularizers.py:253-290`: the penalty `lambda * sum |w|^p` over the optimiser's parameters."""

    def __init__(self, optimizer, initial_lambda: float, lambda_updater: Optional[LambdaUpdater], logger, p: int,
                 val_split: Optional[float] = None) -> None:
        super().__init__(optimizer, initial_lambda, lambda_updater, logger, val_split)
        if not isinstance(p, int) or p < 1:
            raise ValueError("p must be a positive integer")
        self.p = p

    def launch(self, table, stats_row, loss_scale):
        lp_penalty(table, self.p, self.device_lambda(table.device), stats_row, loss_scale)


class WeightDecayRegularizer(WeightRegularizer):
    """`regularizers.py:293-306`: `w += -lambda * lr * w` with the learning rate of the optimiser's (one) parameter
    group."""

    def launch(self, table, stats_row, loss_scale):
        weight_decay(table, self.device_lambda(table.device), float(self.optimizer.param_groups[0]["lr"]))


SHIPPED = (LpRegularizer, WeightDecayRegularizer)
