"""Float64 reference of PPO minibatch steps ([SB3 PPO.train] as `oracle.sb3_restated.PPO.train` restates it), with no GPU
in it: what `tests/test_ppo_ref.py` (any machine) and `tests/test_ppo_gradient_gpu.py` (`-m gpu`) compare against.

The forward pass is the oracle's own `ActorCriticPolicy` (its feature norm, both tanh towers, the DiagGaussian or
Categorical head), deep-copied, converted with `.double()` and fed float64 rows; torch autograd differentiates it. The only
call left out is `preprocess_obs`, whose `obs.float()` would round the rows back to float32 (they ARE float32 values).
Per step, in the oracle's order: train-mode `RunningNorm` update on the minibatch's observations, normalise, towers, log
probability and entropy, advantages normalised with the unbiased std + 1e-8, ratio, clipped surrogate, value MSE, entropy
loss, `loss = pg + ent_coef * ent + vf_coef * value`, backward, `clip_grad_norm_` (coefficient `max_norm / (norm + 1e-6)`
clamped to 1), torch's Adam (restated on flat vectors; `tests/test_ppo_ref.py` holds it against `torch.optim.Adam`).

Cases (`CASES`): a policy geometry, a rollout of T x n rows built by `tests/test_ppo_tower_split_gpu._host_inputs` (the
builder of `test_ppo_epochs_match_oracle`), a minibatch size, ONE epoch on the first `np.random.seed(123)` permutation.
`rows == bs`: one step; `rows == 2 bs + r`: a chain of three steps with a short last minibatch. Each case's seed was
picked on the CPU so that the guards below hold (`SEEDS`: the cases whose seed is not 0).

Guards (`assert_guards`), conditions on the float64 run, never measurements:
  * no row's ratio lies within `RATIO_MARGIN` = 1e-3 of 1 - clip_range or 1 + clip_range at any step: the clip indicator
    cannot switch in float32, so `clip_fraction` is compared exactly (no row is ever left out to get there);
  * where a run is labelled clipped, `total_norm >= 1.05 * max_grad_norm` at every step;
  * every parameter block's largest gradient element is at least `MIN_BLOCK_SCALE` = 5 % of the largest element of the whole
    gradient. The vector measure below is relative to each block's own scale; a one-element block (cb, the head's bias
    with one action) that is a nearly cancelled sum over the rows would measure float32's cancellation (2e-5 on the CPU
    for a cb at 0.4 % of the gradient's scale), not the code under test.

Deviation measures (`deviations`) -- the SAME expressions give the float32-against-float64 noise floor on the CPU and the
figures the GPU tests assert on:
    grad, exp_avg, exp_avg_sq   per parameter block of `pol_offsets` (log_std, pW1, pb1, pW2, pb2, vW1, vb1, vW2, vb2, aW,
                                ab, cW, cb): max |dx| / max |ref| over the block; the worst block (a small block -- log_std,
                                a bias, cb -- cannot hide under a large one)
    params                      max |dx| / (1 + |ref|)
    pg_loss ... clip_coef       |dx| / |ref| (columns 0-3 and 5-7 of the statistics record)
    clip_fraction, norm count   exact (asserted by the callers, not measured)
    norm                        max |dv| / (1 + |v|) over running mean and variance, as `airl_ref` measures them

Noise floor (`FLOOR_STEP`, `FLOOR_CHAIN`): the worst deviation of the float32 oracle (`sb3_restated.PPO.train` on the CPU,
same policy, same buffer, same permutation) from this reference, over all cases, as `tests/test_ppo_ref.py` measures it
(its docstring has the table per case). torch's CPU float32 sums depend on the machine; the factor 8 of `TOL`
(the project's margin for kernels that sum the same fp32 terms in another order: MFMA tiles, slabs, split sums) covers that.
"""
from __future__ import annotations

import copy
import dataclasses
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch as th
from torch.nn import functional as F

from tests import airl_ref

CLIP_RANGE, ENT_COEF, VF_COEF, LR, BETA1, BETA2, ADAM_EPS = 0.2, 0.05, 0.5, 3e-4, 0.9, 0.999, 1e-5
UNCLIPPED, CLIPPED = 1e9, 0.5          # the two `max_grad_norm` every single step is judged with
RATIO_MARGIN = 1e-3
NORM_MARGIN = 1.05
MIN_BLOCK_SCALE = 0.05
STAT_NAMES = ("pg_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss", "grad_norm", "clip_coef")
MEASURED_STATS = tuple(s for s in STAT_NAMES if s != "clip_fraction")
VECTORS = ("grad", "exp_avg", "exp_avg_sq")
QUANTITIES = VECTORS + ("params", "norm") + MEASURED_STATS


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    D: int
    A: int
    H: int
    discrete: bool
    norm: bool
    T: int
    n: int
    bs: int
    seed: int = 0                 # of the rollout's generator; chosen so that `assert_guards` holds
    normalize_adv: bool = True

    @property
    def rows(self) -> int:
        return self.T * self.n

    @property
    def steps(self) -> int:
        return -(-self.rows // self.bs)


# Seeds other than 0, found by `python -m tests.test_ppo_ref seeds` (the first seed at which the guards hold, for both
# `max_grad_norm` of a single step and for `CLIPPED` on a chain; `sens_...`: the sensitivity shapes of that module).
SEEDS: Dict[str, int] = {
    "4x2b_h32_norm_T2n1_bs2": 2,
    "4x2b_h32_plain_T3n21_bs63": 1,
    "4x2b_h32_norm_T4n16_bs64": 2,
    "4x2b_h32_plain_T5n13_bs65": 1,
    "4x2b_h32_norm_T2n65_bs130": 21,
    "4x2b_h64_plain_T2n1_bs2": 1,
    "4x2b_h64_norm_T3n21_bs63": 1,
    "4x2b_h64_plain_T4n16_bs64": 3,
    "4x2b_h64_norm_T5n13_bs65": 3,
    "4x2b_h64_plain_T2n65_bs130": 19,
    "4x2d_h32_plain_T2n1_bs2": 2,
    "4x2d_h32_norm_T3n21_bs63": 1,
    "4x2d_h32_plain_T4n16_bs64": 3,
    "4x2d_h32_norm_T5n13_bs65": 3,
    "4x2d_h32_plain_T2n65_bs130": 5,
    "4x2d_h64_norm_T2n1_bs2": 2,
    "4x2d_h64_plain_T3n21_bs63": 2,
    "4x2d_h64_plain_T5n13_bs65": 6,
    "4x2d_h64_norm_T2n65_bs130": 4,
    "17x6b_h32_plain_T5n13_bs65": 1,
    "17x6b_h64_norm_T3n21_bs63": 2,
    "17x6b_h64_plain_T4n16_bs64": 2,
    "27x8b_h32_plain_T2n65_bs130": 1,
    "27x8b_h64_norm_T2n65_bs130": 5,
    "33x1b_h32_norm_T2n1_bs2": 1,
    "33x1b_h32_plain_T5n13_bs65": 2,
    "33x1b_h64_plain_T4n16_bs64": 2,
    "33x1b_h64_plain_T2n65_bs130": 9,
    "64x16b_h32_norm_T5n13_bs65": 2,
    "64x16b_h32_plain_T2n65_bs130": 5,
    "64x16b_h64_plain_T5n13_bs65": 1,
    "20x13d_h32_norm_T2n1_bs2": 1,
    "20x13d_h32_plain_T3n21_bs63": 1,
    "20x13d_h32_plain_T5n13_bs65": 1,
    "20x13d_h64_plain_T4n16_bs64": 9,
    "20x13d_h64_norm_T5n13_bs65": 13,
    "20x13d_h64_plain_T2n65_bs130": 45,
    "17x6b_h32_norm_T1n1_bs1_rawadv": 1,
    "4x2d_h64_norm_T1n1_bs1_rawadv": 1,
    "17x6b_h32_norm_T4n64_bs256": 2,
    "17x6b_h32_norm_T4n144_bs576": 14,
    "27x8b_h32_norm_T4n16_bs64": 2,
    "33x1b_h32_plain_T4n35_bs140": 1,
    "64x16b_h32_norm_T4n16_bs64": 2,
    "4x2d_h32_plain_T4n4_bs16": 1,
    "33x1b_h64_plain_T4n32_bs128": 1,
    "17x6b_h32_norm_T4n138_bs256": 3,
    "20x13d_h32_norm_T4n56_bs96": 9,
    "4x2d_h64_norm_T3n102_bs128": 111,
    "4x2d_h64_norm_T4n96_bs384": 83,
    "27x8b_h64_norm_T4n105_bs420": 12,
    "sens_20x13d_h32_T4n32_bs96": 1,
}

CASES: Dict[str, Case] = {}


def case_for(D, A, H, discrete, norm, bs, r=None, normalize_adv=True) -> Case:
    """The case of this geometry with one minibatch of `bs` rows (`r` None) or three (`2 bs + r` rows), registered in
    `CASES` on first use. T is the first of 4, 3, 2, 5, 7, 1 that divides the row count."""
    rows = bs if r is None else 2 * bs + r
    T = next(t for t in (4, 3, 2, 5, 7, 1) if rows % t == 0)
    name = f"{D}x{A}{'d' if discrete else 'b'}_h{H}_{'norm' if norm else 'plain'}_T{T}n{rows // T}_bs{bs}"
    if not normalize_adv:
        name += "_rawadv"
    if name not in CASES:
        CASES[name] = Case(name, D, A, H, bool(discrete), bool(norm), T, rows // T, bs, SEEDS.get(name, 0), normalize_adv)
    return CASES[name]


# A. `ia_ppo_minibatch_grad` / `_apply`: every geometry x tower width x the row counts around one and two 64-row blocks (130:
#    three blocks, the last with 2 rows); the feature norm on for every other combination; one row without advantage
#    normalisation.
GEOMETRIES = [(4, 2, False), (4, 2, True), (17, 6, False), (27, 8, False), (33, 1, False), (64, 16, False), (20, 13, True)]
GRAD_BATCHES = (2, 63, 64, 65, 130)
GRAD_CASES: List[str] = []
for _gi, (_D, _A, _disc) in enumerate(GEOMETRIES):
    for _hi, _H in enumerate((32, 64)):
        for _bi, _b in enumerate(GRAD_BATCHES):
            GRAD_CASES.append(case_for(_D, _A, _H, _disc, (_gi + _hi + _bi) % 2 == 0, _b).name)
GRAD_CASES.append(case_for(17, 6, 32, False, True, 1, normalize_adv=False).name)
GRAD_CASES.append(case_for(4, 2, 64, True, True, 1, normalize_adv=False).name)

# B. one step per launch. 32-wide towers (`ia_ppo_epoch`'s two launches per minibatch, `ia_ppo_update`): 12 and 16 rows (the
#    update's `small` kernel), 64 (`local`), 140 (three row blocks, the last of 12 rows), 256, 576 (nine row blocks, two
#    statistics slices, the second of 64 rows); both parameters-per-thread builds ((17, 6); (27, 8) and (33, 1): wide), both
#    observation-width classes ((33, 1), (64, 16): beyond 32 columns), Box and Discrete.
STEP32_CASES = [case_for(17, 6, 32, False, True, b).name for b in (12, 16, 64, 140, 256, 576)] + [
    case_for(27, 8, 32, False, True, 64).name, case_for(27, 8, 32, False, True, 256).name,
    case_for(33, 1, 32, False, False, 140).name, case_for(64, 16, 32, False, True, 64).name,
    case_for(20, 13, 32, True, True, 128).name, case_for(4, 2, 32, True, False, 16).name]
#    64-wide towers (`ia_ppo_epoch`'s one-launch forms): 64 rows (one row block, the parameters halved over two workgroups),
#    128, 200 (short last block); observation widths <= 16, <= 32 and beyond (the word-exchange kernel's three classes).
STEP64_MODE_CASES = [case_for(4, 2, 64, True, True, 64).name, case_for(17, 6, 64, False, True, 128).name,
                     case_for(27, 8, 64, False, True, 200).name]
#    Those three run `ia_ppo_epoch_split` modes 2 and 3 on the two-launch fallback: a 64-wide policy has more than 9 000
#    parameters, and the barrier forms need ceil(P / nrb) <= 2 048 (whole row-block workgroups) and ceil(P / 2 nrb) <= 1 024 (one
#    tower per workgroup) with nrb = ceil(bs / 64) row blocks (`plan_epoch`; `barrier_forms_fit` below). The smallest
#    minibatches that reach `ppo_epoch_persistent_kernel<64>` and `<64, true>`: six row blocks for (4, 2) (9 155 parameters) and
#    (17, 6) (11 085; 330 rows: the last block has 10), seven for (27, 8) (12 497; 420 rows: the last block has 36).
STEP64_BARRIER_CASES = [case_for(4, 2, 64, True, True, 384).name, case_for(17, 6, 64, False, True, 330).name,
                        case_for(27, 8, 64, False, True, 420).name]
STEP64_CASES = STEP64_MODE_CASES + STEP64_BARRIER_CASES + [case_for(33, 1, 64, False, False, 128).name, case_for(64, 16, 64, False, True, 64).name]

# C. three steps, the last minibatch short ((20, 13): 32 rows of 96 -- row block 1 receives none).
CHAIN_CASES = [case_for(17, 6, 32, False, True, 256, r=40).name, case_for(20, 13, 32, True, True, 96, r=32).name,
               case_for(4, 2, 64, True, True, 128, r=50).name]

# The shapes of `test_ppo_epochs_match_oracle` on which a scaled gradient block was shown to pass that test
# (`tests/test_ppo_ref.py`, sensitivity): (17, 6) with 256-row minibatches, (20, 13) Discrete, (17, 6) with 2 048-row ones.
SENSITIVITY_SHAPES = [(17, 6, 32, False, True, 16, 64, 256), (20, 13, 32, True, True, 4, 32, 96),
                      (17, 6, 32, False, True, 16, 256, 2048)]


def param_count(D, A, H, discrete) -> int:
    """`pol_offsets(...).total`: [log_std], two towers of (W1, b1, W2, b2), the action head, the value head."""
    return (0 if discrete else A) + 2 * (H * D + H + H * H + H) + (H * A + A) + (H + 1)


def barrier_forms_fit(case: Case):
    """`plan_epoch`'s chunk conditions for the grid-barrier epoch forms of 64-wide towers, (whole row-block workgroups --
    mode 2, one tower per workgroup -- mode 3): every workgroup steps ceil(P / workgroups) parameters with at most 4 per
    thread of its 512 / 256 threads, and at most 64 workgroups meet at the barrier. Where a condition fails the call runs two
    launches per minibatch."""
    P, nrb = param_count(case.D, case.A, case.H, case.discrete), -(-case.bs // 64)
    return (nrb <= 64 and -(-P // nrb) <= 4 * 512), (2 * nrb <= 64 and -(-P // (2 * nrb)) <= 4 * 256)


def sensitivity_case(D, A, H, discrete, norm, T, n, bs) -> Case:
    name = f"sens_{D}x{A}{'d' if discrete else 'b'}_h{H}_T{T}n{n}_bs{bs}"
    return Case(name, D, A, H, discrete, norm, T, n, bs, SEEDS.get(name, 0))


ULP = 2.0 ** -23
# Ceilings: what the project already allows for the same quantity. Gradient and Adam moments: `airl_ref.CEILING["grad"]`
# (2e-5, the same block-relative measure); parameters: `test_ppo_epochs_match_oracle`'s rtol (1 + k) 1e-5 after k steps;
# norm state: 1e-6 (`airl_ref`); loss statistics: that test's rel 2e-3 (5e-3 for approx_kl); grad_norm and clip_coef, which no
# test compared before: the gradient's 2e-5.
def _ceilings(k: int) -> Dict[str, float]:
    c = dict(grad=airl_ref.CEILING["grad"], exp_avg=airl_ref.CEILING["grad"], exp_avg_sq=airl_ref.CEILING["grad"],
             params=(1 + k) * 1e-5, norm=airl_ref.CEILING["norm"], pg_loss=2e-3, value_loss=2e-3, entropy_loss=2e-3,
             approx_kl=5e-3, loss=2e-3, grad_norm=airl_ref.CEILING["grad"], clip_coef=airl_ref.CEILING["grad"])
    assert set(c) == set(QUANTITIES)
    return c


CEILING_STEP, CEILING_CHAIN = _ceilings(1), _ceilings(3)
# Worst float32-oracle-against-float64 deviation over all single-step cases (both `max_grad_norm`) / all chains, as
# tests/test_ppo_ref.py measures them (tables in that module's docstring), rounded up to two digits. torch's CPU float32
# kernels differ from processor to processor even on one thread: each figure is the largest seen on two machines.
FLOOR_STEP = dict(grad=6.7e-06, exp_avg=7.0e-06, exp_avg_sq=6.2e-06, params=2.1e-06, norm=8.7e-08, pg_loss=4.5e-04,
                  value_loss=6.0e-07, entropy_loss=2.0e-07, approx_kl=5.4e-04, loss=9.7e-05, grad_norm=1.1e-06, clip_coef=1.1e-06)
# (measured on the epoch's logged MEANS of the loss statistics: pg_loss 2.6e-05, value_loss 1.2e-07, entropy_loss 4.5e-08,
#  approx_kl 5.9e-07, loss 2.0e-07. The device's chains are compared step by step, and a chain's step is a single step from
#  a slightly different state: those five columns take the single-step floor.)
FLOOR_CHAIN = dict(grad=2.7e-06, exp_avg=7.1e-07, exp_avg_sq=1.1e-06, params=5.6e-08, norm=1.4e-07,
                   grad_norm=2.3e-07, clip_coef=1.6e-07,
                   **{q: FLOOR_STEP[q] for q in ("pg_loss", "value_loss", "entropy_loss", "approx_kl", "loss")})


def _tolerances(floor, ceiling):
    return {q: min(ceiling[q], max(8.0 * floor[q], 4.0 * ULP)) for q in ceiling}


TOL_STEP, TOL_CHAIN = _tolerances(FLOOR_STEP, CEILING_STEP), _tolerances(FLOOR_CHAIN, CEILING_CHAIN)
# Explained arithmetic, allowed up to the ceiling: every kernel forms Adam's `1.f - beta2` in fp32 -- 1 - 0.999f =
# 0.99998713e-3, 1.29e-5 low relative to the 1e-3 torch rounds from double -- so EVERY element of exp_avg_sq is 1.29e-5 low
# (1.43e-5 measured on the chains with the gradient's own error on top; sqrt(v) is 6.4e-6 low, the step as much larger). A
# bias shared by all forms and far below the 10 % errors these tests are for; the float32 oracle does not have it, so its
# floor cannot cover it. (TOL_STEP's exp_avg_sq is at the ceiling through its floor already.)
EXPLAINED = ("exp_avg_sq",)
for _q in EXPLAINED:
    TOL_CHAIN[_q] = CEILING_CHAIN[_q]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def build(case: Case):
    """(oracle policy, host rollout) of `case`: time-major float32 arrays and the permutations (`perm[0]` is the epoch's)."""
    from tests.test_ppo_tower_split_gpu import _host_inputs
    return _host_inputs(case.D, case.A, case.discrete, case.norm, case.T, case.n, H=case.H, seed=case.seed)


def flat(tensors) -> th.Tensor:
    return th.cat([t.detach().reshape(-1) for t in tensors])


def block_sizes(pol) -> List[int]:
    """Element counts of the parameter blocks in `pol.parameters()` order -- `pol_offsets`' order (12 blocks for a Discrete
    head: no log_std)."""
    return [p.numel() for p in pol.parameters()]


def block_names(pol) -> List[str]:
    names = ["pW1", "pb1", "pW2", "pb2", "vW1", "vb1", "vW2", "vb2", "aW", "ab", "cW", "cb"]
    return (["log_std"] if hasattr(pol, "log_std") else []) + names


# ---- state and steps ----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class State:
    """Everything a minibatch step reads and writes, float64 (count: int). `step`: optimiser steps taken so far."""
    P: th.Tensor
    m: th.Tensor
    v: th.Tensor
    nm: Optional[th.Tensor]
    nv: Optional[th.Tensor]
    nc: int
    step: int = 0


@dataclasses.dataclass
class Step:
    grad: th.Tensor          # flat RAW gradient of the mean loss over the minibatch's rows (before clip_grad_norm_)
    total_norm: float
    clip_coef: float
    stats: np.ndarray        # STAT_NAMES
    state: State             # after the step
    ratio_margin: float      # min over rows of the ratio's distance to 1 - clip_range and 1 + clip_range
    block_scale: float       # min over the parameter blocks of max |g| in the block / max |g| overall
    rows: int


class Reference:
    def __init__(self, case: Case, pol, host: dict, max_grad_norm: float):
        self.case, self.max_grad_norm = case, float(max_grad_norm)
        self.pol = copy.deepcopy(pol).double()
        self.pol.optimizer = None
        self.sizes, self.names = block_sizes(pol), block_names(pol)
        # env-major rows, as `RolloutBuffer.swap_and_flatten` orders them: row = env * T + t
        rows = lambda a: th.as_tensor(np.ascontiguousarray(np.swapaxes(a, 0, 1).reshape(case.rows, -1))).double()
        self.obs, self.act = rows(host["obs"]), rows(host["act"])
        self.lp, self.adv, self.ret = (rows(host[k]).flatten() for k in ("lp", "adv", "ret"))
        self.perm = np.asarray(host["perm"][0])
        self.initial = self._read_state(pol)

    def _read_state(self, pol) -> State:
        P = flat(pol.parameters()).double()
        if self.case.norm:
            rn = pol.features_extractor.normalize
            return State(P, th.zeros_like(P), th.zeros_like(P), rn.running_mean.double().clone(), rn.running_var.double().clone(),
                         int(rn.count))
        return State(P, th.zeros_like(P), th.zeros_like(P), None, None, 0)

    def minibatch(self, mb: int) -> np.ndarray:
        return self.perm[mb * self.case.bs:(mb + 1) * self.case.bs]

    def step_from(self, state: State, mb: Optional[int] = None) -> Step:
        """One step from `state` on minibatch `mb` of the epoch (default: the one that follows `state.step` steps)."""
        case, pol = self.case, self.pol
        idx = self.minibatch(state.step if mb is None else mb)
        with th.no_grad():
            th.nn.utils.vector_to_parameters(state.P.clone(), pol.parameters())
            if case.norm:
                rn = pol.features_extractor.normalize
                rn.running_mean.copy_(state.nm)
                rn.running_var.copy_(state.nv)
                rn.count.fill_(state.nc)
        pol.train(True)
        pol.zero_grad()
        obs, lp_old, adv, ret = self.obs[idx], self.lp[idx], self.adv[idx], self.ret[idx]
        actions = self.act[idx].long().flatten() if case.discrete else self.act[idx]
        # `evaluate_actions` without `preprocess_obs`
        latent_pi, latent_vf = pol.mlp_extractor(pol.features_extractor(obs))
        dist = pol._get_action_dist_from_latent(latent_pi)
        log_prob, entropy = dist.log_prob(actions), dist.entropy()
        values = pol.value_net(latent_vf).flatten()
        if case.normalize_adv and len(adv) > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = th.exp(log_prob - lp_old)
        pg_loss = -th.min(adv * ratio, adv * th.clamp(ratio, 1 - CLIP_RANGE, 1 + CLIP_RANGE)).mean()
        clip_fraction = th.mean((th.abs(ratio - 1) > CLIP_RANGE).double())
        value_loss = F.mse_loss(ret, values)
        entropy_loss = -th.mean(entropy)
        loss = pg_loss + ENT_COEF * entropy_loss + VF_COEF * value_loss
        with th.no_grad():
            log_ratio = log_prob - lp_old
            approx_kl = th.mean((th.exp(log_ratio) - 1) - log_ratio)
            r = ratio.detach()
            margin = float(th.minimum((r - (1 - CLIP_RANGE)).abs(), (r - (1 + CLIP_RANGE)).abs()).min())
        loss.backward()
        g = flat(p.grad for p in pol.parameters()).clone()
        total_norm = float(g.square().sum().sqrt())
        coef = min(self.max_grad_norm / (total_norm + 1e-6), 1.0)
        t = state.step + 1
        gc = g * coef
        m = BETA1 * state.m + (1.0 - BETA1) * gc
        v = BETA2 * state.v + (1.0 - BETA2) * gc * gc
        P = state.P - (LR / (1.0 - BETA1 ** t)) * m / (v.sqrt() / (1.0 - BETA2 ** t) ** 0.5 + ADAM_EPS)
        if case.norm:
            rn = pol.features_extractor.normalize
            after = State(P, m, v, rn.running_mean.clone(), rn.running_var.clone(), int(rn.count), t)
        else:
            after = State(P, m, v, None, None, 0, t)
        stats = np.array([float(x.detach()) for x in (pg_loss, value_loss, entropy_loss, approx_kl, clip_fraction, loss)]
                         + [total_norm, coef])
        scales = [float(b.abs().max()) for b in th.split(g, self.sizes)]
        return Step(g, total_norm, coef, stats, after, margin, min(scales) / max(scales), len(idx))

    def chain(self, state: State, k: int) -> List[Step]:
        """`k` consecutive steps, float64 state carried from one to the next."""
        out = []
        for _ in range(k):
            out.append(self.step_from(state))
            state = out[-1].state
        return out


def clip_and_adam(grad: th.Tensor, state: State, max_grad_norm: float):
    """float64 `clip_grad_norm_` + Adam step `state.step + 1` on a GIVEN gradient (the device's own, for the `_apply`
    entry): (total_norm, clip_coef, m, v, P)."""
    g = grad.detach().cpu().double()
    total_norm = float(g.square().sum().sqrt())
    coef = min(max_grad_norm / (total_norm + 1e-6), 1.0)
    t = state.step + 1
    gc = g * coef
    m = BETA1 * state.m + (1.0 - BETA1) * gc
    v = BETA2 * state.v + (1.0 - BETA2) * gc * gc
    P = state.P - (LR / (1.0 - BETA1 ** t)) * m / (v.sqrt() / (1.0 - BETA2 ** t) ** 0.5 + ADAM_EPS)
    return total_norm, coef, m, v, P


def assert_guards(steps: Sequence[Step], clipped: bool, max_grad_norm: float, what: str = "", ratio: bool = True) -> None:
    """`ratio=False`: only for a comparison that does not involve `clip_fraction` (the 2 048-row sensitivity shape, where no
    seed among the first 1 500 keeps every ratio 1e-3 away from the bounds)."""
    for k, s in enumerate(steps):
        assert not ratio or s.ratio_margin >= RATIO_MARGIN, (f"{what} step {k}: a ratio at {s.ratio_margin:.3g} of a clip bound: the clip "
                                                f"indicator may switch in fp32 -- pick another seed")
        assert s.block_scale >= MIN_BLOCK_SCALE, (f"{what} step {k}: a parameter block's gradient is {s.block_scale:.3g} of the "
                                                  f"largest: a nearly cancelled sum -- pick another seed")
        if clipped:
            assert s.total_norm >= NORM_MARGIN * max_grad_norm, (f"{what} step {k}: norm {s.total_norm:.4g} does not clear "
                                                                 f"{NORM_MARGIN} x {max_grad_norm}: not a clipped case")


def clipped_rows(clip_fraction: float, rows: int) -> int:
    """The number of rows beyond the clip range, from a `clip_fraction` in any precision: what "exact" compares."""
    k = round(float(clip_fraction) * rows)
    # (a float32 k / rows times rows is within rows x 2^-23 of k: 2.5e-4 at 2 048 rows)
    assert abs(float(clip_fraction) * rows - k) < 1e-3, "not a whole number of rows"
    return k


# ---- deviations -----------------------------------------------------------------------------------------------------------------
def _d(t) -> th.Tensor:
    return t.detach().cpu().double() if isinstance(t, th.Tensor) else th.as_tensor(np.asarray(t)).double()


def block_deviation(x, ref, sizes: Sequence[int]) -> List[float]:
    """max |x - ref| / max |ref| per parameter block."""
    x, ref = _d(x).flatten(), _d(ref).flatten()
    assert x.numel() == ref.numel() == sum(sizes)
    out, off = [], 0
    for s in sizes:
        scale = float(ref[off:off + s].abs().max())
        assert scale > 0.0, "a reference block is all zero: nothing to normalise by"
        out.append(float((x[off:off + s] - ref[off:off + s]).abs().max()) / scale)
        off += s
    return out


def deviations(got: dict, ref: Step, sizes: Sequence[int]) -> Dict[str, float]:
    """Deviation of every quantity `got` holds from the reference step, in the measures of the module docstring. Keys of
    `got`: grad, exp_avg, exp_avg_sq, params, stats (8 values), nm, nv (any subset; nm and nv together)."""
    want = dict(grad=ref.grad, exp_avg=ref.state.m, exp_avg_sq=ref.state.v)
    out = {}
    for q in VECTORS:
        if q in got:
            out[q] = max(block_deviation(got[q], want[q], sizes))
    if "params" in got:
        out["params"] = float(((_d(got["params"]) - ref.state.P).abs() / (1.0 + ref.state.P.abs())).max())
    if "stats" in got:
        st = _d(got["stats"]).flatten()
        for j, name in enumerate(STAT_NAMES):
            if name != "clip_fraction":
                out[name] = abs(float(st[j]) - ref.stats[j]) / abs(ref.stats[j])
    if "nm" in got and ref.state.nm is not None:
        out["norm"] = max(float(((_d(got[k]) - w).abs() / (1.0 + w.abs())).max())
                          for k, w in (("nm", ref.state.nm), ("nv", ref.state.nv)))
    return out


# ---- the float32 oracle ----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class OracleRun:
    grads: List[th.Tensor]       # raw float32 gradient of every step (read before clip_grad_norm_ scales it)
    norms: List[float]           # what clip_grad_norm_ returned
    P: th.Tensor
    m: th.Tensor
    v: th.Tensor
    logged: Dict[str, float]
    nm: Optional[th.Tensor]
    nv: Optional[th.Tensor]
    nc: int


def run_oracle(case: Case, pol, host: dict, max_grad_norm: float,
               tamper: Optional[Callable[[int, object, int], None]] = None) -> OracleRun:
    """One epoch of `sb3_restated.PPO.train` (float32, CPU) on `pol` -- which it trains in place --, set up as
    `test_ppo_epochs_match_oracle` sets it up. `tamper(step, policy, rows)` may change the `.grad`s of a step after
    backward and before clip_grad_norm_ (the sensitivity test's injected errors)."""
    from imitation_amd import spaces
    from oracle import sb3_restated as sb
    os_ = spaces.Box(-np.inf, np.inf, (case.D,), np.float32)
    as_ = spaces.Discrete(case.A) if case.discrete else spaces.Box(-1, 1, (case.A,), np.float32)
    algo = sb.PPO(sb.ActorCriticPolicy, None, n_steps=case.T, batch_size=case.bs, n_epochs=1, ent_coef=ENT_COEF,
                  vf_coef=VF_COEF, clip_range=CLIP_RANGE, max_grad_norm=max_grad_norm,
                  normalize_advantage=case.normalize_adv, _init_setup_model=False)
    algo.observation_space, algo.action_space, algo.n_envs = os_, as_, case.n
    algo.policy = pol
    algo.lr_schedule = sb.constant_fn(LR)
    algo.clip_range = sb.constant_fn(CLIP_RANGE)
    algo._logger = sb.Logger(None, [])
    buf = sb.RolloutBuffer(case.T, os_, as_, gamma=0.99, gae_lambda=0.95, n_envs=case.n)
    buf.observations[:] = host["obs"]
    buf.actions[:] = host["act"]
    buf.log_probs[:], buf.advantages[:], buf.returns[:] = host["lp"], host["adv"], host["ret"]
    buf.values[:] = host["ret"] - host["adv"]
    buf.full = True
    algo.rollout_buffer = buf
    grads, norms = [], []
    real_clip = th.nn.utils.clip_grad_norm_

    def recording_clip(parameters, max_norm, *a, **k):
        parameters = list(parameters)
        step = len(grads)
        if tamper is not None:
            tamper(step, pol, min(case.bs, case.rows - step * case.bs))
        grads.append(flat(p.grad for p in parameters).clone())
        norms.append(float(real_clip(parameters, max_norm, *a, **k)))
        return norms[-1]

    th.nn.utils.clip_grad_norm_ = recording_clip
    try:
        np.random.seed(123)
        algo.train()
    finally:
        th.nn.utils.clip_grad_norm_ = real_clip
    st = pol.optimizer.state
    params = list(pol.parameters())
    rn = pol.features_extractor.normalize if case.norm else None
    return OracleRun(grads, norms, flat(params), flat(st[p]["exp_avg"] for p in params), flat(st[p]["exp_avg_sq"] for p in params),
                     dict(algo.logger.name_to_value), rn.running_mean.clone() if rn else None,
                     rn.running_var.clone() if rn else None, int(rn.count) if rn else 0)
