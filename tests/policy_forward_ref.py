"""Float64 reference of the policy forward kernels of csrc/policy.hip (`ia_policy_act`, `ia_policy_evaluate`,
`ia_policy_logits`: [SB3 ActorCriticPolicy.forward / evaluate_actions / predict_values] as `oracle.sb3_restated` restates
them), with no GPU in it: what `tests/test_policy_forward_ref.py` (any machine) and `tests/test_policy_forward_gpu.py`
(`-m gpu`) compare against.

The forward pass is the oracle's own `ActorCriticPolicy` (`tests/test_kernels_gpu._oracle_policy`: its feature norm, both
tanh towers, the DiagGaussian or Categorical head), deep-copied, converted with `.double()` and fed float64 rows, as
`tests/ppo_ref.py` does it; the only call left out is `preprocess_obs`, whose `obs.float()` would round the rows back to
float32 (they ARE float32 values). `run` computes, for one policy in one precision: the first-layer pre-activations of both
towers (for the guards), the head output (means / logits), the values, and
    Gaussian:  sample = mu + noise * exp(log_std), log-prob of that sample, log-prob of GIVEN actions, entropy;
    Discrete:  probabilities and CDF, the inverse-CDF pick of every row's uniform (the first action whose CDF exceeds u, the
               last action when none does), the mode (arg-max, the lowest index of a tie), the log-prob of both picks and of
               GIVEN actions, entropy.
The same `run` on the float32 policy is "the float32 oracle" whose deviation from the reference is the noise floor.

Cases (`CASES`): 130 rows each (three 64-row workgroups, the last of 2 rows); `GRID_CASES`: for H = 32 and H = 64 the
observation widths 1, 3, 4, 5, 16, 17, 33, 63, 64 paired with the action widths 1, 2, 13, 15, 16, the head kind and the
feature norm alternating (a pair that is Gaussian at H = 32 is Discrete at H = 64), the corner (64, 16) with both heads, and
(5, 16), (33, 15), (64, 1). A Gaussian case clips to [-1, 1], to per-dimension asymmetric bounds or to (-inf, +inf)
(`bounds`). Three conditioned cases:
    small      (17, 6) Gaussian, H = 32, norm: W1 and b1 of both towers scaled by `SMALL_SCALE`, so that at least 90 % of
               the first-layer pre-activations have |x| <= 0.1 (fast_tanh's polynomial branch; the second layer's are then
               small too). W2 and the heads stay as they are: scaled as well, the outputs would shrink under the absolute
               part of the deviation measure and a wrong polynomial would not show.
    saturated  (17, 6) Gaussian, H = 32, norm with running_var = 0 on every third column (division by sqrt(eps)); the
               observations of those columns lie within a few hundredths of the running mean, so that at least 25 % of the
               first-layer pre-activations have |x| >= 4 and at least 25 % do not (the rows still matter).
    tie        (20, 13) Discrete, H = 64: rows `TIE_ROWS` of the action head's weight and bias are identical and raised above
               the others, so two logits are bit-equal on the device and the mode must be the lower index on every row.

Guards (`assert_guards`), conditions on the float64 run, never measurements; each case's seed (`SEEDS`: those that are not
0) was picked on the CPU so that EVERY row meets them -- no row is ever left out:
  * sampling: no row's u lies within `CDF_MARGIN` = 1e-5 of a float64 CDF boundary (the boundaries below the last: at or above
    the last one the pick is the last action whether or not a float32 CDF reaches u);
  * placed rows: row 0 has u = 0 and picks action 0; row 1 has u = 1 - 2**-24 and picks A - 1 (with the margin above, the
    last boundary is its only candidate);
  * mode: the top logit clears the next by `LOGIT_MARGIN` = 1e-4 (tie: the tied pair clears the third);
  * the conditioned cases' fractions above.

Deviation measure (`deviation`, `deviations`) -- the SAME expression gives the float32-against-float64 noise floor on the
CPU and the figures the GPU tests assert on: max |dx| / (1 + |ref|) per quantity (head, actions, values, logp, entropy;
`logp` takes every log-prob there is: of the sample, of given actions, of both picks); a value that is not finite deviates
by inf. Discrete picks are compared exactly by the callers.

Tolerances: `TOL[q] = min(CEILING[q], max(8 * FLOOR[q], 4 * ULP))`, as `ppo_ref._tolerances`. `FLOOR`: the worst deviation
of the float32 oracle from this reference over all cases, as `tests/test_policy_forward_ref.py` measures it (table in its
docstring). The saturated case needs no floor of its own: its columns divided by sqrt(eps) hold observations close to the
running mean, obs - mean is exact there, and the float32 oracle is as close to float64 as on any other case (a kernel that
formed obs / sd - mean / sd instead would be 316 times the rounding of obs off, far outside). `CEILING`:
`test_policy_act_and_evaluate`'s rtol 1e-4.
"""
from __future__ import annotations

import copy
import dataclasses
from typing import Dict, List, Optional

import numpy as np
import torch as th
from torch import nn

ROWS = 130
CDF_MARGIN = 1e-5
LOGIT_MARGIN = 1e-4
SMALL_SCALE = 1.0 / 32.0
TIE_ROWS = (4, 9)
QUANTITIES = ("head", "actions", "values", "logp", "entropy")
# field of `Out` -> the quantity it is measured as
FIELDS = dict(head="head", values="values", sample="actions", logp_sample="logp", logp_given="logp", logp_pick="logp",
              logp_mode="logp", entropy="entropy")
U_LAST = float(np.float32(1.0) - np.float32(2.0 ** -24))     # the largest float32 below 1


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    D: int
    A: int
    H: int
    discrete: bool
    norm: bool
    kind: str = "grid"            # grid | small | saturated | tie
    bounds: str = "unit"          # unit | asym | inf (Gaussian heads)
    n: int = ROWS
    seed: int = 0                 # of the inputs' generator; chosen so that `assert_guards` holds


# Seeds other than 0, found by `python -m tests.test_policy_forward_ref seeds` (the first seed at which every row meets the
# guards).
SEEDS: Dict[str, int] = {
}

CASES: Dict[str, Case] = {}


def _add(D, A, H, discrete, norm, kind="grid", bounds="unit") -> str:
    name = f"{D}x{A}{'d' if discrete else 'b'}_h{H}_{'norm' if norm else 'plain'}"
    if kind != "grid":
        name = f"{kind}_{name}"
    assert name not in CASES
    CASES[name] = Case(name, D, A, H, bool(discrete), bool(norm), kind, "unit" if discrete else bounds, ROWS, SEEDS.get(name, 0))
    return name


WIDTHS_D = (1, 3, 4, 5, 16, 17, 33, 63, 64)
WIDTHS_A = (1, 2, 13, 15, 16)
GRID_CASES: List[str] = []
for _hi, _H in enumerate((32, 64)):
    _pairs = [(d, WIDTHS_A[i % len(WIDTHS_A)]) for i, d in enumerate(WIDTHS_D)] + [(5, 16), (33, 15), (64, 1)]
    for _i, (_D, _A) in enumerate(_pairs):
        GRID_CASES.append(_add(_D, _A, _H, (_i + _hi) % 2 == 1, (_i // 2 + _hi) % 2 == 0, bounds=("unit", "asym", "inf")[_i % 3]))
    GRID_CASES.append(_add(64, 16, _H, False, _hi == 0, bounds="asym"))
    GRID_CASES.append(_add(64, 16, _H, True, _hi == 1))
SMALL_CASE = _add(17, 6, 32, False, True, kind="small", bounds="inf")
SATURATED_CASE = _add(17, 6, 32, False, True, kind="saturated", bounds="asym")
TIE_CASE = _add(20, 13, 64, True, False, kind="tie")
CONDITIONED_CASES = [SMALL_CASE, SATURATED_CASE, TIE_CASE]

ULP = 2.0 ** -23
CEILING = {q: 1e-4 for q in QUANTITIES}      # `test_policy_act_and_evaluate`'s rtol
# Worst float32-oracle-against-float64 deviation over all cases, as tests/test_policy_forward_ref.py measures it (table in
# that module's docstring), rounded up to two digits. torch's CPU float32 kernels differ with the processor's vector width and
# the thread count (which also moves the policy's orthogonal initialisation in its last bits): each figure is the largest
# seen on two machines, over one, four and sixteen threads and the AVX2 and AVX-512 kernels.
FLOOR = dict(head=4.3e-07, actions=4.5e-07, values=5.0e-07, logp=3.2e-07, entropy=2.5e-07)


def _tolerances(floor, ceiling):
    return {q: min(ceiling[q], max(8.0 * floor[q], 4.0 * ULP)) for q in ceiling}


TOL = _tolerances(FLOOR, CEILING)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def build(case: Case):
    """(float32 oracle policy in evaluation mode, inputs) of `case`. Inputs, float32 tensors: obs [n, D]; Gaussian: noise
    [n, A], given [n, A] (actions to score), low and high [A]; Discrete: u [n] (rows 0 and 1 placed), given [n] (indices)."""
    from tests.test_kernels_gpu import _oracle_policy
    D, A, n = case.D, case.A, case.n
    pol = _oracle_policy(D, A, case.H, case.discrete, case.norm)
    pol.set_training_mode(False)
    g = th.Generator().manual_seed(7000 + case.seed)
    obs = th.randn(n, D, generator=g)
    with th.no_grad():
        if case.kind == "small":
            for tower in (pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net):
                tower[0].weight.mul_(SMALL_SCALE)
                tower[0].bias.mul_(SMALL_SCALE)
        elif case.kind == "saturated":
            rn = pol.features_extractor.normalize
            cols = th.arange(0, D, 3)
            rn.running_var[cols] = 0.0
            obs[:, cols] = rn.running_mean[cols] + 0.03 * th.randn(n, len(cols), generator=g)
        elif case.kind == "tie":
            i, j = TIE_ROWS
            pol.action_net.weight[j] = pol.action_net.weight[i]
            pol.action_net.bias[i] += 3.0
            pol.action_net.bias[j] = pol.action_net.bias[i]
    inp = dict(obs=obs)
    if case.discrete:
        u = th.rand(n, generator=g)
        u[0] = 0.0
        u[1] = U_LAST
        inp.update(u=u, given=th.randint(0, A, (n,), generator=g).float())
    else:
        a = th.arange(A, dtype=th.float32)
        low, high = {"unit": (-th.ones(A), th.ones(A)), "asym": (-0.1 - 0.2 * a, 0.05 + 0.3 * a),
                     "inf": (th.full((A,), -float("inf")), th.full((A,), float("inf")))}[case.bounds]
        inp.update(noise=th.randn(n, A, generator=g), given=th.randn(n, A, generator=g), low=low, high=high)
    return pol, inp


# ---- the forward pass, in either precision ---------------------------------------------------------------------------------------
@dataclasses.dataclass
class Out:
    """float64 numpy arrays, whatever precision they were computed in. Gaussian: sample, logp_sample; Discrete: probs, cdf,
    pick, mode (int64), logp_pick, logp_mode, cdf_margin, logit_gap, tied (per row)."""
    z1: np.ndarray                       # [2, n, H]: first-layer pre-activations of the policy and the value tower
    head: np.ndarray
    values: np.ndarray
    logp_given: np.ndarray
    entropy: np.ndarray
    sample: Optional[np.ndarray] = None
    logp_sample: Optional[np.ndarray] = None
    probs: Optional[np.ndarray] = None
    cdf: Optional[np.ndarray] = None
    pick: Optional[np.ndarray] = None
    mode: Optional[np.ndarray] = None
    logp_pick: Optional[np.ndarray] = None
    logp_mode: Optional[np.ndarray] = None
    cdf_margin: Optional[np.ndarray] = None
    logit_gap: Optional[np.ndarray] = None
    tied: Optional[np.ndarray] = None


class _CubicTanh(nn.Module):
    def forward(self, x):
        return x - x ** 3 / 3.0


VARIANTS = ("drop_last_column", "head_row", "var_without_eps", "cubic_tanh", "value_from_policy_latent")


def tampered(pol, variant: str):
    """A copy of `pol` with one of the deliberate restatement errors of the sensitivity test built into its modules (the
    two errors of the data flow are made by `run`)."""
    pol = copy.deepcopy(pol)
    with th.no_grad():
        if variant == "head_row":
            pol.action_net.weight[-1] = pol.action_net.weight[-2]
            pol.action_net.bias[-1] = pol.action_net.bias[-2]
        elif variant == "var_without_eps":
            pol.features_extractor.normalize.eps = 0.0
        elif variant == "cubic_tanh":
            for tower in (pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net):
                for k, m in enumerate(tower):
                    if isinstance(m, nn.Tanh):
                        tower[k] = _CubicTanh()
        else:
            assert variant in VARIANTS
    return pol


def inverse_cdf(cdf: np.ndarray, u: np.ndarray) -> np.ndarray:
    """The first action whose CDF exceeds u; the last action when none does."""
    hit = u[:, None] < cdf
    return np.where(hit.any(1), hit.argmax(1), cdf.shape[1] - 1)


def _np(t) -> np.ndarray:
    return t.detach().double().numpy()


def run(case: Case, pol, inp: dict, dtype, variant: Optional[str] = None) -> Out:
    """The forward pass of `pol` (already of `dtype`) on the inputs converted to `dtype`."""
    with th.no_grad():
        obs = inp["obs"].to(dtype)
        x = pol.features_extractor(obs)            # `extract_features` without `preprocess_obs`
        if variant == "drop_last_column":
            x = x.clone()
            x[:, -1] = 0.0
        mlp = pol.mlp_extractor
        z1 = th.stack([mlp.policy_net[0](x), mlp.value_net[0](x)])
        lat_pi, lat_vf = mlp(x)
        if variant == "value_from_policy_latent":
            lat_vf = lat_pi
        values = pol.value_net(lat_vf).flatten()
        head = pol.action_net(lat_pi)
        if not bool(th.isfinite(head).all()):
            # (a tampered run only -- `var` for `var + eps` divides by zero; torch's distributions refuse such parameters)
            assert variant is not None and not case.discrete
            nan = np.full(case.n, np.nan)
            return Out(_np(z1), _np(head), _np(values), nan, nan, sample=_np(head), logp_sample=nan)
        dist = pol._get_action_dist_from_latent(lat_pi)
        if not case.discrete:
            sample = head + inp["noise"].to(dtype) * pol.log_std.exp()
            return Out(_np(z1), _np(head), _np(values), _np(dist.log_prob(inp["given"].to(dtype))), _np(dist.entropy()),
                       sample=_np(sample), logp_sample=_np(dist.log_prob(sample)))
        probs = th.softmax(head, 1)
        cdf = probs.cumsum(1)
        u = inp["u"].to(dtype)
        pick = inverse_cdf(cdf.numpy(), u.numpy())
        h = _np(head)
        top = h.max(1, keepdims=True)
        tied = h >= top - 1e-9                      # (float64: equal logits may differ in the last bits of a BLAS sum)
        mode = tied.argmax(1)
        rest = np.where(tied, -np.inf, h).max(1)
        margin = np.abs(_np(u)[:, None] - _np(cdf)[:, :-1]).min(1) if case.A > 1 else np.full(case.n, np.inf)
        lp = lambda a: _np(dist.log_prob(th.as_tensor(a).long()))
        return Out(_np(z1), h, _np(values), lp(inp["given"]), _np(dist.entropy()), probs=_np(probs), cdf=_np(cdf), pick=pick,
                   mode=mode, logp_pick=lp(pick), logp_mode=lp(mode), cdf_margin=margin, logit_gap=top[:, 0] - rest,
                   tied=tied.sum(1))


def reference(case: Case, pol, inp: dict, variant: Optional[str] = None) -> Out:
    """The float64 run. `pol` (float32) is left alone."""
    p = copy.deepcopy(pol) if variant is None else tampered(pol, variant)
    p.optimizer = None
    return run(case, p.double(), inp, th.float64, variant)


def oracle(case: Case, pol, inp: dict, variant: Optional[str] = None) -> Out:
    """The float32 oracle: the same pass in torch's CPU float32."""
    return run(case, pol if variant is None else tampered(pol, variant), inp, th.float32, variant)


# ---- guards -----------------------------------------------------------------------------------------------------------------
def fraction_small(ref: Out) -> float:
    return float((np.abs(ref.z1) <= 0.1).mean())


def fraction_saturated(ref: Out) -> float:
    return float((np.abs(ref.z1) >= 4.0).mean())


def assert_guards(case: Case, ref: Out) -> None:
    what = case.name
    if case.discrete:
        assert ref.cdf_margin.min() >= CDF_MARGIN, (f"{what}: row {ref.cdf_margin.argmin()} has u within {ref.cdf_margin.min():.3g} "
                                                    f"of a CDF boundary -- pick another seed")
        assert ref.pick[0] == 0 and ref.pick[1] == case.A - 1, f"{what}: the placed rows pick {ref.pick[:2]}"
        assert ref.logit_gap.min() >= LOGIT_MARGIN, (f"{what}: row {ref.logit_gap.argmin()}: the top logit clears the next by "
                                                     f"{ref.logit_gap.min():.3g} -- pick another seed")
        if case.kind == "tie":
            assert (ref.tied == 2).all() and (ref.mode == TIE_ROWS[0]).all(), f"{what}: the tied pair is not on top of every row"
        else:
            assert (ref.tied == 1).all(), f"{what}: an unintended tie"
    if case.kind == "small":
        assert fraction_small(ref) >= 0.9, f"{what}: only {fraction_small(ref):.3f} of the pre-activations within 0.1"
    if case.kind == "saturated":
        f = fraction_saturated(ref)
        assert 0.25 <= f <= 0.75, f"{what}: {f:.3f} of the pre-activations beyond 4"


# ---- deviations -----------------------------------------------------------------------------------------------------------------
def deviation(x, ref) -> float:
    """max |x - ref| / (1 + |ref|); inf where x is not finite."""
    x = x.detach().cpu().double().numpy() if isinstance(x, th.Tensor) else np.asarray(x, np.float64)
    ref = np.asarray(ref, np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if not np.isfinite(x).all():
        return float("inf")
    return float((np.abs(x - ref) / (1.0 + np.abs(ref))).max())


def deviations(got: dict, ref: Out) -> Dict[str, float]:
    """Per quantity, the worst deviation of the fields of `Out` that `got` holds (any subset of `FIELDS`)."""
    out: Dict[str, float] = {}
    for f, x in got.items():
        q = FIELDS[f]
        out[q] = max(out.get(q, 0.0), deviation(x, getattr(ref, f)))
    return out


def fields(out: Out) -> dict:
    """The measured fields an `Out` holds: `deviations(fields(oracle run), reference)` is the floor."""
    return {f: getattr(out, f) for f in FIELDS if getattr(out, f) is not None}
