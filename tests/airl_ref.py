"""Float64 reference of ONE AIRL discriminator update of the shaped reward net, with no GPU in it: what
`tests/test_airl_ref.py` (any machine) and `tests/test_airl_fused_gpu.py` (`-m gpu`) compare against.

The forward pass is `oracle.imitation_restated.BasicShapedRewardNet` itself (pinned to the reference project by
`tests/test_oracle_pinning.py`), converted with `.double()` and loaded from the HIP net's `state_dict()` -- parameters and
the running mean / variance / count of both input norms. Nothing here restates `g + gamma (1 - d) h(s') - h(s)`: the
module's `forward` is called, torch autograd differentiates it, forward hooks read the hidden pre-activations and the
norm state after every evaluation (base, potential on s', potential on s: `rewards/reward_nets.py:708-710`).

Case data: expert / generator tables of at most 64 transitions, index vectors drawn with repetition up to the case's
row count (few distinct rows -> few distinct pre-activations, so the input conditions of `conditions()` can be met at
4100 rows), log pi drawn uniformly from [-12, 3] per row.

Deviation measures (`deviations`) -- the SAME expressions give the float32-against-float64 noise floor on the CPU and
the figures the GPU tests assert on:
    logits   max_i |dx_i| / (1 + |x_i|)                      norm   max |dv| / (1 + |v|) over mean, variance (, EMA rate)
    loss     |d| / max(1, |loss|)      entropy  |d| / max(1, |H|)      grad   max |dg| / max |g_ref|
"""
from __future__ import annotations

import copy
import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch as th
from torch import nn

from imitation_amd import networks, reward_nets, spaces
from oracle import imitation_restated as O


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    od: int
    ad: int
    discrete: bool
    flags: Tuple[int, int, int, int]      # use_state, use_action, use_next_state, use_done
    n_expert: int
    n_gen: int
    norm: Optional[str]                   # "running", "ema" or None
    gamma: float
    scale: float
    seed: int                             # chosen on the CPU so that `conditions()` holds (tests/test_airl_ref.py)
    all_done: bool = False                # every transition terminal: d h(s') == 0
    saturate: bool = False                # log pi = -40 on the first half of each group, +40 on the rest
    reward_hid: Tuple[int, ...] = (32,)
    potential_hid: Tuple[int, ...] = (32, 32)

    @property
    def R(self) -> int:
        return self.n_expert + self.n_gen

    @property
    def Db(self) -> int:
        f = self.flags
        return f[0] * self.od + f[1] * self.ad + f[2] * self.od + f[3]


# What each case reaches in csrc/airl_fused.hip is in tests/test_airl_fused_gpu.py's docstring.
CASES: Dict[str, Case] = {c.name: c for c in [
    Case("1_baseline", 11, 3, False, (1, 1, 0, 0), 33, 31, "running", 0.99, 1.0, seed=0),
    Case("2_one_by_one", 1, 1, False, (0, 0, 0, 1), 1, 1, None, 0.99, 1.0, seed=0),
    Case("3_discrete_129", 4, 2, True, (1, 1, 0, 0), 65, 64, "running", 0.99, 0.5, seed=0),
    Case("4_db64_385", 29, 6, False, (1, 1, 1, 0), 193, 192, "running", 0.99, 1.0, seed=1),
    Case("5_dp64", 64, 3, False, (0, 1, 0, 0), 64, 65, None, 0.9, 1.0, seed=0),
    Case("6_dp33_gamma1", 33, 2, False, (1, 1, 0, 0), 100, 93, "running", 1.0, 1.0, seed=0),
    Case("7_done_gamma0", 12, 4, False, (1, 1, 1, 1), 40, 40, "running", 0.0, 1.0, seed=0),
    Case("8_33_workgroups", 11, 3, False, (1, 1, 0, 0), 2050, 2050, "running", 0.99, 1.0, seed=2),
    Case("9_all_done", 11, 3, False, (1, 1, 0, 0), 33, 31, "running", 0.99, 1.0, seed=1, all_done=True),
    Case("10_saturated", 11, 3, False, (1, 1, 0, 0), 33, 31, "running", 0.99, 1.0, seed=0, saturate=True),
    # geometries the fused update refuses: the stack-by-stack path only
    Case("hid64", 11, 3, False, (1, 1, 0, 0), 33, 31, "running", 0.99, 1.0, seed=0, reward_hid=(64,),
         potential_hid=(64, 64)),
    Case("ema", 11, 3, False, (1, 1, 0, 0), 33, 31, "ema", 0.99, 1.0, seed=0),
]}
FUSED_CASES = [n for n in CASES if n[0].isdigit()]
STACKS_ONLY_CASES = ["hid64", "ema"]

N_UPDATES = 2
N_WARM = 77                # rows of the earlier batch that makes count / mean / variance non-trivial
MIN_ABS_LOGIT = 1e-4       # no reference logit nearer to 0: the four count statistics are exact
MIN_ABS_PREACT = 1e-5      # no hidden pre-activation nearer to 0: no ReLU may switch between fp32 and fp64

ULP = 2.0 ** -23
# Ceilings: what tests/test_disc_fused_gpu.py uses for the same quantity, in the measures of `deviations`
# (logits rtol 1e-5 / atol 2e-5; loss 1e-5; entropy 1e-4; gradient atol 2e-5 max(1, max|g|); norm rtol 1e-5 / atol 1e-6).
CEILING = dict(logits=1e-5, loss=1e-5, entropy=1e-4, grad=2e-5, norm=1e-6)
# Worst float32-against-float64 deviation of the oracle module over all cases and both updates, as
# tests/test_airl_ref.py measures it; per case in that module's docstring. torch's CPU float32 sums depend on the
# machine (thread count, BLAS blocking): the worst figure seen on either of two machines is kept (gradient: 5.5e-7 at
# 4100 rows on a 16-thread host against 1.5e-7 on the other).
FLOOR = dict(logits=1.4e-7, loss=1.2e-7, entropy=3.4e-7, grad=5.5e-7, norm=1.3e-7)
# 8 x the floor (the kernels sum the same fp32 terms in another order: 32-row waves, 128-row slabs, split-K), at least
# four fp32 ulps of the quantity's scale, at most the ceiling.
TOL = {q: min(CEILING[q], max(8.0 * FLOOR[q], 4.0 * ULP)) for q in CEILING}
ADAM_ATOL, ADAM_RTOL = 1e-7, 1e-6   # float64 Adam fed the kernel's own gradients: only fp32 sqrt and one division differ


# ---- nets ---------------------------------------------------------------------------------------------------------------
def make_nets(case: Case):
    """(HIP net on the CPU -- a plain state holder until `.to("cuda")` --, float64 oracle loaded from its state_dict)."""
    osp = spaces.Box(-np.inf, np.inf, (case.od,), np.float32)
    asp = spaces.Discrete(case.ad) if case.discrete else spaces.Box(-1, 1, (case.ad,), np.float32)
    kw = dict(reward_hid_sizes=case.reward_hid, potential_hid_sizes=case.potential_hid, use_state=bool(case.flags[0]),
              use_action=bool(case.flags[1]), use_next_state=bool(case.flags[2]), use_done=bool(case.flags[3]),
              discount_factor=case.gamma)
    hip_norm = {"running": networks.RunningNorm, "ema": networks.EMANorm, None: None}[case.norm]
    ref_norm = {"running": O.RunningNorm, "ema": O.EMANorm, None: None}[case.norm]
    th.manual_seed(case.seed)
    net = reward_nets.BasicShapedRewardNet(osp, asp, **kw, **({"normalize_input_layer": hip_norm} if hip_norm else {}))
    oracle = O.BasicShapedRewardNet(osp, asp, **kw, **({"normalize_input_layer": ref_norm} if ref_norm else {})).double()
    load_oracle(oracle, net.state_dict())
    return net, oracle


def load_oracle(oracle: nn.Module, state_dict) -> None:
    """Parameters and norm buffers of the HIP net into the oracle (strict: the key sets must be equal)."""
    oracle.load_state_dict({k: v.detach().cpu() for k, v in state_dict.items()}, strict=True)


def float32_twin(oracle: nn.Module) -> nn.Module:
    return copy.deepcopy(oracle).float()


def norm_modules(oracle: nn.Module) -> List[O.RunningNorm]:
    """[base input norm, potential input norm] of the oracle, or [] without input normalisation."""
    return [m for m in oracle.modules() if isinstance(m, O.RunningNorm)]


def norm_state(m) -> Dict[str, th.Tensor]:
    """Floating-point statistics and the sample count of an input norm (the oracle's module or the HIP state holder)."""
    out = dict(mean=m.running_mean, var=m.running_var, count=m.count)
    if hasattr(m, "inv_learning_rate"):
        out["inv_learning_rate"] = m.inv_learning_rate
    return {k: v.detach().cpu().clone() for k, v in out.items()}


# ---- case data ------------------------------------------------------------------------------------------------------------
def make_data(case: Case) -> dict:
    """Tables (host arrays, <= 64 rows each), warm-up batches for the two norms, and per update the index draws and
    log pi. Deterministic in `case.seed`."""
    g = np.random.default_rng(1000 + case.seed)

    def table(n):
        obs = g.standard_normal((n, case.od)).astype(np.float32) * 1.7 + 0.3
        nxt = g.standard_normal((n, case.od)).astype(np.float32)
        acts = (g.integers(0, case.ad, n).astype(np.int64) if case.discrete
                else g.uniform(-1, 1, (n, case.ad)).astype(np.float32))
        dones = np.ones(n, np.uint8) if case.all_done else (g.random(n) < 0.3).astype(np.uint8)
        return dict(obs=obs, acts=acts, next_obs=nxt, dones=dones)

    data = dict(expert=table(64), gen=table(61),
                warm_base=g.standard_normal((N_WARM, case.Db)).astype(np.float32) * 0.5 + 0.2,
                warm_pot=g.standard_normal((N_WARM, case.od)).astype(np.float32) * 0.5 + 0.2, updates=[])
    for _ in range(N_UPDATES):
        logp = g.uniform(-12.0, 3.0, case.R).astype(np.float32)
        if case.saturate:
            for lo, n in ((0, case.n_expert), (case.n_expert, case.n_gen)):
                logp[lo:lo + n // 2] = -40.0
                logp[lo + n // 2:lo + n] = 40.0
        data["updates"].append(dict(e_idx=g.integers(0, 64, case.n_expert), g_idx=g.integers(0, 61, case.n_gen), logp=logp))
    return data


def gathered(case: Case, data: dict, u: int, dtype=th.float64):
    """The gathered batch (s, a, s', done, log pi) of update `u`: expert rows first. Discrete actions one-hot."""
    upd = data["updates"][u]
    cols = {}
    for k in ("obs", "acts", "next_obs", "dones"):
        cols[k] = np.concatenate([data["expert"][k][upd["e_idx"]], data["gen"][k][upd["g_idx"]]])
    a = np.eye(case.ad, dtype=np.float32)[cols["acts"]] if case.discrete else cols["acts"]
    t = lambda x: th.as_tensor(np.ascontiguousarray(x)).to(dtype)
    return t(cols["obs"]), t(a), t(cols["next_obs"]), t(cols["dones"]), t(upd["logp"])


def base_inputs(case: Case, batch) -> th.Tensor:
    """[s | a | s' | done] as flagged: the rows the base stack reads (for the direct calls' assembled buffers)."""
    s, a, ns, d, _ = batch
    parts = [x for x, f in zip((s, a, ns, d[:, None]), case.flags) if f]
    return th.cat(parts, dim=1)


# ---- the reference update ---------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Ref:
    x: th.Tensor                   # logits f - log pi
    loss: float                    # scale * BCEWithLogits(x, y)
    grad: th.Tensor                # flat, the store's order: base stack, then potential
    stats: np.ndarray              # [scaled mean loss, correct, correct expert, correct generator, predicted generator,
                                   #  entropy sum, n_expert, n_gen] (csrc/airl_fused.hip: sc[0..5] and stats[6], stats[7])
    norms: List[Dict[str, th.Tensor]]        # [base, potential] after the update ([] without norm)
    norm_trace: List[Dict[str, th.Tensor]]   # state after each evaluation: base, potential(s'), potential(s)
    preacts: List[th.Tensor]       # hidden pre-activations, evaluation by evaluation, layer by layer


def reference_update(oracle: nn.Module, batch, n_expert: int, scale: float, train: bool = True) -> Ref:
    """One update's forward + backward on the oracle module, in the module's dtype. `train`: the norms update (base with
    the batch; potential with the next-state batch, then with the state batch) before they normalise."""
    s, a, ns, d, logp = batch
    R = s.shape[0]
    preacts: List[th.Tensor] = []
    trace: List[Dict[str, th.Tensor]] = []
    hooks = []
    for name, m in oracle.named_modules():
        if isinstance(m, nn.Linear) and not name.endswith("dense_final"):
            hooks.append(m.register_forward_hook(lambda _m, _i, out: preacts.append(out.detach().clone())))
        elif isinstance(m, O.RunningNorm):
            hooks.append(m.register_forward_hook(lambda m_, _i, _o: trace.append(norm_state(m_))))
    oracle.train(train)
    oracle.zero_grad()
    try:
        f = oracle(s, a, ns, d)
    finally:
        for h in hooks:
            h.remove()
    x = f - logp
    y = th.cat([th.ones(n_expert), th.zeros(R - n_expert)]).to(x.dtype)
    loss = scale * nn.functional.binary_cross_entropy_with_logits(x, y)
    loss.backward()
    grad = th.cat([p.grad.reshape(-1) for p in oracle.parameters()]).detach().clone()
    xd = x.detach()
    # the counts as `compute_train_stats` (adversarial/common.py:27-92) forms them, before its divisions
    pred_gen, true_gen = xd < 0, y == 0
    correct = th.eq(pred_gen, true_gen)
    entropy = th.distributions.Bernoulli(logits=xd).entropy().sum()
    stats = np.array([float(loss.detach()), float(correct.sum()), float((correct & ~true_gen).sum()), float((correct & true_gen).sum()),
                      float(pred_gen.sum()), float(entropy), float(n_expert), float(R - n_expert)])
    return Ref(x=xd.clone(), loss=float(loss.detach()), grad=grad, stats=stats, norms=[norm_state(m) for m in norm_modules(oracle)],
               norm_trace=trace, preacts=preacts)


def conditions(ref: Ref) -> Tuple[float, float]:
    """(min |logit|, min |hidden pre-activation|) of a reference update."""
    return float(ref.x.abs().min()), min(float(z.abs().min()) for z in ref.preacts)


def assert_conditions(ref: Ref, what: str = "") -> None:
    min_x, min_z = conditions(ref)
    assert min_x >= MIN_ABS_LOGIT, f"{what}: a reference logit at {min_x:.3g} of 0: the count statistics are not exact"
    assert min_z >= MIN_ABS_PREACT, f"{what}: a hidden pre-activation at {min_z:.3g} of 0: a ReLU may switch in fp32"


def deviations(logits, loss, entropy, grad, norms: Sequence[Dict[str, th.Tensor]], ref: Ref) -> Dict[str, float]:
    """Deviation of each quantity from the reference, in the measures of the module docstring."""
    d = lambda t: t.detach().cpu().double()
    out = dict(logits=float(((d(logits) - ref.x.double()).abs() / (1.0 + ref.x.double().abs())).max()),
               loss=abs(float(loss) - ref.stats[0]) / max(1.0, abs(ref.stats[0])),
               entropy=abs(float(entropy) - ref.stats[5]) / max(1.0, abs(ref.stats[5])),
               grad=float((d(grad) - ref.grad.double()).abs().max() / ref.grad.double().abs().max()), norm=0.0)
    assert len(norms) == len(ref.norms)
    for got, want in zip(norms, ref.norms):
        for k, w in want.items():
            if k != "count":
                out["norm"] = max(out["norm"], float(((d(got[k]) - w.double()).abs() / (1.0 + w.double().abs())).max()))
    return out


# ---- Adam in float64 ----------------------------------------------------------------------------------------------------------
def adam_steps(params0: th.Tensor, grads: Sequence[th.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
    """`torch.optim.Adam` (no weight decay, no amsgrad) on one flat float64 vector, one step per gradient of `grads`
    starting from zero moments. Returns (parameters, exp_avg, exp_avg_sq)."""
    b1, b2 = betas
    p = params0.detach().cpu().double().clone()
    m, v = th.zeros_like(p), th.zeros_like(p)
    for t, g in enumerate(grads, start=1):
        g = g.detach().cpu().double()
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        p = p - (lr / (1.0 - b1 ** t)) * m / (v.sqrt() / (1.0 - b2 ** t) ** 0.5 + eps)
    return p, m, v
