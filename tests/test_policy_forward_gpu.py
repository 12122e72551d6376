"""The policy forward kernels of csrc/policy.hip -- `ia_policy_transpose`, `ia_policy_act`, `ia_policy_evaluate` (all four
pointer combinations), `ia_policy_logits` -- against the float64 reference of `tests/policy_forward_ref.py` (`-m gpu`), on
every case of that module: both tower widths, observation widths 1, 3, 4, 5, 16, 17, 33, 63, 64 (first-layer fragment counts
1, 2, 4, 5, 9, 16 with every remainder), action widths 1, 2, 13, 15, 16, both heads, with and without the feature norm,
and the three conditioned cases (fast_tanh's polynomial branch, saturation behind a division by sqrt(eps), a tied pair of
logits). No mailbox kernel is launched: they stay resident and wait on host flags, and `test_adversarial_gpu.py` holds them
against the per-step launches tested here.

A. `ia_policy_transpose` is bit-equal to a numpy restatement of `transpose_params_kernel`.
B. `ia_policy_act`, Gaussian: actions, values, logp within `TOL`; `clipped` bit-equal to clamping the device's own actions
   ([-1, 1], per-dimension asymmetric bounds, (-inf, +inf)); zero noise (a tensor of zeros and a NULL pointer: the same
   bits) returns the head means -- the bits `ia_policy_logits` writes --, scored by itself and by `ia_policy_evaluate` at
   sum(-log_std - log sqrt(2 pi)).
C. `ia_policy_act`, Discrete: inverse-CDF picks exact on every row under the guards, u = 0 and u = 1 - 2**-24 included;
   u < 0 gives the float64 arg-max, the lower index of the tied pair; logp of the pick and values within `TOL`;
   `actions == clipped` bitwise.
D. `ia_policy_evaluate`: the full call against float64; logp only: the full call's bits; values only: the full call's and
   `ia_policy_act`'s bits; `actions == NULL` with `logp != NULL` (the thread-per-row `policy_eval_kernel`, which no caller in
   the tree reaches): values and entropy against float64.
E. `ia_policy_logits`: logits against the float64 head output, values bit-equal to `ia_policy_act`'s, with and without the
   values pointer.
F. every output row of act, evaluate (both kernels) and logits on the first n of 130 rows, n in {1, 15, 16, 17, 63, 64, 65,
   130}, is bit-equal to the same row of the 130-row run.
G. every output is allocated with 64 rows more than the launch covers, filled with a NaN bit pattern, and the bits behind
   row n are compared after EVERY launch of this module (`_launch`); n in {1, 17, 65} for all entry points and forms.
H. obs_dim 0 and 65, act_dim 0 and 17, hidden 48, n = 0 and `ia_policy_logits` without a logits pointer return IA_ERR_ARG
   (-1: `pol_ok` or the row count fails before anything is launched; a width other than 32 and 64 never reaches
   `by_hidden`'s IA_ERR_UNSUPPORTED) and leave canary-filled outputs untouched.

Tolerances: `policy_forward_ref.TOL` (8 x the float32 oracle's own deviation from the reference, at most 1e-4). Worst
deviation measured on an MI355X over all cases, beside the tolerance:

                 B: act, Gaussian     C: act, Discrete     D: evaluate          D: thread per row    E: logits
    head         3.38e-07 / 3.4e-06   (picks: exact)       --                   --                   4.08e-07 / 3.4e-06
    actions      3.68e-07 / 3.6e-06   (picks: exact)       --                   --                   --
    values       4.09e-07 / 4.0e-06   5.69e-07 / 4.0e-06   5.69e-07 / 4.0e-06   4.95e-07 / 4.0e-06   5.69e-07 / 4.0e-06
    logp         2.10e-07 / 2.6e-06   2.82e-07 / 2.6e-06   2.23e-07 / 2.6e-06   --                   --
    entropy      --                   --                   2.71e-07 / 2.0e-06   3.18e-07 / 2.0e-06   --
    Every figure is at most a seventh of its tolerance and a fiftieth of the 1e-4 ceiling: the kernels are as close to
    float64 as torch's CPU float32 is (floor: 4.3e-7, 4.5e-7, 5.0e-7, 3.2e-7, 2.5e-7). Per case the small-pre-activation case
    measures head 4.9e-8, the saturated case 2.1e-7. All picks and modes equal float64's on every row; every bit-equality of
    B-G holds on every case (logp-only and values-only calls against the full call, values of evaluate and logits against
    act's, rows alone against rows in the 130-row batch, the canaries behind row n).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from tests import policy_forward_ref as R
from tests.test_kernels_gpu import DEV, DevPolicy

pytestmark = pytest.mark.gpu

ALL_CASES = list(R.CASES)
GAUSSIAN = [n for n in ALL_CASES if not R.CASES[n].discrete]
DISCRETE = [n for n in ALL_CASES if R.CASES[n].discrete]
# F and G: both tower widths x both heads at the widest geometry and at odd ones, and the saturated case
ROW_CASES = ["64x16b_h32_norm", "64x16d_h64_norm", "5x15d_h32_plain", "17x1b_h64_plain", "33x15b_h32_plain", R.SATURATED_CASE]
ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65, 130)
PAD = 64
CANARY = 0x7FC0DEAD          # a quiet NaN
IA_ERR_ARG = -1

_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not th.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    yield
    sections = sorted({s for s, _ in _WORST})
    print("\n    worst deviation / tolerance   " + "   ".join(f"{s:<22s}" for s in sections))
    for q in R.QUANTITIES:
        print(f"    {q:<28s}  " + "   ".join(f"{_WORST[s, q]:.2e} / {R.TOL[q]:.1e}    " if (s, q) in _WORST else " " * 22 for s in sections))


_CASES = {}


def _case(name):
    """(case, policy, inputs, float64 reference, device policy, device inputs): computed once, shared, never changed."""
    if name not in _CASES:
        case = R.CASES[name]
        pol, inp = R.build(case)
        ref = R.reference(case, pol, inp)
        R.assert_guards(case, ref)
        dp = DevPolicy(pol, case.D, case.A, case.H, case.discrete, case.norm)
        _CASES[name] = (case, pol, inp, ref, dp, {k: v.to(DEV).contiguous() for k, v in inp.items()})
    return _CASES[name]


def _assert_within(section, what, got, ref):
    dev = R.deviations(got, ref)
    print(f"\n    {what}: " + "  ".join(f"{q} {v:.2e}/{R.TOL[q]:.1e}" for q, v in dev.items()))
    for q, v in dev.items():
        _WORST[section, q] = max(_WORST.get((section, q), 0.0), v)
    for q, v in dev.items():
        assert v <= R.TOL[q], f"{what}: {q} deviates by {v:.3g} from float64, tolerance {R.TOL[q]:.3g}"


# ---- launches: every output has PAD canary rows behind row n, checked after the launch (G) -------------------------------------------
def _canary(rows, width=None):
    shape = (rows + PAD,) if width is None else (rows + PAD, width)
    return th.full(shape, CANARY, dtype=th.int32, device=DEV).view(th.float32)


def _bits(t):
    return t.contiguous().view(th.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and th.equal(_bits(a), _bits(b))


def _untouched(t):
    return bool((_bits(t) == CANARY).all())


def _launch(name, n, outs, *args):
    """Calls entry point `name`, then returns the first n rows of every output (None stays None) after checking that
    nothing behind them was written."""
    L.call(name, *args)
    th.cuda.synchronize()
    for k, t in outs.items():
        assert t is None or _untouched(t[n:]), f"{name}: `{k}` was written behind row {n}"
    return {k: None if t is None else t[:n] for k, t in outs.items()}


def _head(dp):
    return C.byref(dp.d), L.ptr(dp.P), L.ptr(dp.Pt), L.ptr(dp.nm), L.ptr(dp.nv)


def _rows(t, n):
    return None if t is None else t[:n].clone()      # a buffer of exactly n rows


def act(case, dp, dv, n, noise="given"):
    """`ia_policy_act` on the first n rows. noise: "given" (the case's noise / uniforms), "zero", None (a NULL pointer) or
    "mode" (Discrete: u = -1)."""
    aw = 1 if case.discrete else case.A
    src = dv["u"] if case.discrete else dv["noise"]
    nz = {"given": _rows(src, n), "zero": th.zeros_like(src[:n]), None: None, "mode": th.full_like(src[:n], -1.0)}[noise]
    low, high = (dv["low"], dv["high"]) if not case.discrete else (th.zeros(1, device=DEV), th.zeros(1, device=DEV))
    obs = _rows(dv["obs"], n)
    o = dict(actions=_canary(n, aw), clipped=_canary(n, aw), values=_canary(n), logp=_canary(n))
    return _launch("ia_policy_act", n, o, *_head(dp), L.ptr(obs), n, L.ptr(nz), L.ptr(low), L.ptr(high),
                   L.ptr(o["actions"]), L.ptr(o["clipped"]), L.ptr(o["values"]), L.ptr(o["logp"]), L.stream())


def evaluate(case, dp, dv, n, actions="given", logp=True, values=True, entropy=True):
    """`ia_policy_evaluate` on the first n rows; actions: "given" (the case's), a tensor, or None (a NULL pointer)."""
    aw = 1 if case.discrete else case.A
    a = _rows(dv["given"], n) if isinstance(actions, str) else actions
    a = None if a is None else a.reshape(n, aw).contiguous()
    obs = _rows(dv["obs"], n)
    o = dict(logp=_canary(n) if logp else None, values=_canary(n) if values else None, entropy=_canary(n) if entropy else None)
    return _launch("ia_policy_evaluate", n, o, *_head(dp), L.ptr(obs), L.ptr(a), n, L.ptr(o["logp"]),
                   L.ptr(o["values"]), L.ptr(o["entropy"]), L.stream())


def logits(case, dp, dv, n, values=True):
    obs = _rows(dv["obs"], n)
    o = dict(logits=_canary(n, case.A), values=_canary(n) if values else None)
    return _launch("ia_policy_logits", n, o, *_head(dp), L.ptr(obs), n, L.ptr(o["logits"]), L.ptr(o["values"]),
                   L.stream())


# ---- A -----------------------------------------------------------------------------------------------------------------------------
def _transposed(flat, D, A, H, discrete):
    """`transpose_params_kernel`, restated: pW1, pW2, vW1, vW2 go from [out][in] to [in][out]; the rest is copied."""
    out, off = flat.copy(), (0 if discrete else A)
    for _ in range(2):
        for cols in (D, H):
            out[off:off + H * cols] = flat[off:off + H * cols].reshape(H, cols).T.reshape(-1)
            off += H * cols + H
    assert off + H * A + A + H + 1 == flat.size
    return out


@pytest.mark.parametrize("name", ALL_CASES)
def test_transpose_is_exact(name):
    case, pol, inp, ref, dp, dv = _case(name)
    flat = dp.P.cpu().numpy()
    out = th.full((flat.size + PAD,), CANARY, dtype=th.int32, device=DEV).view(th.float32)
    L.call("ia_policy_transpose", C.byref(dp.d), L.ptr(dp.P), L.ptr(out), L.stream())
    th.cuda.synchronize()
    want = _transposed(flat, case.D, case.A, case.H, case.discrete)
    assert np.array_equal(out[:flat.size].cpu().numpy().view(np.int32), want.view(np.int32))
    assert _untouched(out[flat.size:]) and _same_bits(out[:flat.size], dp.Pt)


# ---- B -----------------------------------------------------------------------------------------------------------------------------
def _clamped(a, low, high):
    return th.minimum(th.maximum(a, low), high)      # fminf(fmaxf(a, low), high)


@pytest.mark.parametrize("name", GAUSSIAN)
def test_act_gaussian(name):
    case, pol, inp, ref, dp, dv = _case(name)
    n = case.n
    o = act(case, dp, dv, n)
    _assert_within("B act, Gaussian", name, dict(sample=o["actions"], values=o["values"], logp_sample=o["logp"]), ref)
    assert _same_bits(o["clipped"], _clamped(o["actions"], dv["low"], dv["high"])), "clipping is exact"
    if case.bounds == "inf":
        assert _same_bits(o["clipped"], o["actions"])
    else:
        a = o["actions"]
        assert (a < dv["low"]).any() and (a > dv["high"]).any() and ((a > dv["low"]) & (a < dv["high"])).any(), \
            "the case clips on neither side, or everywhere"
    # zero noise: the head means
    z, znull, lg = act(case, dp, dv, n, "zero"), act(case, dp, dv, n, None), logits(case, dp, dv, n)
    assert all(_same_bits(z[k], znull[k]) for k in z), "a NULL noise pointer is zero noise"
    assert _same_bits(z["actions"], lg["logits"]), "zero noise returns the head means, bit for bit"
    assert _same_bits(z["values"], o["values"]) and _same_bits(z["clipped"], _clamped(z["actions"], dv["low"], dv["high"]))
    at_mean = np.full(n, float(-(pol.log_std.detach().double() + math.log(math.sqrt(2.0 * math.pi))).sum()))
    ev = evaluate(case, dp, dv, n, actions=z["actions"], values=False, entropy=False)
    for what, lp in (("act", z["logp"]), ("evaluate", ev["logp"])):
        d = R.deviation(lp, at_mean)
        print(f"    {name}: logp of the mean, {what}: {d:.2e}/{R.TOL['logp']:.1e}")
        _WORST["B act, Gaussian", "logp"] = max(_WORST["B act, Gaussian", "logp"], d)
        assert d <= R.TOL["logp"], f"{what} scores the mean {d:.3g} away from sum(-log_std - log sqrt(2 pi))"
    _assert_within("B act, Gaussian", name + " means", dict(head=z["actions"]), ref)


# ---- C -----------------------------------------------------------------------------------------------------------------------------
def _picks(o):
    a = o["actions"].cpu().flatten()
    assert th.equal(a, a.round()), "action indices are whole numbers"
    return a.long().numpy()


@pytest.mark.parametrize("name", DISCRETE)
def test_act_discrete(name):
    case, pol, inp, ref, dp, dv = _case(name)
    n = case.n
    assert float(inp["u"][0]) == 0.0 and float(inp["u"][1]) == R.U_LAST
    o = act(case, dp, dv, n)
    picks = _picks(o)
    wrong = np.flatnonzero(picks != ref.pick)
    assert wrong.size == 0, (f"rows {wrong[:8]}: picked {picks[wrong[:8]]}, float64 inverse CDF {ref.pick[wrong[:8]]} "
                             f"(u {inp['u'].numpy()[wrong[:8]]})")
    assert picks[0] == 0 and picks[1] == case.A - 1
    assert _same_bits(o["actions"], o["clipped"])
    _assert_within("C act, Discrete", name, dict(values=o["values"], logp_pick=o["logp"]), ref)
    m = act(case, dp, dv, n, "mode")
    modes = _picks(m)
    wrong = np.flatnonzero(modes != ref.mode)
    assert wrong.size == 0, f"rows {wrong[:8]}: mode {modes[wrong[:8]]}, float64 arg-max {ref.mode[wrong[:8]]}"
    if case.kind == "tie":
        lg = logits(case, dp, dv, n)["logits"]
        assert _same_bits(lg[:, R.TIE_ROWS[0]], lg[:, R.TIE_ROWS[1]]), "the tied logits are bit-equal on the device"
        assert (modes == min(R.TIE_ROWS)).all()
    assert _same_bits(m["actions"], m["clipped"]) and _same_bits(m["values"], o["values"])
    _assert_within("C act, Discrete", name + " mode", dict(logp_mode=m["logp"]), ref)


# ---- D -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_evaluate_in_all_its_forms(name):
    case, pol, inp, ref, dp, dv = _case(name)
    n = case.n
    full = evaluate(case, dp, dv, n)
    _assert_within("D evaluate", name, dict(logp_given=full["logp"], values=full["values"], entropy=full["entropy"]), ref)
    only_lp = evaluate(case, dp, dv, n, values=False, entropy=False)        # AIRL's log pi(a|s)
    assert _same_bits(only_lp["logp"], full["logp"]), "logp only: the full call's bits"
    only_v = evaluate(case, dp, dv, n, actions=None, logp=False, entropy=False)   # `values_rows`, the GAE bootstrap
    assert _same_bits(only_v["values"], full["values"]), "values only: the full call's bits"
    assert _same_bits(only_v["values"], act(case, dp, dv, n)["values"]), "values only: the rollout step's bits"
    # actions == NULL with logp != NULL: the thread-per-row kernel
    row = evaluate(case, dp, dv, n, actions=None)
    _assert_within("D thread per row", name, dict(values=row["values"], entropy=row["entropy"]), ref)
    if case.discrete:
        assert _untouched(row["logp"]), "no actions: a Categorical log-prob is not written"


# ---- E -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_logits(name):
    case, pol, inp, ref, dp, dv = _case(name)
    n = case.n
    lg = logits(case, dp, dv, n)
    _assert_within("E logits", name, dict(head=lg["logits"], values=lg["values"]), ref)
    assert _same_bits(lg["values"], act(case, dp, dv, n)["values"]), "the values of the rollout step, bit for bit"
    assert _same_bits(logits(case, dp, dv, n, values=False)["logits"], lg["logits"])


# ---- F, G ---------------------------------------------------------------------------------------------------------------------------
def _every_form(case, dp, dv, n):
    """All outputs of every entry point and form on the first n rows, flat: {"form.output": tensor}."""
    runs = {"act": act(case, dp, dv, n), "evaluate": evaluate(case, dp, dv, n),
            "evaluate_logp": evaluate(case, dp, dv, n, values=False, entropy=False),
            "evaluate_values": evaluate(case, dp, dv, n, actions=None, logp=False, entropy=False),
            "evaluate_rows": evaluate(case, dp, dv, n, actions=None), "logits": logits(case, dp, dv, n),
            "logits_only": logits(case, dp, dv, n, values=False)}
    runs["act_mode" if case.discrete else "act_zero"] = act(case, dp, dv, n, "mode" if case.discrete else "zero")
    return {f"{f}.{k}": t for f, o in runs.items() for k, t in o.items() if t is not None}


@pytest.mark.parametrize("name", ROW_CASES)
def test_rows_do_not_depend_on_the_batch(name):
    case, pol, inp, ref, dp, dv = _case(name)
    assert case.n == 130
    whole = _every_form(case, dp, dv, 130)
    for n in ROW_COUNTS:
        part = _every_form(case, dp, dv, n)
        assert set(part) == set(whole)
        for k, t in part.items():
            assert _same_bits(t, whole[k][:n]), f"{k}: {n} rows alone differ from the first {n} of 130"


@pytest.mark.parametrize("n", [1, 17, 65])
@pytest.mark.parametrize("name", ROW_CASES)
def test_nothing_past_row_n_is_written(name, n):
    case, pol, inp, ref, dp, dv = _case(name)
    outs = _every_form(case, dp, dv, n)        # (`_launch` compares the PAD rows behind row n of every output)
    assert all(t.shape[0] == n for t in outs.values())
    written = {k for k, t in outs.items() if not _untouched(t)}
    unwritten = set(outs) - written
    # the only output a launch leaves alone: the log-prob of the thread-per-row form without actions, Categorical head
    assert unwritten == ({"evaluate_rows.logp"} if case.discrete else set()), unwritten


# ---- H -----------------------------------------------------------------------------------------------------------------------------
BAD_DESCRIPTORS = {"obs_dim 0": dict(D=0), "obs_dim 65": dict(D=65), "act_dim 0": dict(A=0), "act_dim 17": dict(A=17),
                   "hidden 48": dict(H=48)}


def _refused(desc, n, dp, with_logits=True):
    """Return codes of the row entry points for (desc, n) (without a logits pointer: of `ia_policy_logits` alone), each on
    canary-filled outputs that must stay untouched."""
    lib = L.load()
    big = lambda: th.full((130 * 65,), CANARY, dtype=th.int32, device=DEV).view(th.float32)
    ins = [th.zeros(130 * 65, device=DEV) for _ in range(4)]      # obs, noise / actions, low, high
    head = (C.byref(desc), L.ptr(dp.P), L.ptr(dp.Pt), L.ptr(ins[0]), L.ptr(ins[0]))
    outs = [big() for _ in range(4)]
    codes = {}
    if not with_logits:
        codes["logits"] = lib.ia_policy_logits(*head, L.ptr(ins[0]), n, None, L.ptr(outs[1]), L.stream())
        th.cuda.synchronize()
        assert all(_untouched(t) for t in outs), "a refused call wrote to its outputs"
        return codes
    codes["act"] = lib.ia_policy_act(*head, L.ptr(ins[0]), n, L.ptr(ins[1]), L.ptr(ins[2]), L.ptr(ins[3]), *(L.ptr(t) for t in outs),
                                     L.stream())
    codes["evaluate"] = lib.ia_policy_evaluate(*head, L.ptr(ins[0]), L.ptr(ins[1]), n, *(L.ptr(t) for t in outs[:3]), L.stream())
    codes["evaluate_rows"] = lib.ia_policy_evaluate(*head, L.ptr(ins[0]), None, n, *(L.ptr(t) for t in outs[:3]), L.stream())
    codes["logits"] = lib.ia_policy_logits(*head, L.ptr(ins[0]), n, L.ptr(outs[0]), L.ptr(outs[1]), L.stream())
    th.cuda.synchronize()
    assert all(_untouched(t) for t in outs), "a refused call wrote to its outputs"
    return codes


@pytest.mark.parametrize("what", list(BAD_DESCRIPTORS))
def test_bad_descriptors_are_refused(what):
    case, pol, inp, ref, dp, dv = _case("64x16b_h32_norm")
    g = dict(D=case.D, A=case.A, H=case.H)
    g.update(BAD_DESCRIPTORS[what])
    desc = L.PolicyDesc(g["D"], g["A"], g["H"], 0, 1, 1e-5)
    lib = L.load()
    assert lib.ia_policy_param_count(C.byref(desc)) == IA_ERR_ARG
    out = th.full((20000,), CANARY, dtype=th.int32, device=DEV).view(th.float32)
    assert lib.ia_policy_transpose(C.byref(desc), L.ptr(dp.P), L.ptr(out), L.stream()) == IA_ERR_ARG
    th.cuda.synchronize()
    assert _untouched(out)
    assert _refused(desc, 130, dp) == dict(act=IA_ERR_ARG, evaluate=IA_ERR_ARG, evaluate_rows=IA_ERR_ARG, logits=IA_ERR_ARG)


def test_no_rows_and_a_missing_logits_pointer_are_refused():
    for name in ("64x16b_h32_norm", "64x16d_h64_norm"):
        case, pol, inp, ref, dp, dv = _case(name)
        assert _refused(dp.d, 0, dp) == dict(act=IA_ERR_ARG, evaluate=IA_ERR_ARG, evaluate_rows=IA_ERR_ARG, logits=IA_ERR_ARG)
        assert _refused(dp.d, 130, dp, with_logits=False) == dict(logits=IA_ERR_ARG)
