"""The PPO update kernels of csrc/policy.hip against the float64 reference of `tests/ppo_ref.py` (`-m gpu`): what they
compute BEFORE the parameters move -- the raw gradient, its norm and clip coefficient, Adam's two moments -- beside the
parameters, the transposed copy, all eight statistics columns and the feature norm's state. (The bit-identity tests
between forms cannot see an error the forms share; parameters after a few Adam steps barely see a mis-scaled block of
the gradient -- `tests/test_ppo_ref.py`, sensitivity.)

A. `ia_ppo_minibatch_grad` leaves the UNCLIPPED mean-loss gradient of its rows at `ws + ia_ppo_grad_offset()`: compared
   element-wise (per parameter block) with the reference's raw gradient; `ia_ppo_minibatch_apply` on it, with the scalars of
   steps 1 and 2, against float64 clip + Adam FED THE DEVICE'S OWN GRADIENT (`airl_ref.ADAM_ATOL` / `ADAM_RTOL`: only fp32
   rounding of the step differs; exp_avg_sq at rtol 2e-5 -- the kernels form `1.f - beta2` in fp32, 1.3e-5 low relative to
   1 - 0.999 in double).
B. every update form, one step per launch (T n == batch_size, one epoch), judged alone against `step_from(initial state)`,
   once with `max_grad_norm` = 1e9 (clip_coef == 1 and exp_avg == (1 - beta1) g: the element-wise view of the gradient
   of forms that never expose it) and once with 0.5 (clipped: grad_norm and clip_coef asserted).
C. chains of three steps with a short last minibatch against `chain(initial state, 3)`: the last step's exp_avg shows
   whether the short minibatch's gradient was averaged over its own rows.

Which kernel a case reaches, checked against `plan_epoch` and `ppo_update_launch`. The library has no query for the form
it chose and falls back quietly, so for `ia_ppo_epoch` / `ia_ppo_epochs` every run OBSERVES the class of kernel that ran,
through the measurement buffer of `ia_ppo_epoch_debug_timing` (it changes no result and no selection): the two-launch
form never writes it, the word-exchange kernels add ticks to slots 0-4, the grid-barrier kernels to slots 0-5.
  * 32-wide towers: always two launches per minibatch (`ppo_grad_mfma_kernel<32>` + `ppo_apply_split_kernel`).
  * 64-wide, modes 0, 4, 6, 7: word exchange wherever 2 x row blocks <= 64 and the tower images fit LDS
    ((20 544 + 2 (64 D + 4 224) + 4 D + 128 + lenB + 16) floats <= 161 792 bytes: 154 508 at (64, 16), the widest). Mode 0:
    `ppo_epoch_ll2_kernel` on 32-row blocks, eight waves, for D <= 32 (`<1, ...>` up to 16 columns, `<2, ...>` beyond),
    `ppo_epoch_ll_kernel` for (33, 1) and (64, 16); 4: `ppo_epoch_ll_kernel`; 6: 64-row blocks; 7: four waves. 64 rows: one
    row block, the parameters halved over two workgroups; 200: a short last block.
  * 64-wide, modes 2 and 3 (`ppo_epoch_persistent_kernel<64>` / `<64, true>`): need ceil(P / nrb) <= 2 048 and
    ceil(P / 2 nrb) <= 1 024 (`ppo_ref.barrier_forms_fit`). P is 9 155, 11 085 and 12 497 for (4, 2), (17, 6) and (27, 8), so
    the 64-, 128- and 200-row shapes of the other modes select NEITHER: there both modes run `ppo_grad_mfma_kernel<64>` +
    `ppo_apply_split_kernel` (two launches -- kept as that form's 64-wide cases). The barrier kernels are reached at 384
    rows (4, 2: 1 526 / 763 per workgroup), 330 rows (17, 6: six blocks, the last of 10 rows: 1 848 / 924) and 420 rows
    (27, 8: seven blocks: 1 786 / 893) -- STEP64_BARRIER_CASES; their images (133 k bytes at D = 27) fit the 162 816 allowed.
  * `ia_ppo_update` (32-wide; not observable, the arithmetic of `ppo_update_launch`): <= 16 rows `small`, <= 64 `local`
    (P4 <= the staging area), 140 three row blocks (the last of 12 rows), 576 nine blocks and two 512-row statistics
    slices; (17, 6) P = 3 501 <= 4 096: 8 parameters per thread, (27, 8) 4 209 and (33, 1) 4 355: 9; (33, 1) the 16-column
    first-layer fragments; (64, 16) has 6 849 parameters > 9 x 512 (`ia_ppo_update_ws_floats` == 0: skipped there, covered
    through `ia_ppo_epoch`); packing needs nblk > 1 and nblk + 1 + slices <= 32 (at most 12 here); the tower-split grid is
    2 nblk + 1 + 2 slices <= 23 workgroups, one per compute unit of 256, so `fits_resident` holds and the split kernels
    run (both slice ownerships: every pass of at most 9 x 512 lanes fits); `ia_ppo_update_sharded`: loopback world of one.

Tolerances: `ppo_ref.TOL_STEP` / `TOL_CHAIN` (8 x the float32 oracle's own deviation from the reference, at most the
project's ceilings). Worst deviation measured on an MI355X over all forms and cases, beside the tolerance:

                   A: `_grad` / `_apply`      B: one step, every form    C: chains of three steps
    grad           3.14e-06 / 2.0e-05         (not exposed)              (not exposed)
    exp_avg        (float64 Adam on the       2.64e-06 / 2.0e-05         9.36e-07 / 5.7e-06
    exp_avg_sq      device's own gradient:    1.58e-05 / 2.0e-05         1.43e-05 / 2.0e-05
    params          assert_close, above)      1.56e-06 / 1.7e-05         5.32e-08 / 4.8e-07
    norm           9.17e-08 / 7.0e-07         9.17e-08 / 7.0e-07         1.36e-07 / 1.0e-06
    pg_loss        7.22e-05 / 2.0e-03         8.37e-05 / 2.0e-03         7.10e-05 / 2.0e-03
    value_loss     5.03e-07 / 4.8e-06         2.11e-07 / 4.8e-06         2.53e-07 / 4.8e-06
    entropy_loss   6.64e-07 / 1.6e-06         6.05e-07 / 1.6e-06         3.19e-07 / 1.6e-06
    approx_kl      4.82e-04 / 4.3e-03         5.83e-06 / 4.3e-03         1.08e-06 / 4.3e-03
    loss           3.42e-04 / 7.8e-04         2.57e-06 / 7.8e-04         3.13e-07 / 7.8e-04
    grad_norm      5.53e-07 / 8.8e-06         4.75e-07 / 8.8e-06         3.21e-07 / 1.8e-06
    clip_coef      (as grad_norm)             4.78e-07 / 8.8e-06         3.17e-07 / 1.3e-06
    clip_fraction, norm count: equal on every case. No form is outside its tolerance.
    The grid-barrier kernels alone (modes 2 and 3 at 384, 330 and 420 rows): exp_avg 1.38e-06, exp_avg_sq 1.51e-05, params
    1.05e-07, entropy_loss 5.22e-07, grad_norm 2.07e-07, clip_coef 1.81e-07.

exp_avg_sq: every element is 1.29e-5 low on every form -- the kernels form `1.f - beta2` in fp32 (`ppo_ref.EXPLAINED`); the
rest of its figure is twice the gradient's own deviation. That is why it sits near its ceiling where exp_avg, from the same
gradient, is at 1e-6. The worst approx_kl and loss of A are a two-row and a 63-row minibatch on which the statistic is a
nearly cancelled sum (the float32 oracle's own worst figures for these two columns are 5.3e-4 and 8.3e-5).
"""
import ctypes as C
import math

import pytest
import torch as th

from imitation_amd import _lib as L
from tests import airl_ref
from tests import ppo_ref as R
from tests.test_kernels_gpu import DEV, DevPolicy
from tests.test_ppo_tower_split_gpu import _upload

pytestmark = pytest.mark.gpu

EXP_AVG_SQ_RTOL = 2e-5   # A: `1.f - beta2` formed in fp32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not th.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


_REFERENCES = {}


def _reference(name, max_grad_norm):
    """(policy, host rollout, Reference, its steps from the initial state) of a case: computed once, shared, never changed."""
    key = (name, max_grad_norm)
    if key not in _REFERENCES:
        case = R.CASES[name]
        pol, host = R.build(case)
        ref = R.Reference(case, pol, host, max_grad_norm)
        steps = ref.chain(ref.initial, case.steps)
        R.assert_guards(steps, max_grad_norm == R.CLIPPED, max_grad_norm, name)
        _REFERENCES[key] = (pol, host, ref, steps)
    return _REFERENCES[key]


def _device_policy(case, pol):
    return DevPolicy(pol, case.D, case.A, case.H, case.discrete, case.norm)


def _transposed(dp):
    out = th.empty_like(dp.P)
    L.call("ia_policy_transpose", C.byref(dp.d), L.ptr(dp.P), L.ptr(out), L.stream())
    th.cuda.synchronize()
    return out


def _report(what, dev, tol):
    print(f"\n    {what}: " + "  ".join(f"{q} {v:.2e}/{tol[q]:.1e}" for q, v in dev.items()))


def _assert_within(what, dev, tol):
    _report(what, dev, tol)
    for q, v in dev.items():
        assert v <= tol[q], f"{what}: {q} deviates by {v:.3g} from float64, tolerance {tol[q]:.3g}"


def _assert_exact_counts(case, dp, stats, steps):
    st = stats.detach().cpu().double().reshape(len(steps), 8)
    for k, s in enumerate(steps):
        assert R.clipped_rows(float(st[k, 4]), s.rows) == R.clipped_rows(s.stats[4], s.rows), f"clip_fraction, step {k}"
    if case.norm:
        assert int(dp.nc.item()) == steps[-1].state.nc


# ---- A -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.GRAD_CASES)
def test_minibatch_grad_leaves_the_raw_gradient_and_apply_clips_and_steps_it(name):
    case = R.CASES[name]
    pol, host, ref, (step,) = _reference(name, R.CLIPPED)
    rows = _upload(host)
    dp = _device_policy(case, pol)
    lib = L.load()
    nP, b = dp.P.numel(), case.bs
    ws = th.zeros(int(lib.ia_ppo_ws_floats(C.byref(dp.d), b, b)), device=DEV)
    idx = rows["perm"][0].contiguous()
    P0, Pt0 = dp.P.clone(), dp.Pt.clone()
    L.call("ia_ppo_minibatch_grad", C.byref(dp.d), L.ptr(dp.P), L.ptr(dp.Pt), L.ptr(dp.nm), L.ptr(dp.nv), L.ptr(dp.nc),
           int(case.norm), L.ptr(rows["obs"]), L.ptr(rows["act"]), L.ptr(rows["lp"]), L.ptr(rows["adv"]), L.ptr(rows["ret"]),
           L.ptr(idx), b, case.T, case.n, int(case.normalize_adv), R.CLIP_RANGE, R.ENT_COEF, R.VF_COEF, L.ptr(ws), L.stream())
    th.cuda.synchronize()
    off = int(lib.ia_ppo_grad_offset(C.byref(dp.d), b))
    assert 0 < off and off + nP <= ws.numel()
    g = ws[off:off + nP].clone()
    assert th.equal(dp.P, P0) and th.equal(dp.Pt, Pt0) and not dp.m.any() and not dp.v.any(), "`_grad` steps nothing"
    got = dict(grad=g)
    if case.norm:
        got.update(nm=dp.nm, nv=dp.nv)
    dev = R.deviations(got, step, ref.sizes)
    # `_apply` with the scalars of steps 1 and 2 on that gradient, against float64 clip + Adam fed the SAME gradient
    stats = th.zeros(2, 8, device=DEV)
    state = ref.initial
    for t in (1, 2):
        bc1, bc2 = 1.0 - R.BETA1 ** t, 1.0 - R.BETA2 ** t
        L.call("ia_ppo_minibatch_apply", C.byref(dp.d), L.ptr(dp.P), L.ptr(dp.Pt), b, R.ENT_COEF, R.VF_COEF, R.CLIPPED,
               L.ptr(dp.m), L.ptr(dp.v), R.BETA1, R.BETA2, R.ADAM_EPS, R.LR / bc1, math.sqrt(bc2), L.ptr(ws), L.ptr(stats[t - 1]),
               L.stream())
        th.cuda.synchronize()
        assert th.equal(ws[off:off + nP], g), "`_apply` leaves the gradient as it found it"
        total_norm, coef, m64, v64, P64 = R.clip_and_adam(g, state, R.CLIPPED)
        state = R.State(P64, m64, v64, None, None, 0, t)
        st = stats[t - 1].cpu().double()
        assert abs(float(st[6]) - total_norm) <= R.TOL_STEP["grad_norm"] * total_norm, (t, float(st[6]), total_norm)
        assert abs(float(st[7]) - coef) <= R.TOL_STEP["clip_coef"] * coef and coef < 1.0, (t, float(st[7]), coef)
        kw = dict(rtol=airl_ref.ADAM_RTOL, atol=airl_ref.ADAM_ATOL)
        th.testing.assert_close(dp.m.cpu().double(), m64, msg=lambda s, t=t: f"exp_avg, step {t}: {s}", **kw)
        th.testing.assert_close(dp.v.cpu().double(), v64, rtol=EXP_AVG_SQ_RTOL, atol=airl_ref.ADAM_ATOL,
                                msg=lambda s, t=t: f"exp_avg_sq, step {t}: {s}")
        th.testing.assert_close(dp.P.cpu().double(), P64, msg=lambda s, t=t: f"parameters, step {t}: {s}", **kw)
        # (atol dominates rtol on most elements of exp_avg_sq ~ 1e-3 g^2: relative to each block's own largest element too)
        for q, x, w in (("exp_avg", dp.m, m64), ("exp_avg_sq", dp.v, v64)):
            worst = max(R.block_deviation(x, w, ref.sizes))
            assert worst <= EXP_AVG_SQ_RTOL, f"{q}, step {t}: {worst:.3g} of a block's scale"
        assert th.equal(dp.Pt, _transposed(dp)), f"transposed copy, step {t}"
    # the loss statistics of the record (the same on both calls: the gradient kernel's partial sums)
    assert th.equal(stats[0, :6], stats[1, :6])
    dev.update({q: v for q, v in R.deviations(dict(stats=stats[0]), step, ref.sizes).items() if q not in ("grad_norm", "clip_coef")})
    # (grad_norm of the record against the reference's own norm as well: the gradient's error carries over)
    dev["grad_norm"] = abs(float(stats[0, 6]) - step.total_norm) / step.total_norm
    _assert_exact_counts(case, dp, stats[0], [step])
    _assert_within(name, dev, R.TOL_STEP)


# ---- the forms of B and C --------------------------------------------------------------------------------------------------------------
def _epoch_kernel_class(case, mode):
    """The class of kernel `plan_epoch` selects for a one-minibatch epoch of `case` under `ia_ppo_epoch_split(mode)`, from
    its conditions (module docstring); `_launch` compares it with the class that ran."""
    if case.H != 64:
        return "two_launches"
    whole, split = R.barrier_forms_fit(case)
    if mode in (2, 3):
        return "barrier" if (whole if mode == 2 else split) else "two_launches"
    assert 2 * -(-case.bs // 64) <= 64
    return "word_exchange"


def _launch(form, case, dp, rows, max_grad_norm, stats):
    """One epoch of `case` through `form` = (entry, switches); returns the workspace's error word (0 where the form has
    none). Resets every mode switch it sets."""
    entry, sw = form
    lib = L.load()
    d = C.byref(dp.d)
    perm = rows["perm"][:1].contiguous()
    head = (d, L.ptr(dp.P), L.ptr(dp.Pt), L.ptr(dp.nm), L.ptr(dp.nv), L.ptr(dp.nc), int(case.norm), L.ptr(rows["obs"]),
            L.ptr(rows["act"]), L.ptr(rows["lp"]), L.ptr(rows["adv"]), L.ptr(rows["ret"]), L.ptr(perm))
    hyper = (int(case.normalize_adv), R.CLIP_RANGE, R.ENT_COEF, R.VF_COEF, float(max_grad_norm), L.ptr(dp.m), L.ptr(dp.v), R.LR,
             R.BETA1, R.BETA2, R.ADAM_EPS, 0)
    try:
        if entry in ("epoch", "epochs"):
            lib.ia_ppo_epoch_split(sw.get("epoch_split", 0))
            ws = th.zeros(int(lib.ia_ppo_ws_floats(d, case.bs, case.rows)), device=DEV)
            ticks = th.zeros(64, dtype=th.int64, device=DEV)
            lib.ia_ppo_epoch_debug_timing(C.c_void_p(ticks.data_ptr()))
            if entry == "epoch":
                L.call("ia_ppo_epoch", *head, case.T, case.n, case.bs, *hyper, L.ptr(ws), L.ptr(stats), L.stream())
            else:
                L.call("ia_ppo_epochs", *head, 1, case.T, case.n, case.bs, *hyper, L.ptr(ws), L.ptr(stats), L.stream())
            th.cuda.synchronize()
            t = ticks[:6].cpu()
            ran = "barrier" if int(t[5]) > 0 else ("word_exchange" if int(t[0]) > 0 else "two_launches")
            assert ran == _epoch_kernel_class(case, sw.get("epoch_split", 0)), f"{ran} ran: another form than the case is for"
            return int(ws[5:6].view(th.int32).item()) if ran != "two_launches" else 0
        if entry == "update":
            nws = int(lib.ia_ppo_update_ws_floats(d, case.bs))
            if nws == 0:
                pytest.skip("shape not covered by the persistent kernel (parameter copies do not fit LDS)")
            ws = th.zeros(nws, device=DEV)
            lib.ia_ppo_update_xcd_pack(sw.get("xcd_pack", 0))
            lib.ia_ppo_update_tower_split(sw.get("tower_split", 0))
            assert lib.ia_ppo_update_slice_owner(sw.get("slice_owner", 0)) == 0
            L.call("ia_ppo_update", *head, 1, case.T, case.n, case.bs, *hyper, L.ptr(ws), L.ptr(stats), L.stream())
            th.cuda.synchronize()
            return int(ws[8:9].view(th.int32).item())
        assert entry == "sharded"
        from imitation_amd.distributed import PeerExchange
        nws = int(lib.ia_ppo_update_sharded_ws_floats(d, case.bs, 1))
        if nws == 0:
            pytest.skip("shape not covered by the persistent kernel (parameter copies do not fit LDS)")
        ws = th.zeros(nws, device=DEV)
        ex = PeerExchange.loopback(1, dp.d)
        assert ex.ok
        try:
            L.call("ia_ppo_update_sharded", *head, 1, case.T, case.n, case.bs, *hyper, L.ptr(ws), L.ptr(stats), 1, 0,
                   ex.take_steps(case.steps), ex.recv, ex.peer_recv, 1, 5.0, L.stream())
            th.cuda.synchronize()
            return int(ws[8:9].view(th.int32).item())
        finally:
            th.cuda.synchronize()
            ex.close()
    finally:
        lib.ia_ppo_epoch_debug_timing(None)
        lib.ia_ppo_epoch_split(0)
        lib.ia_ppo_update_xcd_pack(0)
        lib.ia_ppo_update_tower_split(0)
        lib.ia_ppo_update_slice_owner(0)


def _several_blocks(names):
    return [n for n in names if R.CASES[n].bs > 64]


EPOCH, EPOCHS, UPDATE = ("epoch", {}), ("epochs", {}), ("update", {})
PACKED = ("update", dict(xcd_pack=1))
SPLIT0, SPLIT1 = ("update", dict(tower_split=1, slice_owner=0)), ("update", dict(tower_split=1, slice_owner=1))
SHARDED = ("sharded", {})
FORMS = {"epoch": EPOCH, "epochs": EPOCHS, "update": UPDATE, "update_packed": PACKED, "update_split_owner0": SPLIT0,
         "update_split_owner1": SPLIT1, "update_shard1": SHARDED}
FORMS.update({f"epoch_mode{m}": ("epoch", dict(epoch_split=m)) for m in (2, 3, 4, 6, 7)})

STEP_RUNS = ([("epoch", n) for n in R.STEP32_CASES + R.STEP64_CASES]                   # (64-wide: mode 0)
             + [("epochs", n) for n in R.STEP32_CASES[2:4] + R.STEP64_MODE_CASES]
             + [(f"epoch_mode{m}", n) for m in (2, 3, 4, 6, 7) for n in R.STEP64_MODE_CASES]    # (2, 3: two launches here)
             + [(f"epoch_mode{m}", n) for m in (2, 3) for n in R.STEP64_BARRIER_CASES]          # (the barrier kernels)
             + [("update", n) for n in R.STEP32_CASES]
             + [(f, n) for f in ("update_packed", "update_split_owner0", "update_split_owner1")
                for n in _several_blocks(R.STEP32_CASES)]
             + [("update_shard1", n) for n in R.STEP32_CASES[:5] + R.STEP32_CASES[7:9]])
CHAIN_RUNS = ([("epoch", n) for n in R.CHAIN_CASES]
              + [(f, n) for f in ("update", "update_split_owner0", "update_split_owner1")
                 for n in R.CHAIN_CASES if R.CASES[n].H == 32])


def _outputs(case, dp, stats):
    got = dict(exp_avg=dp.m, exp_avg_sq=dp.v, params=dp.P, stats=stats)
    if case.norm:
        got.update(nm=dp.nm, nv=dp.nv)
    return got


# ---- B -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_grad_norm", [R.UNCLIPPED, R.CLIPPED], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("form,name", STEP_RUNS)
def test_one_step_of_every_form_matches_float64(form, name, max_grad_norm):
    case = R.CASES[name]
    pol, host, ref, (step,) = _reference(name, max_grad_norm)
    rows = _upload(host)
    dp = _device_policy(case, pol)
    stats = th.zeros(1, 1, 8, device=DEV)
    err = _launch(FORMS[form], case, dp, rows, max_grad_norm, stats)
    assert err == 0, f"the workspace's error word is {err}: a wait timed out"
    dev = R.deviations(_outputs(case, dp, stats[0, 0]), step, ref.sizes)
    if max_grad_norm == R.UNCLIPPED:
        assert float(stats[0, 0, 7]) == 1.0
    else:
        assert float(stats[0, 0, 7]) < 1.0
    _assert_exact_counts(case, dp, stats, [step])
    assert th.equal(dp.Pt, _transposed(dp)), "the transposed copy follows the parameters"
    _assert_within(f"{form} {name}", dev, R.TOL_STEP)


# ---- C -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,name", CHAIN_RUNS)
def test_three_steps_with_a_short_last_minibatch_match_float64(form, name):
    case = R.CASES[name]
    pol, host, ref, steps = _reference(name, R.CLIPPED)
    assert len(steps) == 3 and steps[-1].rows < case.bs
    rows = _upload(host)
    dp = _device_policy(case, pol)
    stats = th.zeros(1, 3, 8, device=DEV)
    err = _launch(FORMS[form], case, dp, rows, R.CLIPPED, stats)
    assert err == 0, f"the workspace's error word is {err}: a wait timed out"
    dev = R.deviations(_outputs(case, dp, stats[0, 2]), steps[-1], ref.sizes)
    for k in (0, 1):   # the earlier steps' records
        for q, v in R.deviations(dict(stats=stats[0, k]), steps[k], ref.sizes).items():
            dev[q] = max(dev[q], v)
    _assert_exact_counts(case, dp, stats, steps)
    assert th.equal(dp.Pt, _transposed(dp)), "the transposed copy follows the parameters"
    _assert_within(f"{form} {name}", dev, R.TOL_CHAIN)
