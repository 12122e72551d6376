"""The inputs and the noise floor of `tests/test_airl_fused_gpu.py`, proven on the CPU (no GPU, no HIP library).

For every case of `tests/airl_ref.py` and both of its updates, on the float64 reference alone:
  * no logit x = f - log pi has |x| < 1e-4, so the four count statistics can be asserted exactly on the device;
  * no hidden pre-activation has |z| < 1e-5, so no ReLU can legitimately switch between fp32 and fp64 (a switch moves
    a weight gradient by a whole row's contribution -- far more than summation order does).
Each case's seed in `airl_ref.CASES` was picked here so that both hold.

Noise floor: the SAME oracle module run in float32 and in float64 from the same state (the float32 twin plays the
device: warm-up of the norms, then per update its state is copied into the float64 module, as the GPU test copies the
HIP net's). Worst deviation over the two updates, in the measures of `airl_ref.deviations`; (min |x|, min |z|) are the
margins of the two conditions:

    case              logits     loss       entropy    grad       norm       min |x|    min |z|
    1_baseline        7.70e-08   4.22e-08   2.75e-07   7.36e-08   6.21e-08   2.07e-03   7.75e-05
    2_one_by_one      2.95e-08   7.68e-08   1.67e-07   7.92e-08   0.00e+00   6.24e+00   3.03e-04
    3_discrete_129    5.02e-08   2.46e-08   1.48e-07   1.20e-07   6.90e-08   7.97e-02   7.82e-05
    4_db64_385        8.72e-08   6.09e-08   1.67e-07   8.82e-08   1.07e-07   2.58e-03   3.13e-05
    5_dp64            1.14e-07   1.11e-07   2.81e-07   7.69e-08   0.00e+00   4.88e-02   3.69e-05
    6_dp33_gamma1     1.03e-07   1.17e-07   1.14e-07   9.66e-08   1.08e-07   4.41e-02   4.65e-05
    7_done_gamma0     9.18e-08   5.30e-08   3.33e-07   1.07e-07   6.27e-08   5.31e-02   1.70e-05
    8_33_workgroups   1.03e-07   6.45e-08   6.13e-08   1.50e-07   1.23e-07   3.60e-04   3.77e-05
    9_all_done        4.49e-08   2.28e-08   1.73e-07   9.78e-08   7.43e-08   1.98e-01   2.94e-05
    10_saturated      4.75e-08   8.33e-09   6.22e-23   2.80e-07   6.21e-08   3.90e+01   5.96e-05
    hid64             5.57e-08   8.82e-08   1.92e-07   8.69e-08   6.21e-08   2.01e-01   3.02e-05
    ema               1.32e-07   9.56e-08   2.66e-07   1.04e-07   6.82e-08   1.17e-02   2.05e-05
    worst             1.32e-07   1.17e-07   3.33e-07   2.80e-07   1.23e-07
    another machine   (8_33_workgroups, 16 threads)    5.49e-07   (every other figure within the worst above)
    airl_ref.FLOOR    1.4e-07    1.2e-07    3.4e-07    5.5e-07    1.3e-07
    airl_ref.TOL      1.12e-06   9.6e-07    2.72e-06   4.4e-06    1e-06 (the ceiling)

`airl_ref.FLOOR` holds the worst figure recorded for each column. torch's float32 sums on the CPU depend on the
machine (thread count, BLAS blocking), so the figures move from host to host -- which is the very difference the
factor 8 in `airl_ref.TOL` (8 x floor, at least 4 fp32 ulps, at most the ceiling of tests/test_disc_fused_gpu.py) is
there for. This test therefore asserts that float32 on the machine it runs on stays within `airl_ref.TOL`: a recorded
floor that understates float32's own error by more than that factor fails here, not on the device.
"""
import pytest
import torch as th

from tests import airl_ref as A


def run_case(case):
    """Both updates of `case` on the float64 oracle and on its float32 twin. Returns (worst deviations, min |x|, min |z|)."""
    data = A.make_data(case)
    _, o64 = A.make_nets(case)
    o32 = A.float32_twin(o64)
    for m, warm in zip(A.norm_modules(o32), (data["warm_base"], data["warm_pot"])):
        m.update_stats(th.as_tensor(warm))
    worst = dict.fromkeys(A.CEILING, 0.0)
    min_x = min_z = float("inf")
    params0 = th.cat([p.detach().reshape(-1) for p in o32.parameters()]).double()
    grads = []
    for u in range(A.N_UPDATES):
        A.load_oracle(o64, o32.state_dict())
        r64 = A.reference_update(o64, A.gathered(case, data, u, th.float64), case.n_expert, case.scale)
        r32 = A.reference_update(o32, A.gathered(case, data, u, th.float32), case.n_expert, case.scale)
        mx, mz = A.conditions(r64)
        min_x, min_z = min(min_x, mx), min(min_z, mz)
        assert [int(n["count"]) for n in r32.norms] == [int(n["count"]) for n in r64.norms]
        assert (r32.stats[[1, 2, 3, 4, 6, 7]] == r64.stats[[1, 2, 3, 4, 6, 7]]).all()
        dev = A.deviations(r32.x, r32.stats[0], r32.stats[5], r32.grad, r32.norms, r64)
        worst = {q: max(worst[q], dev[q]) for q in worst}
        # the twin's parameters move as the device's do: Adam on the update's gradient
        grads.append(r64.grad)
        p_new, _, _ = A.adam_steps(params0, grads)
        th.nn.utils.vector_to_parameters(p_new.float(), o32.parameters())
    return worst, min_x, min_z


@pytest.mark.parametrize("name", list(A.CASES))
def test_case_meets_the_input_conditions_and_the_recorded_noise_floor(name):
    case = A.CASES[name]
    worst, min_x, min_z = run_case(case)
    print(f"\n    {name:<17s} " + " ".join(f"{worst[q]:<10.2e}" for q in ("logits", "loss", "entropy", "grad", "norm"))
          + f" {min_x:<10.2e} {min_z:<10.2e}")
    assert min_x >= A.MIN_ABS_LOGIT, f"a reference logit at {min_x:.3g} of 0: pick another seed for {name}"
    assert min_z >= A.MIN_ABS_PREACT, f"a hidden pre-activation at {min_z:.3g} of 0: pick another seed for {name}"
    for q, v in worst.items():
        assert v <= A.TOL[q], (f"{q}: float32 itself deviates by {v:.3g}, above the tolerance {A.TOL[q]:.3g} derived from "
                               f"the recorded floor {A.FLOOR[q]:.3g}")


def test_tolerances_follow_from_the_floor_and_stay_under_the_ceilings():
    for q, tol in A.TOL.items():
        assert tol <= A.CEILING[q]
        assert tol == min(A.CEILING[q], max(8.0 * A.FLOOR[q], 4.0 * A.ULP))


def test_reference_update_is_the_oracle_modules_own_training_step():
    """`reference_update` against the pieces of `oracle.imitation_restated.AIRL.train_disc` spelled out: logits from
    `ShapedRewardNet.forward` minus log pi, `binary_cross_entropy_with_logits`, `compute_train_stats`."""
    from oracle import imitation_restated as O

    case = A.CASES["1_baseline"]
    data = A.make_data(case)
    _, o64 = A.make_nets(case)
    sd = {k: v.clone() for k, v in o64.state_dict().items()}
    batch = A.gathered(case, data, 0)
    ref = A.reference_update(o64, batch, case.n_expert, case.scale)
    o64.load_state_dict(sd)
    o64.train(True)
    s, a, ns, d, logp = batch
    x = o64(s, a, ns, d) - logp
    assert th.equal(x.detach(), ref.x)
    labels = th.cat([th.ones(case.n_expert), th.zeros(case.n_gen)]).long()
    loss = th.nn.functional.binary_cross_entropy_with_logits(x, labels.double())
    st = O.compute_train_stats(x.detach(), labels, loss.detach())
    R = case.R
    assert ref.stats[1] == round(st["disc_acc"] * R) and ref.stats[2] == round(st["disc_acc_expert"] * case.n_expert)
    assert ref.stats[3] == round(st["disc_acc_gen"] * case.n_gen)
    assert ref.stats[4] == R - round(st["disc_proportion_expert_pred"] * R)
    assert abs(ref.stats[5] / R - st["disc_entropy"]) < 1e-12 and abs(ref.stats[0] - case.scale * float(loss.detach())) < 1e-15
    assert ref.stats[6] == st["n_expert"] and ref.stats[7] == st["n_generated"]
    # three evaluations were hooked (base; potential on s', on s), the potential's norm absorbed 2 R rows
    assert len(ref.preacts) == 1 + 2 * 2 and len(ref.norm_trace) == 3
    assert int(ref.norms[0]["count"]) == R and int(ref.norms[1]["count"]) == 2 * R
    assert int(ref.norm_trace[1]["count"]) == R


def test_float64_adam_is_torch_adam():
    g = th.Generator().manual_seed(0)
    p0 = th.randn(50, generator=g, dtype=th.float64)
    grads = [th.randn(50, generator=g, dtype=th.float64) * 10.0 ** -k for k in (0, 4)]
    p = th.nn.Parameter(p0.clone())
    opt = th.optim.Adam([p], lr=1e-3)
    for gr in grads:
        p.grad = gr.clone()
        opt.step()
    got, m, v = A.adam_steps(p0, grads)
    th.testing.assert_close(got, p.detach(), rtol=1e-13, atol=1e-15)
    th.testing.assert_close(m, opt.state[p]["exp_avg"], rtol=1e-13, atol=0)
    th.testing.assert_close(v, opt.state[p]["exp_avg_sq"], rtol=1e-13, atol=0)
