"""The float64 policy-forward reference of `tests/policy_forward_ref.py`, validated and measured on the CPU (no GPU, no HIP
library).

For every case of `tests/policy_forward_ref.py` (all cases of tests/test_policy_forward_gpu.py):
  * validation and floor: the float64 reference against the float32 oracle (the same `ActorCriticPolicy` in torch's CPU
    float32, on one thread) in the measures of `policy_forward_ref.deviations`; the figures are what `FLOOR` records
    (worst over the cases and over the thread counts and vector widths named there, rounded up to two digits); a larger
    figure fails here. The inverse-CDF picks and the modes are equal on every row (the tie case: the float32 mode is one of
    the tied pair -- on the CPU two columns of one matrix product need not come out bit-equal);
  * guards: `policy_forward_ref.assert_guards` holds on every row; each case's seed was picked by
    `python -m tests.test_policy_forward_ref seeds` so that it does.
Sensitivity: the float32 oracle with one deliberate restatement error is out of tolerance at least tenfold on the case
meant to catch it.

`python -m tests.test_policy_forward_ref` prints this table (cdf: the smallest distance of a row's u from a CDF boundary;
gap: the smallest lead of the top logit; small / big: the fractions of first-layer pre-activations with |x| <= 0.1 / >= 4):

    case                           head      actions   values    logp      entropy   cdf       gap       small  big
    1x1b_h32_norm                  8.4e-08   7.8e-08   7.7e-08   1.3e-07   1.9e-08   inf       inf       0.40   0.00
    3x2d_h32_norm                  8.0e-08   0.0e+00   1.7e-07   9.0e-08   7.3e-08   5.7e-03   2.3e-03   0.17   0.00
    4x13b_h32_plain                1.4e-07   1.4e-07   1.5e-07   1.7e-07   8.2e-09   inf       inf       0.17   0.00
    5x15d_h32_plain                1.3e-07   0.0e+00   1.6e-07   1.2e-07   1.7e-07   5.6e-04   1.4e-03   0.15   0.00
    16x16b_h32_norm                1.8e-07   1.6e-07   2.0e-07   1.6e-07   4.3e-08   inf       inf       0.06   0.00
    17x1d_h32_norm                 1.2e-07   0.0e+00   2.4e-07   0.0e+00   0.0e+00   inf       inf       0.06   0.00
    33x2b_h32_plain                1.9e-07   2.4e-07   2.7e-07   1.5e-07   1.9e-08   inf       inf       0.05   0.01
    63x13d_h32_plain               2.3e-07   0.0e+00   3.0e-07   1.2e-07   2.3e-07   4.6e-04   1.0e-03   0.05   0.02
    64x15b_h32_norm                2.4e-07   2.0e-07   2.5e-07   1.9e-07   1.6e-08   inf       inf       0.05   0.02
    5x16d_h32_norm                 1.5e-07   0.0e+00   9.8e-08   1.3e-07   1.9e-07   3.2e-05   9.7e-04   0.12   0.00
    33x15b_h32_plain               2.0e-07   2.4e-07   2.3e-07   2.1e-07   1.6e-08   inf       inf       0.05   0.01
    64x1d_h32_plain                2.0e-07   0.0e+00   2.6e-07   0.0e+00   0.0e+00   inf       inf       0.05   0.02
    64x16b_h32_norm                2.4e-07   2.5e-07   2.6e-07   1.6e-07   2.3e-08   inf       inf       0.05   0.03
    64x16d_h32_plain               2.0e-07   0.0e+00   2.5e-07   1.5e-07   1.8e-07   4.7e-04   6.0e-04   0.05   0.02
    1x1d_h64_plain                 9.2e-08   0.0e+00   1.3e-07   0.0e+00   0.0e+00   inf       inf       0.46   0.00
    3x2b_h64_plain                 1.7e-07   1.7e-07   1.9e-07   1.3e-07   8.5e-09   inf       inf       0.27   0.00
    4x13d_h64_norm                 2.5e-07   0.0e+00   1.9e-07   1.4e-07   1.9e-07   5.3e-04   3.3e-03   0.23   0.00
    5x15b_h64_norm                 3.5e-07   2.6e-07   2.5e-07   2.2e-07   6.2e-08   inf       inf       0.17   0.00
    16x16d_h64_plain               2.9e-07   0.0e+00   2.8e-07   1.8e-07   2.0e-07   2.3e-04   2.6e-04   0.10   0.00
    17x1b_h64_plain                1.7e-07   1.4e-07   2.4e-07   1.4e-07   3.1e-10   inf       inf       0.10   0.00
    33x2d_h64_norm                 2.3e-07   0.0e+00   2.5e-07   1.3e-07   9.5e-08   4.2e-04   1.0e-03   0.07   0.00
    63x13b_h64_norm                4.3e-07   3.3e-07   3.4e-07   2.4e-07   4.3e-08   inf       inf       0.05   0.03
    64x15d_h64_plain               4.0e-07   0.0e+00   3.2e-07   1.7e-07   2.2e-07   6.1e-05   9.5e-04   0.05   0.02
    5x16b_h64_plain                2.7e-07   3.4e-07   1.8e-07   1.5e-07   4.0e-08   inf       inf       0.19   0.00
    33x15d_h64_norm                3.7e-07   0.0e+00   2.7e-07   1.8e-07   2.0e-07   1.4e-04   1.5e-03   0.06   0.00
    64x1b_h64_norm                 2.4e-07   1.4e-07   3.0e-07   1.7e-07   1.3e-08   inf       inf       0.05   0.02
    64x16b_h64_plain               3.8e-07   3.5e-07   3.5e-07   1.5e-07   7.6e-08   inf       inf       0.05   0.01
    64x16d_h64_norm                4.0e-07   0.0e+00   3.2e-07   1.7e-07   1.6e-07   3.7e-04   1.3e-03   0.05   0.03
    small_17x6b_h32_norm           2.6e-08   9.1e-08   5.4e-08   1.3e-07   6.4e-08   inf       inf       0.98   0.00
    saturated_17x6b_h32_norm       2.7e-07   2.1e-07   2.6e-07   1.4e-07   6.4e-08   inf       inf       0.01   0.49
    tie_20x13d_h64_plain           2.8e-07   0.0e+00   2.0e-07   1.9e-07   2.4e-07   9.9e-05   8.6e-01   0.08   0.00
    worst: head 4.29e-07, actions 3.53e-07, values 3.47e-07, logp 2.35e-07, entropy 2.44e-07
    the same machine, worst over one and four threads and the AVX2 and AVX-512 kernels:
           head 4.29e-07, actions 4.50e-07, values 5.00e-07, logp 2.35e-07, entropy 2.44e-07
    a second machine, worst lines only -- as `python -m tests.test_policy_forward_ref` prints it there, then on 16 threads:
           head 3.93e-07, actions 4.42e-07, values 3.90e-07, logp 3.13e-07, entropy 2.03e-07
           head 3.91e-07, actions 3.88e-07, values 4.36e-07, logp 2.37e-07, entropy 2.21e-07
    `policy_forward_ref.FLOOR`: per quantity the largest of these worst lines, rounded up to two digits (torch's float32
    CPU kernels are chosen by processor and the figures move by up to 40 % from host to host, which the factor 8 of TOL
    covers).
    policy_forward_ref.TOL: head 3.4e-6, actions 3.6e-6, values 4.0e-6, logp 2.6e-6, entropy 2.0e-6 (all 8 x floor, far
    below the 1e-4 ceiling). Discrete heads have no `actions` figure: picks are compared exactly.
"""
import contextlib

import numpy as np
import pytest
import torch as th

from tests import policy_forward_ref as R


@contextlib.contextmanager
def one_thread():
    """float32 sums on one thread: the measured floor does not depend on how many cores the machine has."""
    n = th.get_num_threads()
    th.set_num_threads(1)
    try:
        yield
    finally:
        th.set_num_threads(n)


_RUNS = {}


def _runs(name):
    """(case, policy, inputs, float64 reference, float32 oracle run): computed once, shared, never changed."""
    if name not in _RUNS:
        case = R.CASES[name]
        with one_thread():
            pol, inp = R.build(case)
            _RUNS[name] = (case, pol, inp, R.reference(case, pol, inp), R.oracle(case, pol, inp))
    return _RUNS[name]


def measure(name):
    case, pol, inp, ref, o32 = _runs(name)
    return R.deviations(R.fields(o32), ref), ref


def _row(name, dev, ref):
    inf = float("inf")
    cdf = ref.cdf_margin.min() if ref.cdf_margin is not None else inf
    gap = ref.logit_gap.min() if ref.logit_gap is not None else inf
    return (f"    {name:<30s} " + " ".join(f"{dev.get(q, 0.0):<9.1e}" for q in R.QUANTITIES)
            + f" {cdf:<9.1e} {gap:<9.1e} {R.fraction_small(ref):<6.2f} {R.fraction_saturated(ref):<6.2f}")


HEADER = f"    {'case':<30s} " + " ".join(f"{q:<9s}" for q in R.QUANTITIES) + f" {'cdf':<9s} {'gap':<9s} {'small':<6s} {'big':<6s}"


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_matches_the_float32_oracle_and_meets_the_guards(name):
    case, pol, inp, ref, o32 = _runs(name)
    dev = R.deviations(R.fields(o32), ref)
    print("\n" + HEADER + "\n" + _row(name, dev, ref))
    R.assert_guards(case, ref)
    assert ref.head.shape == (case.n, case.A) and ref.values.shape == (case.n,) and ref.z1.shape == (2, case.n, case.H)
    if case.discrete:
        assert np.array_equal(o32.pick, ref.pick), "inverse-CDF picks are exact under the guard"
        if case.kind == "tie":
            assert np.isin(o32.mode, R.TIE_ROWS).all()
        else:
            assert np.array_equal(o32.mode, ref.mode), "modes are exact under the guard"
        assert np.allclose(ref.cdf[:, -1], 1.0, atol=1e-12) and (np.diff(ref.cdf, axis=1) >= 0).all()
    floor = R.FLOOR
    over = {q: (float(f"{v:.4g}"), floor[q]) for q, v in dev.items() if v > floor[q]}
    assert not over, f"float32 deviates by more than the recorded floor (measured, recorded): {over}"


def test_the_grid_covers_every_width_for_both_tower_widths():
    for H in (32, 64):
        grid = [R.CASES[n] for n in R.GRID_CASES if R.CASES[n].H == H]
        assert {c.D for c in grid} == set(R.WIDTHS_D) and {c.A for c in grid} == set(R.WIDTHS_A)
        assert {c.discrete for c in grid if (c.D, c.A) == (64, 16)} == {False, True}
        assert {c.norm for c in grid} == {False, True} and {c.discrete for c in grid} == {False, True}
    gauss = [R.CASES[n] for n in R.CASES if not R.CASES[n].discrete]
    assert {c.bounds for c in gauss} == {"unit", "asym", "inf"}
    assert all(c.n <= 130 for c in R.CASES.values())
    assert set(R.GRID_CASES + R.CONDITIONED_CASES) == set(R.CASES)


def test_every_gpu_case_is_a_reference_case():
    from tests import test_policy_forward_gpu as gpu
    listed = set(gpu.ALL_CASES) | set(gpu.GAUSSIAN) | set(gpu.DISCRETE) | set(gpu.ROW_CASES)
    assert listed == set(R.CASES)
    assert set(gpu.GAUSSIAN) | set(gpu.DISCRETE) == set(R.CASES)


def test_tolerances_follow_from_the_floor_and_stay_under_the_ceilings():
    assert set(R.FLOOR) == set(R.CEILING) == set(R.TOL) == set(R.QUANTITIES)
    for q in R.TOL:
        assert R.FLOOR[q] > 0.0, f"{q}: no measured floor recorded"
        assert R.TOL[q] == min(R.CEILING[q], max(8.0 * R.FLOOR[q], 4.0 * R.ULP)) <= R.CEILING[q] == 1e-4


def test_placed_rows_and_the_inverse_cdf():
    assert np.float32(R.U_LAST) == R.U_LAST < 1.0 and np.nextafter(np.float32(R.U_LAST), np.float32(2)) == 1.0
    cdf = np.array([[0.25, 0.5, 1.0], [0.25, 0.5, 0.99999994]])
    assert list(R.inverse_cdf(cdf, np.array([0.0, R.U_LAST]))) == [0, 2]
    assert list(R.inverse_cdf(cdf, np.array([0.25, 0.4999]))) == [1, 1]


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
def _grid(D=None, A=None):
    return [n for n in R.GRID_CASES if (D is None or R.CASES[n].D == D) and (A is None or R.CASES[n].A == A)]


SENSITIVITY = ([(n, "drop_last_column", ("head", "values")) for D in (5, 33) for n in _grid(D=D)]
               + [(n, "head_row", ("head",)) for A in (15, 16) for n in _grid(A=A)]
               + [(R.SATURATED_CASE, "var_without_eps", ("head", "values")), (R.SATURATED_CASE, "cubic_tanh", ("head", "values")),
                  (R.SATURATED_CASE, "value_from_policy_latent", ("values",)), (_grid(D=17)[0], "value_from_policy_latent", ("values",)),
                  (_grid(D=64, A=16)[0], "value_from_policy_latent", ("values",))])


@pytest.mark.parametrize("name,variant,quantities", SENSITIVITY, ids=lambda v: v if isinstance(v, str) else "+".join(v))
def test_a_restatement_error_exceeds_the_tolerance_tenfold(name, variant, quantities):
    """The float32 oracle restated with one error -- the last observation column dropped, action A - 1's head row replaced
    by row A - 2, `var` for `var + eps`, x - x^3 / 3 for tanh, the value head on the policy tower's latent -- against the
    reference, in the measures and tolerances the GPU tests use; the clean oracle is within them."""
    case, pol, inp, ref, o32 = _runs(name)
    tol = R.TOL
    base = R.deviations(R.fields(o32), ref)
    with one_thread():
        bad = R.deviations(R.fields(R.oracle(case, pol, inp, variant)), ref)
    print(f"\n    {name} {variant}: " + "  ".join(f"{q} {bad[q]:.2e} (clean {base[q]:.1e}, tol {tol[q]:.1e})" for q in quantities))
    assert all(base[q] <= tol[q] for q in R.QUANTITIES if q in base)
    for q in quantities:
        assert bad[q] >= 10.0 * tol[q], f"{q}: the case is too weak for this error"


# ---- `python -m tests.test_policy_forward_ref`: the seed search and the table of this docstring ---------------------------------------
def _find_seed(case: R.Case, limit: int = 2000):
    import dataclasses
    for seed in range(limit):
        c = dataclasses.replace(case, seed=seed)
        pol, inp = R.build(c)
        try:
            R.assert_guards(c, R.reference(c, pol, inp))
        except AssertionError:
            continue
        return seed
    raise RuntimeError(case.name)


if __name__ == "__main__":
    import sys
    if "seeds" in sys.argv:
        found = {}
        for c in R.CASES.values():
            s = _find_seed(c)
            if s:
                found[c.name] = s
            print(c.name, s, flush=True)
        print("SEEDS =", found)
    else:
        print(HEADER)
        worst = dict.fromkeys(R.QUANTITIES, 0.0)
        for n in R.CASES:
            dev, ref = measure(n)
            worst.update({q: max(worst[q], v) for q, v in dev.items()})
            print(_row(n, dev, ref))
        print("    worst:", ", ".join(f"{q} {v:.2e}" for q, v in worst.items()))
