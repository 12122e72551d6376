"""The AIRL discriminator update of the shaped reward net against float64, `-m gpu`: the fused update
(`csrc/airl_fused.hip`: `airl_rows_kernel` + three grouped split-K TN GEMMs + `ia_reduce_partials_adam`, through
`ShapedRewardNet.disc_step_fused` and through `ia_airl_step_shaped` directly) and the stack-by-stack path the trainer
falls back to (`ShapedRewardNet.disc_forward` / `disc_backward`). The reference is `tests/airl_ref.py`: the pinned oracle
module in float64, loaded from the HIP net's own state before every update, so each update is judged alone.

Cases (`airl_ref.CASES`; obs_dim, act_dim, flags (state, action, next, done), n_expert + n_gen) and what they reach:
    1   11, 3, (1,1,0,0), 33+31          one workgroup, ragged second wave (baseline)
    2   1, 1, (0,0,0,1), 1+1, no norm    Db = Dp = 1, R = 2: one live lane pair, ld = 4, clamped loads everywhere
    3   4, 2 discrete, 65+64, scale 0.5  one-hot actions; R = 129: second workgroup with one live row and three dead waves;
                                         GEMM splits of 96 + 33 rows
    4   29, 6, (1,1,1,0), 193+192        Db = 64 (maximum, all 8 chunks); R = 385: the last of 4 splits holds one base row
    5   64, 3, (0,1,0,0), 64+65, no norm Dp = 64 (maximum) with Db = 3; gamma 0.9
    6   33, 2, (1,1,0,0), 100+93         Dp = 33, Db = 35: fifth chunk with one / three live columns; gamma = 1
    7   12, 4, (1,1,1,1), 40+40          use_done column; gamma = 0: the next-state deltas must be exactly zero
    8   11, 3, (1,1,0,0), 2050+2050      33 workgroups: second trip of the ticket fold loop, last workgroup of 4 rows
    9   case 1, every done = 1           d h(s') == 0
    10  case 1, log pi = -40 / +40       saturated BCE: log1p(exp(-|x|)), p - y at 0 and +-1
    hid64, ema                           geometries `fused_step_ok()` refuses: stack-by-stack path only

Tolerances (`airl_ref.TOL`), in the measures of `airl_ref.deviations`: 8 x the float32-against-float64 deviation of the
oracle module itself (measured per case in tests/test_airl_ref.py), at least 4 fp32 ulps, at most what
tests/test_disc_fused_gpu.py allows for the same quantity:
    quantity   float32 floor   tolerance   ceiling
    logits     1.4e-07         1.12e-06    1e-05
    loss       1.2e-07         9.6e-07     1e-05
    entropy    3.4e-07         2.72e-06    1e-04
    gradient   5.5e-07         4.4e-06     2e-05   (relative to max |g_ref|)
    norm state 1.3e-07         1e-06       1e-06
Counts (correct, correct expert / generator, predicted generator, n_expert, n_gen, norm sample counts) are exact: no
reference logit is within 1e-4 of 0 and no hidden pre-activation within 1e-5 (asserted on every reference here again).
Adam: parameters, exp_avg, exp_avg_sq after two steps against float64 Adam fed the device's own fp32 gradients,
atol 1e-7 + rtol 1e-6.

Measured on an MI355X, worst over all cases, both paths and both updates: logits 1.8e-07, loss 1.3e-07, entropy
2.8e-07, gradient 1.8e-07, norm state 1.2e-07 -- at the float32 floor, 6 to 24 times under the tolerances. Adam:
parameters within 6.6e-08, exp_avg within 2.2e-08, exp_avg_sq within 6.4e-09 absolute. exp_avg_sq is 1.30e-05 low
RELATIVE to float64 in every case: the kernels form the increment's coefficient as `1.f - beta2` from the fp32-rounded
beta2 (0.00099998713 instead of 0.001), torch rounds 1 - beta2 itself. At these gradient magnitudes that stays under the
absolute bound above (a step differs by 6e-6 of its size); the test prints the figure.
"""
import functools

import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from imitation_amd import networks, reward_nets
from imitation_amd.networks import HipAdam, TransitionTable
from tests import airl_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not th.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


@functools.lru_cache(maxsize=None)
def _data(name):
    return A.make_data(A.CASES[name])


def _dev(x):
    return th.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _table(host, discrete):
    return TransitionTable(_dev(host["obs"]), _dev(host["acts"]), _dev(host["next_obs"]), _dev(host["dones"]), discrete)


def _bits(t):
    return t.detach().contiguous().view(th.int32)


def _assert_bit_identical(a, b, what):
    ia, ib = _bits(a).reshape(-1), _bits(b).reshape(-1)
    if not th.equal(ia, ib):
        ii = th.nonzero(ia != ib).reshape(-1)
        raise AssertionError(f"{what}: {ii.numel()} of {ia.numel()} values differ, first at {ii[:6].tolist()}: "
                             f"{a.reshape(-1)[ii[:3]].tolist()} vs {b.reshape(-1)[ii[:3]].tolist()}")


def _assert_within(dev, what, quantities=tuple(A.TOL)):
    print(f"    {what}: " + "  ".join(f"{q} {dev[q]:.2e} (tol {A.TOL[q]:.2e})" for q in quantities))
    for q in quantities:
        assert dev[q] <= A.TOL[q], f"{what}: {q} deviates by {dev[q]:.3g} from float64, tolerance {A.TOL[q]:.3g}"


# ---- a. one update through the net API ----------------------------------------------------------------------------------------
class _Run:
    """A HIP net on the device with warmed norms, its float64 oracle, tables and the optimiser of one case."""

    def __init__(self, case):
        self.case, self.data = case, _data(case.name)
        self.net, self.oracle = A.make_nets(case)
        self.net.to(DEV)
        self.base, self.pot = self.net._base.mlp, self.net.potential._potential_net
        self.hip_norms = [self.base.norm, self.pot.norm] if case.norm else []
        for n, warm in zip(self.hip_norms, (self.data["warm_base"], self.data["warm_pot"])):
            n.update_stats(_dev(warm))
        self.e_tab, self.g_tab = _table(self.data["expert"], case.discrete), _table(self.data["gen"], case.discrete)
        self.opt = HipAdam(self.net._store.flat, self.net._store.grad, lr=1e-3)
        self.stats = th.zeros(8, device=DEV)
        self.dlogits = th.empty(case.R, device=DEV)
        self.bce_ws = th.zeros(int(L.load().ia_bce_ws_floats(case.R)), device=DEV)

    def sources(self, u):
        upd = self.data["updates"][u]
        return [(self.e_tab, _dev(upd["e_idx"]), self.case.n_expert), (self.g_tab, _dev(upd["g_idx"]), self.case.n_gen)]

    def reference(self, u):
        """The float64 update from the HIP net's present parameters and norm state."""
        A.load_oracle(self.oracle, self.net.state_dict())
        ref = A.reference_update(self.oracle, A.gathered(self.case, self.data, u), self.case.n_expert, self.case.scale)
        A.assert_conditions(ref, f"{self.case.name} update {u}")
        return ref

    def update(self, u, path, adam=True):
        case, logp = self.case, _dev(self.data["updates"][u]["logp"])
        with networks.training(self.net):
            if path == "fused":
                logits = self.net.disc_step_fused(self.sources(u), logp, case.scale, self.stats, self.opt if adam else None)
            else:   # the trainer's general schedule (adversarial/common.py: disc_forward, BCE, disc_backward, optimiser step)
                logits = self.net.disc_forward(self.sources(u), case.n_expert, logp)
                L.call("ia_bce_logits", L.ptr(logits), case.R, case.n_expert, case.scale, L.ptr(self.dlogits),
                       L.ptr(self.stats), L.ptr(self.bce_ws), L.stream())
                assert not self.net.disc_backward(self.dlogits, accumulate=False)
                self.opt.step()
        th.cuda.synchronize()
        return dict(logits=logits.detach().cpu().clone(), stats=self.stats.cpu().double().numpy().copy(),
                    grad=self.opt.grad.detach().cpu().clone(), norms=[A.norm_state(n) for n in self.hip_norms])


def _check_update(run, u, path, got, ref, counts_before):
    case = run.case
    dev = A.deviations(got["logits"], got["stats"][0], got["stats"][5], got["grad"], got["norms"], ref)
    _assert_within(dev, f"{case.name} [{path}] update {u}")
    exact = [1, 2, 3, 4, 6, 7]
    assert (got["stats"][exact] == ref.stats[exact]).all(), (got["stats"], ref.stats)
    assert got["stats"][6] == case.n_expert and got["stats"][7] == case.n_gen
    for k, (n, want, before) in enumerate(zip(got["norms"], ref.norms, counts_before)):
        assert int(n["count"]) == int(want["count"]) == before + (k + 1) * case.R   # base + R, potential + 2 R
    if case.gamma == 0.0 or case.all_done:   # nothing may flow into h(s')
        if path == "fused":
            ws = run.net._fused[0]
            assert not ws["Dp1"][:case.R].any() and not ws["Dp2"][:case.R].any()
        else:
            assert not run.net._last[3]["dh_next"].any()


def _two_updates(case, path):
    run = _Run(case)
    params0 = run.net._store.flat.detach().cpu().clone()
    grads = []
    for u in range(A.N_UPDATES):
        counts = [int(n.count) for n in run.hip_norms]
        ref = run.reference(u)
        got = run.update(u, path)
        _check_update(run, u, path, got, ref, counts)
        grads.append(got["grad"])
    # Adam, bias correction of step 2 included, against float64 Adam on the device's own gradients
    p64, m64, v64 = A.adam_steps(params0, grads, lr=1e-3)
    for name, got_t, want in (("parameters", run.net._store.flat, p64), ("exp_avg", run.opt.exp_avg, m64),
                              ("exp_avg_sq", run.opt.exp_avg_sq, v64)):
        g64 = got_t.detach().cpu().double()
        print(f"    {case.name} [{path}] Adam {name}: max |d| {float((g64 - want).abs().max()):.2e}, "
              f"max |d| / |ref| {float(((g64 - want).abs() / want.abs().clamp_min(1e-30)).max()):.2e}")
        th.testing.assert_close(g64, want, atol=A.ADAM_ATOL, rtol=A.ADAM_RTOL, msg=lambda m, n=name: f"Adam {n}: {m}")
    assert run.opt.step_count == 2


@pytest.mark.parametrize("path", ["fused", "stacks"])
@pytest.mark.parametrize("name", A.FUSED_CASES)
def test_shaped_update_matches_float64(name, path, monkeypatch):
    case = A.CASES[name]
    if path == "stacks":
        monkeypatch.setattr(reward_nets, "FUSED_AIRL_STEP", False)
    else:
        probe, _ = A.make_nets(case)
        assert probe.fused_step_ok(), "the case must take the fused update"
    _two_updates(case, path)


@pytest.mark.parametrize("name", A.STACKS_ONLY_CASES)
def test_stack_by_stack_update_matches_float64_where_the_fused_update_refuses(name):
    case = A.CASES[name]
    probe, _ = A.make_nets(case)
    assert reward_nets.FUSED_AIRL_STEP and not probe.fused_step_ok()
    _two_updates(case, "stacks")


def test_fused_finish_without_adam_leaves_the_same_gradient_bit_for_bit():
    """`fused_finish(adam=None)` (`ia_reduce_partials` into the store's gradient; the trainer's form under the gradient
    penalty) against the Adam form's gradient output, from identical states."""
    case = A.CASES["1_baseline"]
    outs = []
    for adam in (True, False):
        run = _Run(case)
        got = run.update(0, "fused", adam=adam)
        outs.append((got, run.net._store.grad.detach().cpu().clone()))
    _assert_bit_identical(outs[0][0]["logits"], outs[1][0]["logits"], "logits")
    _assert_bit_identical(outs[0][1], outs[1][1], "gradient in the store")
    assert outs[1][1].abs().max() > 0


# ---- b. ia_airl_step_shaped called directly -------------------------------------------------------------------------------------
WORKSPACES = ("Ab", "Db1", "Ap", "H1", "Dp1", "Dp2", "part", "logits", "bce_part", "stats")


class _Direct:
    """Buffers of one `ia_airl_step_shaped` call, built as `fused_prepare` / `fused_finish` build them, for update 0 of a
    case. `pad`: extra floats per row of Xb / Sn / Sc (and of the normalised copies), padding columns set to 1e6.
    `fill`: initial content of every workspace the call writes. `train`: statistics as the train-mode updates leave them
    (the oracle's, rounded to fp32; potential: after s' and after s) or frozen (the eval-mode call: A and B the same)."""

    def __init__(self, case, pad=0, fill=0.0, train=True, n_expert=None, with_ref=True):
        self.case = case
        data = _data(case.name)
        net, oracle = A.make_nets(case)
        norms = A.norm_modules(oracle)
        for m, warm in zip(norms, (data["warm_base"], data["warm_pot"])):
            m.update_stats(th.as_tensor(warm).double())
        A.load_oracle(oracle, {k: (v.float() if v.is_floating_point() else v) for k, v in oracle.state_dict().items()})
        batch = A.gathered(case, data, 0)
        R, Db, Dp = case.R, case.Db, case.od
        self.R, self.Db, self.Dp = R, Db, Dp
        self.n_expert = case.n_expert if n_expert is None else n_expert
        self.ref = None
        if with_ref or (train and norms):
            self.ref = A.reference_update(oracle, batch, self.n_expert, case.scale, train=train)
        f32 = lambda t: t.float().to(DEV).contiguous()
        self.nst = None
        if norms:   # base, potential after s', potential after s
            if train:
                self.nst = [(f32(t["mean"]), f32(t["var"])) for t in self.ref.norm_trace]
            else:
                b, q = [(f32(m.running_mean), f32(m.running_var)) for m in norms]
                self.nst = [b, q, q]   # (literally the same arrays twice)
        self.beps = float(norms[0].eps) if norms else 0.0
        flat = net._store.flat.detach().to(DEV).contiguous()
        self.flat, self.nb = flat, net._base.mlp.n_params
        self.ldb, self.ldp = (Db + 3) // 4 * 4 + pad, (Dp + 3) // 4 * 4 + pad

        def padded(x, ld):
            out = th.full((R, ld), 1e6 if pad else 0.0, device=DEV)
            out[:, :x.shape[1]] = x.float().to(DEV)
            return out

        s, _, ns, d, logp = batch
        self.Xb, self.Sn, self.Sc = padded(A.base_inputs(case, batch), self.ldb), padded(ns, self.ldp), padded(s, self.ldp)
        self.dones, self.logp = f32(d), f32(logp)
        self.nblk = int(L.load().ia_airl_fused_slabs(R))
        P = flat.numel()
        mk = lambda *shape: th.full(shape, fill, device=DEV)
        self.ws = dict(Ab=mk(R, self.ldb), Db1=mk(R, 32), Ap=mk(2 * R, self.ldp), H1=mk(2 * R, 32), Dp1=mk(2 * R, 32),
                       Dp2=mk(2 * R, 32), part=mk(self.nblk, P), logits=mk(R), bce_part=mk(self.nblk * 8), stats=mk(8))
        self.ticket = th.zeros(1, dtype=th.int32, device=DEV)
        self.grad = th.zeros(P, device=DEV)

    def call(self, **over):
        """Returns the entry point's code. `over`: arguments replaced by name (the refusal checks)."""
        w, st = self.ws, self.nst
        p = lambda t: None if t is None else t.data_ptr()
        a = dict(Xb=p(self.Xb), ldb=self.ldb, Db=self.Db, Sn=p(self.Sn), Sc=p(self.Sc), ldp=self.ldp, Dp=self.Dp,
                 dones=p(self.dones), logp=p(self.logp),
                 bmean=p(st[0][0]) if st else None, bvar=p(st[0][1]) if st else None, beps=self.beps,
                 pmeanA=p(st[1][0]) if st else None, pvarA=p(st[1][1]) if st else None,
                 pmeanB=p(st[2][0]) if st else None, pvarB=p(st[2][1]) if st else None, peps=self.beps,
                 params_base=p(self.flat), params_pot=self.flat.data_ptr() + 4 * self.nb, gamma=self.case.gamma,
                 scale=self.case.scale, R=self.R, n_expert=self.n_expert, Ab=p(w["Ab"]), ldab=self.ldb, Db1=p(w["Db1"]),
                 Ap=p(w["Ap"]), ldap=self.ldp, H1=p(w["H1"]), Dp1=p(w["Dp1"]), Dp2=p(w["Dp2"]), partials=p(w["part"]),
                 logits=p(w["logits"]), stats=p(w["stats"]), bce_part=p(w["bce_part"]), ticket=p(self.ticket), adam=None,
                 stream=L.stream())
        assert set(over) <= set(a)
        a.update(over)
        rc = L.load().ia_airl_step_shaped(*a.values())
        th.cuda.synchronize()
        return rc

    def outputs(self):
        """logits, statistics row, split-K partial buffer and the gradient reduced from it (clones)."""
        L.call("ia_reduce_partials", L.ptr(self.ws["part"]), self.nblk, self.grad.numel(), 1.0, 0, L.ptr(self.grad), L.stream())
        th.cuda.synchronize()
        return {k: v.clone() for k, v in (("logits", self.ws["logits"]), ("stats", self.ws["stats"]),
                                          ("part", self.ws["part"]), ("grad", self.grad))}

    def check_against_reference(self, out, what):
        st = out["stats"].cpu().double().numpy()
        dev = A.deviations(out["logits"], st[0], st[5], out["grad"], self.ref.norms, self.ref)   # (norms: the oracle's own)
        _assert_within(dev, what, ("logits", "loss", "entropy", "grad"))
        exact = [1, 2, 3, 4, 6, 7]
        assert (st[exact] == self.ref.stats[exact]).all(), (st, self.ref.stats)


def _same_outputs(a, b, what):
    for k in ("logits", "stats", "part", "grad"):
        _assert_bit_identical(a[k], b[k], f"{what}: {k}")


def test_direct_call_needs_no_workspace_but_the_ticket_initialised():
    """Every workspace the call writes poisoned with NaN: the entry point's contract asks for a zeroed ticket only, so
    logits, statistics, every slab of the partial buffer and the reduced gradient must come out as from zeroed ones --
    and match float64 (train-mode statistics)."""
    case = A.CASES["1_baseline"]
    clean, poisoned = _Direct(case, fill=0.0), _Direct(case, fill=NAN)
    assert clean.call() == 0 and poisoned.call() == 0
    a, b = clean.outputs(), poisoned.outputs()
    assert all(bool(th.isfinite(v).all()) for v in b.values())
    _same_outputs(a, b, "NaN-poisoned workspaces")
    clean.check_against_reference(a, "direct call, train-mode statistics")


def test_direct_call_ignores_row_padding():
    """Rows eight floats wider than the padded width, padding columns of Xb / Sn / Sc at 1e6: bit-identical results."""
    case = A.CASES["1_baseline"]
    tight, wide = _Direct(case), _Direct(case, pad=8)
    assert wide.ldb == tight.ldb + 8 and wide.ldp == tight.ldp + 8
    assert tight.call() == 0 and wide.call() == 0
    _same_outputs(tight.outputs(), wide.outputs(), "padded rows")


@pytest.mark.parametrize("which", ["none_expert", "all_expert", "mixed"])
def test_direct_call_with_frozen_statistics_and_degenerate_labels(which):
    """The eval-mode call (pmeanA / pvarA and pmeanB / pvarB the same arrays) against the oracle in eval mode, with the
    ordinary labels and with n_expert = 0 and n_expert = R."""
    case = A.CASES["1_baseline"]
    n_expert = dict(none_expert=0, all_expert=case.R, mixed=case.n_expert)[which]
    d = _Direct(case, train=False, n_expert=n_expert)
    assert d.nst[1][0].data_ptr() == d.nst[2][0].data_ptr() and d.nst[1][1].data_ptr() == d.nst[2][1].data_ptr()
    assert d.call() == 0
    out = d.outputs()
    d.check_against_reference(out, f"frozen statistics, n_expert = {n_expert}")
    st = out["stats"].cpu().numpy()
    assert st[6] == n_expert and st[7] == case.R - n_expert


@pytest.mark.parametrize("name", ["1_baseline", "8_33_workgroups"])
def test_direct_call_is_reusable_and_deterministic(name):
    """Twice on the same workspaces without re-zeroing the ticket (one workgroup, and 33: the ticket fold's second trip):
    every output bit-identical, the ticket back at 0."""
    d = _Direct(A.CASES[name], with_ref=False)
    assert d.nblk == (33 if name == "8_33_workgroups" else 1)
    assert d.call() == 0
    first = d.outputs()
    assert int(d.ticket[0]) == 0
    assert d.call() == 0
    second = d.outputs()
    assert int(d.ticket[0]) == 0
    _same_outputs(first, second, "second call on the same workspaces")
    assert first["stats"][6] == d.n_expert and bool(th.isfinite(first["grad"]).all())


@pytest.mark.parametrize("over", [dict(Db=65), dict(Dp=0), dict(ldb=18), dict(ldab=12)])
def test_direct_call_refuses_unsupported_arguments_without_touching_outputs(over):
    """Argument checks only: IA_ERR_UNSUPPORTED before anything is launched, logits and statistics untouched."""
    d = _Direct(A.CASES["1_baseline"], with_ref=False)
    assert d.Db == 14 and d.ldb == 16 and d.Dp == 11   # (ldab = 12 < 16 = Db rounded up to 4)
    d.ws["logits"].fill_(123.0)
    d.ws["stats"].fill_(123.0)
    assert d.call(**over) == L.ERR_UNSUPPORTED
    assert bool((d.ws["logits"] == 123.0).all()) and bool((d.ws["stats"] == 123.0).all())
    assert int(d.ticket[0]) == 0
