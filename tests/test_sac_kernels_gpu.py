"""The SAC kernels of csrc/sac.hip and a whole step (`SACPolicy.update`) against float64 torch autograd on the CPU from the same
float32 inputs.

The rule is `test_td3_kernels_gpu.py`'s: the device's deviation from the float64 evaluation may be at most 4 x the deviation
of torch's own float32 evaluation, floored at half a float32 epsilon, one scale per phase (the largest deviation over the
phase's outputs). What has one right answer -- copied observation columns, the clamped log_std, which elements the clamp bound,
the argmin records, the 0 / 1 seeds -- is compared exactly. Parameters after Adam are held to a float64 Adam applied to the
kernel's OWN gradient, and the actor phase is restated from the device's own updated critic, as there.
"""
import ctypes as C

import numpy as np
import pytest
import torch as th
from torch.nn import functional as F

import imitation_amd as p
from imitation_amd import _lib as L
from tests.test_td3_kernels_gpu import GAMMA, HALF_EPS, LR, TAU, Case, dev_t, rel, stack_forward, torch_adam

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1), (5, 2), (17, 6)]
BATCHES = [1, 7, 64, 257, 300]   # below one wave, a ragged tail, past one 256-thread workgroup
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8


def i8(*shape):
    return th.zeros(*shape, dtype=th.int8, device="cuda")


def f32(*shape):
    return th.empty(*shape, device="cuda")


def squash(head, eps, A):
    """[SB3 Actor.action_log_prob] from the head output [mu | log_std] in the dtype of `head`."""
    mu, raw = head[:, :A], head[:, A:]
    std = raw.clamp(-20, 2).exp()
    u = mu + eps.to(head.dtype) * std
    a = th.tanh(u)
    logp = th.distributions.Normal(mu, std).log_prob(u).sum(dim=1) - th.log(1 - a ** 2 + 1e-6).sum(dim=1)
    return a, logp


def make_head(g, B, A):
    """Head outputs whose log_std the clamp binds below on some elements, above on some and on neither for the rest, and
    whose |u| reaches about 9 (where 1 - a^2 underflows in float32 and the 1e-6 carries the log-probability)."""
    mu = g.normal(size=(B, A)).astype(np.float32)
    raw = g.uniform(-3, 1, size=(B, A)).astype(np.float32)
    kind = np.arange(B * A).reshape(B, A) % 7
    raw[kind == 1] = g.uniform(-30, -20.5, size=int((kind == 1).sum()))
    raw[kind == 2] = g.uniform(2.5, 6, size=int((kind == 2).sum()))
    big = kind == 3
    mu[big] = (g.choice([-1.0, 1.0], size=int(big.sum())) * g.uniform(4, 9, size=int(big.sum()))).astype(np.float32)
    raw[big] = -4.0
    if big.any():
        mu[tuple(np.argwhere(big)[0])] = 9.0
    eps = g.normal(size=(B, A)).astype(np.float32)
    return np.concatenate([mu, raw], axis=1), eps


def run_sample(head, eps, S, B, D, A, ld):
    out = dict(X=th.full((B, ld), 7.0, device="cuda"), logp=f32(B), a=f32(B, A), ls=f32(B, A), om=f32(B, A), bound=i8(B, A))
    ins = [dev_t(head), None if eps is None else dev_t(eps), dev_t(S)]
    L.call("ia_sac_sample", *(L.ptr(t) for t in ins), B, D, A, ld, *(L.ptr(out[k]) for k in ("X", "logp", "a", "ls", "om", "bound")),
           L.stream())
    return {k: v.cpu().numpy() for k, v in out.items()}, out, ins


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("D,A", SHAPES)
def test_sample_actions_and_log_probabilities(D, A, B, pad):
    g = np.random.default_rng(100 * B + A)
    ld = D + A + pad
    head, eps = make_head(g, B, A)
    S = g.normal(size=(B, D)).astype(np.float32)
    got, _, _ = run_sample(head, eps, S, B, D, A, ld)
    again, _, _ = run_sample(head, eps, S, B, D, A, ld)
    for k in got:
        assert np.array_equal(got[k], again[k]), k   # a launch repeats bit for bit
    raw = head[:, A:]
    assert np.array_equal(got["X"][:, :D], S) and not got["X"][:, D + A:].any()
    assert np.array_equal(got["X"][:, D:D + A], got["a"]) and np.abs(got["a"]).max() <= 1
    assert np.array_equal(got["ls"], np.clip(raw, -20, 2).astype(np.float32))
    assert np.array_equal(got["bound"], (raw > 2).astype(np.int8) - (raw < -20).astype(np.int8))
    if B * A >= 7:
        assert (got["bound"] == -1).any() and (got["bound"] == 1).any() and (got["bound"] == 0).any()
    (a64, l64), (a32, l32) = (squash(th.from_numpy(head).to(t), th.from_numpy(eps), A) for t in (th.float64, th.float32))
    u64 = th.from_numpy(head[:, :A]).double() + th.from_numpy(eps).double() * th.from_numpy(got["ls"]).double().exp()
    if B * A >= 4:
        assert float(u64.abs().max()) > 8   # the saturated end is reached
    om64 = (1 - a64 ** 2).numpy()
    dev = max(rel(a32, a64), rel(l32, l64), HALF_EPS)
    res = (rel(got["a"], a64), rel(got["logp"], l64))
    print(f"sample D {D} A {A} B {B} pad {pad}: torch32 {dev:.3e}, device {res}")
    assert max(res) <= 4 * dev, (res, dev)
    assert rel(got["om"], om64) <= 4 * max(rel((1 - a32 ** 2).numpy(), om64), HALF_EPS)
    # eps == NULL: the deterministic action tanh(mu)
    det, _, _ = run_sample(head, None, S, B, D, A, ld)
    m64 = th.tanh(th.from_numpy(head[:, :A]).double())
    assert rel(det["a"], m64) <= 4 * max(rel(th.tanh(th.from_numpy(head[:, :A])), m64), HALF_EPS)


@pytest.mark.parametrize("B", BATCHES)
def test_alpha_step_against_a_float64_adam_over_three_steps(B):
    g = np.random.default_rng(B)
    te = -2.0
    state = dev_t(np.array([-0.7, 0.0, 0.0, 0.0], np.float32))   # log_ent_coef, exp_avg, exp_avg_sq, alpha slot
    ptr = state.data_ptr()
    prev = state.cpu().numpy()   # the device's own state before each step
    for t in range(1, 4):
        logp = (g.normal(size=B) * 2 + 1.5 - t).astype(np.float32)
        lec = float(state[0].cpu())
        stats, lp = f32(2), dev_t(logp)
        step = np.array([LR / (1 - B1 ** t), (1 - B2 ** t) ** 0.5], np.float32)
        L.call("ia_sac_alpha_step", L.ptr(lp), B, te, ptr, ptr + 4, ptr + 8, B1, B2, ADAM_EPS, float(step[0]), float(step[1]),
               ptr + 12, L.ptr(stats), L.stream())
        s, st = state.cpu().numpy().astype(np.float64), stats.cpu().numpy()
        assert st[0] == s[3]   # the slot and the stats block hold the same alpha: that of BEFORE the step
        term64 = th.from_numpy(logp).double() + te
        loss64, loss32 = float(-(lec * term64).mean()), float(-(th.tensor(lec) * (th.from_numpy(logp) + te)).mean())
        a64, a32 = float(np.exp(np.float64(lec))), float(th.exp(th.tensor(lec)))
        dev = max(abs(loss32 - loss64) / abs(loss64), abs(a32 - a64) / a64, HALF_EPS)
        res = (abs(st[1] - loss64) / abs(loss64), abs(st[0] - a64) / a64)
        assert max(res) <= 4 * dev, (t, res, dev)
        grad = np.array([np.float32(-float(term64.mean()))])   # the kernel's own gradient: the rounded float64 mean
        want = torch_adam(prev[:1], grad, prev[1:2], prev[2:3], t - 1, th.float64)
        t32 = torch_adam(prev[:1].copy(), grad, prev[1:2], prev[2:3], t - 1, th.float32)
        for name, gv, wv, tv in zip(("log_ent_coef", "exp_avg", "exp_avg_sq"), s[:3], want, t32):
            assert abs(gv - wv[0]) <= 4 * max(abs(tv[0] - wv[0]), HALF_EPS * abs(wv[0])), (t, name, gv, wv, tv)
        prev = state.cpu().numpy()
    assert prev[0] != np.float32(-0.7) and prev[1] != 0 and prev[2] > 0


@pytest.mark.parametrize("n_critics", [1, 2])
@pytest.mark.parametrize("B", BATCHES)
def test_critic_loss_against_float64_and_repeats_bit_for_bit(B, n_critics):
    g = np.random.default_rng(B + n_critics)
    q = g.normal(size=(n_critics, B)).astype(np.float32)
    qt = g.normal(size=(n_critics, B)).astype(np.float32)
    logp2 = (g.normal(size=B) - 1).astype(np.float32)
    rew = (g.uniform(size=B) < 0.5).astype(np.float32)
    done = (np.arange(B) % 3 == 0).astype(np.float32)
    alpha = np.float32(0.37)

    def ref(dtype):
        f = lambda x: th.from_numpy(np.asarray(x)).to(dtype)
        cur = f(q).clone().requires_grad_()
        mn = f(qt).min(dim=0)
        y = f(rew) + (1 - f(done)) * GAMMA * (mn.values - f(alpha) * f(logp2))
        loss = 0.5 * sum(F.mse_loss(cur[i], y) for i in range(n_critics))
        loss.backward()
        return float(loss.detach()), cur.grad.numpy(), y.numpy(), mn.indices.numpy().astype(np.int8)

    runs = []
    ins = [dev_t(q), dev_t(qt), dev_t(logp2), dev_t(rew), dev_t(done), dev_t(np.array([alpha]))]
    for _ in range(2):
        dq, y, am, loss = f32(n_critics, B), f32(B), i8(B) + 5, f32(1)
        L.call("ia_sac_critic_loss", *(L.ptr(t) for t in ins), B, n_critics, GAMMA, L.ptr(dq), L.ptr(y), L.ptr(am), L.ptr(loss),
               L.stream())
        runs.append((float(loss.cpu()), dq.cpu().numpy(), y.cpu().numpy(), am.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and all(np.array_equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))
    (l64, g64, y64, am64), (l32, g32, y32, _) = ref(th.float64), ref(th.float32)
    dev = max(abs(l32 - l64) / abs(l64), rel(g32, g64), rel(y32, y64), HALF_EPS)
    got = (abs(runs[0][0] - l64) / abs(l64), rel(runs[0][1], g64), rel(runs[0][2], y64))
    print(f"critic loss B {B} critics {n_critics}: torch32 {dev:.3e}, device {got}")
    assert max(got) <= 4 * dev, (got, dev)
    assert np.array_equal(runs[0][3], am64)
    if B > 1:
        assert (done == 1).any() and (done == 0).any()
        assert n_critics == 1 or ((am64 == 0).any() and (am64 == 1).any())   # each critic is the minimum somewhere


@pytest.mark.parametrize("n_critics", [1, 2])
@pytest.mark.parametrize("B", BATCHES)
def test_min_seed_selects_the_first_minimum(B, n_critics):
    g = np.random.default_rng(B)
    q = g.normal(size=(n_critics, B)).astype(np.float32)
    if n_critics == 2:
        q[1, B // 2] = q[0, B // 2]   # one exact tie: it goes to the first critic
    qd = dev_t(q)
    seeds, minq, am = th.full((n_critics, B), 7.0, device="cuda"), f32(B), i8(B) + 5
    L.call("ia_sac_min_seed", L.ptr(qd), B, n_critics, L.ptr(seeds), L.ptr(minq), L.ptr(am), L.stream())
    mn = th.from_numpy(q).min(dim=0)
    assert np.array_equal(am.cpu().numpy(), mn.indices.numpy().astype(np.int8)) and int(am[B // 2]) == 0
    assert np.array_equal(minq.cpu().numpy(), mn.values.numpy())
    assert np.array_equal(seeds.cpu().numpy(), np.stack([(mn.indices.numpy() == i).astype(np.float32) for i in range(n_critics)]))
    if n_critics == 2 and B >= 7:
        assert (mn.indices == 0).any() and (mn.indices == 1).any()
    if n_critics == 1:
        assert (seeds == 1).all()


def make_critic(D, A, arch, n_critics, seed):
    th.manual_seed(seed)
    c = p.ContinuousCritic(p.Box(-np.inf, np.inf, (D,)), p.Box(-1, 1, (A,)), list(arch), n_critics=n_critics)
    c._flat = c._flat.to("cuda").contiguous()
    return c


@pytest.mark.parametrize("n_critics", [1, 2])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("D,A", SHAPES)
def test_actor_seed_against_autograd_through_real_critics(D, A, B, n_critics):
    g = np.random.default_rng(B + 10 * A + n_critics)
    ld, alpha = D + A + 1, np.float32(0.6)
    head, eps = make_head(g, B, A)
    S = g.normal(size=(B, D)).astype(np.float32)
    crit = make_critic(D, A, (32, 24), n_critics, seed=B)
    sc, nq = crit.stacks[0], crit.stacks[0].numel
    got, dev_out, ins = run_sample(head, eps, S, B, D, A, ld)
    hid = [f32(B * sc.hidden_per_row) for _ in range(n_critics)]
    dhid, scratch = f32(B * sc.hidden_per_row), f32(1, nq)
    qpi, seeds, minq, am = f32(n_critics, B), f32(n_critics, B), f32(B), i8(B)
    dX = [f32(B, ld) for _ in range(n_critics)]
    st = L.stream()
    for i in range(n_critics):
        L.call("ia_mlp_forward", C.byref(sc.desc), crit._flat.data_ptr() + 4 * i * nq, L.ptr(dev_out["X"]), ld, B, L.ptr(hid[i]),
               qpi.data_ptr() + 4 * i * B, L.ACT_NONE, st)
    L.call("ia_sac_min_seed", L.ptr(qpi), B, n_critics, L.ptr(seeds), L.ptr(minq), L.ptr(am), st)
    for i in range(n_critics):
        L.call("ia_mlp_backward", C.byref(sc.desc), crit._flat.data_ptr() + 4 * i * nq, L.ptr(dev_out["X"]), ld, B, L.ptr(hid[i]),
               seeds.data_ptr() + 4 * i * B, L.ptr(dhid), L.ptr(scratch), 1, L.ptr(dX[i]), st)
    slot = dev_t(np.array([alpha]))
    runs = []
    for _ in range(2):
        dhead, loss = f32(B, 2 * A), f32(1)
        L.call("ia_sac_actor_seed", L.ptr(dX[0]), L.ptr(dX[1]) if n_critics == 2 else None, ld, D, L.ptr(dev_out["a"]),
               L.ptr(dev_out["om"]), L.ptr(ins[1]), L.ptr(dev_out["ls"]), L.ptr(dev_out["bound"]), L.ptr(slot),
               L.ptr(dev_out["logp"]), L.ptr(minq), B, A, L.ptr(dhead), L.ptr(loss), st)
        runs.append((float(loss.cpu()), dhead.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    flat = crit._flat.cpu()

    def autograd(dtype):
        h = th.from_numpy(head).to(dtype).requires_grad_()
        a, logp = squash(h, th.from_numpy(eps), A)
        x = th.cat([th.from_numpy(S).to(dtype), a], dim=1)   # (the tile's pad column is no input of the critics)
        q = th.cat([stack_forward(flat[i * nq:(i + 1) * nq].to(dtype), sc.dims, x, False) for i in range(n_critics)], dim=1)
        mn = q.min(dim=1)
        loss = (float(alpha) * logp - mn.values).mean()
        loss.backward()
        return float(loss.detach()), h.grad.numpy(), mn.indices.numpy().astype(np.int8)

    (l64, g64, am64), (l32, g32, _) = autograd(th.float64), autograd(th.float32)
    assert np.array_equal(am.cpu().numpy(), am64)   # no near tie in this construction: one gradient route for all
    dev = max(abs(l32 - l64) / abs(l64), rel(g32, g64), HALF_EPS)
    res = (abs(runs[0][0] - l64) / abs(l64), rel(runs[0][1], g64))
    print(f"actor seed D {D} A {A} B {B} critics {n_critics}: torch32 {dev:.3e}, device {res}")
    assert max(res) <= 4 * dev, (res, dev)
    bound = got["bound"] != 0
    assert not runs[0][1][:, A:][bound].any() and not g64[:, A:][bound].any()   # clamp-bound: exactly zero
    if B * A >= 7:
        assert bound.any() and runs[0][1][:, A:][~bound].all()


# ---- a whole step ----------------------------------------------------------------------------------------------------------

def make_policy(D, A, arch, n_critics, learned, seed):
    th.manual_seed(seed)
    pol = p.SACPolicy(p.Box(-np.inf, np.inf, (D,)), p.Box(-1, 1, (A,)), lambda _: LR, net_arch=list(arch), n_critics=n_critics)
    g = th.Generator().manual_seed(seed + 1)
    pol._target.add_(0.05 * th.randn(pol._target.shape, generator=g))   # a target that differs from the online critic
    pol.exp_avg.copy_(1e-3 * th.randn(pol.exp_avg.shape, generator=g))
    pol.exp_avg_sq.copy_(1e-6 * th.rand(pol.exp_avg_sq.shape, generator=g))
    pol.actor_adam_steps = pol.critic_adam_steps = 2
    pol.setup_ent_coef(learned, 0.6 if learned else 0.2)
    if learned:
        pol.ent_state[1:3] = th.tensor([1e-2, 1e-3])
        pol.ent_adam_steps = 2
    return pol.to("cuda")


def snapshot(pol):
    na = pol.actor.numel()
    h = lambda t: t.detach().cpu().numpy().copy()
    return dict(actor=h(pol._online[:na]), critic=h(pol._online[na:]), critic_t=h(pol._target), m=h(pol.exp_avg),
                v=h(pol.exp_avg_sq), ent=h(pol.ent_state), a_dims=pol.actor.stacks[0].dims, c_dims=pol.critic.stacks[0].dims,
                nc=pol.critic.n_critics, nq=pol.critic.stacks[0].numel, na=na, A=pol.actor.act_dim)


def make_eps(c, seed):
    return np.random.default_rng(seed).normal(size=(c.n_steps, 2, c.B, c.A)).astype(np.float32)


def run_update(pol, c, tabs, eps, n_steps, interval=1, idx=None):
    stats = th.full((n_steps, 4), float("nan"), device="cuda")
    if not pol.ent_learned:
        stats[:, 2] = float(pol.ent_state[3])
    argmin = i8(n_steps, 2, c.B) + 5
    idx_dev, eps_dev = dev_t(c.idx if idx is None else idx), dev_t(eps)
    pol.update(tabs[0], tabs[1], idx_dev, eps_dev, c.n_new, n_steps, c.B, GAMMA, TAU, interval, -float(c.A), LR, stats, argmin)
    return stats.cpu().numpy(), argmin.cpu().numpy()


def critic_phase(s, c, eps, alpha, dtype, step=0):
    f = lambda x: th.as_tensor(x).to(dtype)
    b, nc, nq, A = c.batch(step), s["nc"], s["nq"], s["A"]
    crit = f(s["critic"]).clone().requires_grad_()
    with th.no_grad():
        a2, lp2 = squash(stack_forward(f(s["actor"]), s["a_dims"], f(b["next_obs"]), False), th.from_numpy(eps[step, 1]), A)
        x2 = th.cat([f(b["next_obs"]), a2], dim=1)
        qt = th.cat([stack_forward(f(s["critic_t"])[i * nq:(i + 1) * nq], s["c_dims"], x2, False) for i in range(nc)], dim=1)
        mn = qt.min(dim=1, keepdim=True)
        y = f(b["reward"]).reshape(-1, 1) + (1 - f(b["done"]).reshape(-1, 1)) * GAMMA * (mn.values - alpha * lp2.reshape(-1, 1))
    x = th.cat([f(b["obs"]), f(b["action"])], dim=1)
    loss = 0.5 * sum(F.mse_loss(stack_forward(crit[i * nq:(i + 1) * nq], s["c_dims"], x, False), y) for i in range(nc))
    loss.backward()
    return float(loss.detach()), crit.grad.numpy().astype(np.float64), mn.indices.reshape(-1).numpy().astype(np.int8)


def actor_phase(s, critic_now, c, eps, alpha, dtype, step=0):
    f = lambda x: th.as_tensor(x).to(dtype)
    b, nc, nq, A = c.batch(step), s["nc"], s["nq"], s["A"]
    act = f(s["actor"]).clone().requires_grad_()
    obs = f(b["obs"])
    a, lp = squash(stack_forward(act, s["a_dims"], obs, False), th.from_numpy(eps[step, 0]), A)
    x = th.cat([obs, a], dim=1)
    q = th.cat([stack_forward(f(critic_now)[i * nq:(i + 1) * nq], s["c_dims"], x, False) for i in range(nc)], dim=1)
    mn = q.min(dim=1)
    loss = (alpha * lp - mn.values).mean()
    loss.backward()
    return (float(loss.detach()), act.grad.numpy().astype(np.float64), mn.indices.numpy().astype(np.int8),
            lp.detach().numpy().astype(np.float64))


def check_adam(tag, p0, grad, m0, v0, got, t_done=2):
    want = torch_adam(p0, grad, m0, v0, t_done, th.float64)
    t32 = torch_adam(p0.copy(), grad, m0, v0, t_done, th.float32)   # (a float32 run steps the array it is given in place)
    for name, gv, wv, tv in zip(("params", "exp_avg", "exp_avg_sq"), got, want, t32):
        assert rel(gv, wv) <= 4 * max(rel(tv, wv), HALF_EPS), (tag, name, rel(gv, wv), rel(tv, wv))


STEP_CASES = [(D, A, B, nc, arch, learned)
              for (D, A, B), (nc, arch) in zip([(3, 1, 7), (17, 6, 64), (5, 2, 257), (17, 6, 300)],
                                               [(2, (32, 24)), (1, (48,)), (1, (32, 24)), (2, (48,))])
              for learned in (True, False)]


@pytest.mark.parametrize("D,A,B,n_critics,arch,learned", STEP_CASES)
def test_a_whole_step_against_float64_autograd(D, A, B, n_critics, arch, learned):
    for n_new in sorted({B // 2, B}):
        c = Case(D, A, B, n_new, seed=11 + n_new)
        eps = make_eps(c, seed=B)
        pol = make_policy(D, A, arch, n_critics, learned, seed=B)
        tabs = c.device_tables()
        s0 = snapshot(pol)
        na = s0["na"]
        stats, argmin = run_update(pol, c, tabs, eps, 1)
        w = pol._workspace(B)
        s1 = snapshot(pol)
        grads_c, grads_a = w["grads_c"].cpu().numpy(), w["grads_a"].cpu().numpy()
        alpha = float(stats[0, 2])
        tag = f"step D {D} A {A} B {B} critics {n_critics} arch {arch} learned {learned} n_new {n_new}"
        # the temperature: alpha as it stood, the loss from the step's log-probabilities, Adam on the scalar
        (a64, ga64, am_pi64, lp64), (a32, ga32, _, lp32) = (actor_phase(s0, s1["critic"], c, eps, alpha, t)
                                                            for t in (th.float64, th.float32))
        logp_dev = w["logp"].cpu().numpy()
        assert rel(logp_dev, lp64) <= 4 * max(rel(lp32, lp64), HALF_EPS)
        if learned:
            lec0 = float(s0["ent"][0])
            assert alpha == float(s1["ent"][3]) and abs(alpha - np.exp(lec0)) <= 4 * HALF_EPS * alpha
            term = lp64 - float(A)
            l64 = float(-(lec0 * term).mean())
            l32 = float(-(np.float32(lec0) * (lp32.astype(np.float32) - np.float32(A))).mean())
            assert abs(stats[0, 3] - l64) <= 4 * max(abs(l32 - l64), HALF_EPS * abs(l64)), ("ent_coef_loss", stats[0, 3], l64)
            grad = np.array([np.float32(-(logp_dev.astype(np.float64) - float(A)).mean())])
            want = torch_adam(s0["ent"][:1], grad, s0["ent"][1:2], s0["ent"][2:3], 2, th.float64)
            t32 = torch_adam(s0["ent"][:1].copy(), grad, s0["ent"][1:2], s0["ent"][2:3], 2, th.float32)
            for gv, wv, tv in zip(s1["ent"][:3], want, t32):
                assert abs(gv - wv[0]) <= 4 * max(abs(tv[0] - wv[0]), HALF_EPS * abs(wv[0])), ("alpha adam", gv, wv, tv)
            assert s1["ent"][0] != s0["ent"][0]
        else:
            assert np.array_equal(s0["ent"], s1["ent"]) and alpha == float(np.float32(0.2)) and np.isnan(stats[0, 3])
        # critic half
        (l64, g64, am_t64), (l32, g32, _) = (critic_phase(s0, c, eps, alpha, t) for t in (th.float64, th.float32))
        assert np.array_equal(argmin[0, 0], am_t64) and np.array_equal(argmin[0, 1], am_pi64)
        dev = max(abs(l32 - l64) / abs(l64), rel(g32, g64), HALF_EPS)
        got = (abs(stats[0, 0] - l64) / abs(l64), rel(grads_c, g64))
        print(f"{tag}: critic torch32 {dev:.3e} device {got}")
        assert max(got) <= 4 * dev, ("critic", got, dev)
        check_adam("critic adam", s0["critic"], grads_c, s0["m"][na:], s0["v"][na:], (s1["critic"], s1["m"][na:], s1["v"][na:]))
        # actor half, from the device's own updated critic
        dev = max(abs(a32 - a64) / abs(a64), rel(ga32, ga64), HALF_EPS)
        got = (abs(stats[0, 1] - a64) / abs(a64), rel(grads_a, ga64))
        print(f"    actor torch32 {dev:.3e} device {got}")
        assert max(got) <= 4 * dev, ("actor", got, dev)
        check_adam("actor adam", s0["actor"], grads_a, s0["m"][:na], s0["v"][:na], (s1["actor"], s1["m"][:na], s1["v"][:na]))
        # the critic target, from the device's own updated critic
        on, t0 = s1["critic"].astype(np.float64), s0["critic_t"].astype(np.float64)
        w64 = t0 * (1 - TAU) + TAU * on
        w32 = (th.from_numpy(s0["critic_t"]) * (1 - TAU) + TAU * th.from_numpy(s1["critic"])).numpy()
        assert rel(s1["critic_t"], w64) <= 4 * max(rel(w32, w64), HALF_EPS)
        assert not np.array_equal(s1["critic_t"], s0["critic_t"])
        assert (pol.actor_adam_steps, pol.critic_adam_steps, pol.ent_adam_steps) == (3, 3, 3 if learned else 0)


def test_target_update_interval_two_leaves_the_target_untouched_in_the_second_step():
    c = Case(5, 2, 7, 3, seed=2, n_steps=2)
    eps = make_eps(c, seed=3)
    tabs = c.device_tables()
    two = make_policy(5, 2, (32, 24), 2, True, seed=4)
    t0 = two._target.clone()
    run_update(two, c, tabs, eps, 2, interval=2)
    one = make_policy(5, 2, (32, 24), 2, True, seed=4)
    run_update(one, c, tabs, eps[:1], 1, interval=2, idx=c.idx[:1])
    online_after_one = one._online.clone()
    assert th.equal(two._target, one._target) and not th.equal(two._target, t0)   # step 0 updated it, step 1 did not
    assert not th.equal(two._online, online_after_one)                             # while step 1 did move the online nets
    every = make_policy(5, 2, (32, 24), 2, True, seed=4)
    run_update(every, c, tabs, eps, 2, interval=1)
    assert th.equal(every._online, two._online) and not th.equal(every._target, two._target)


@pytest.mark.parametrize("D,A,B,n_critics,arch,learned", [(3, 1, 7, 2, (32, 24), True), (17, 6, 64, 1, (48,), False)])
def test_one_step_calls_equal_one_call_of_n_steps_bit_for_bit(D, A, B, n_critics, arch, learned):
    n = 3
    c = Case(D, A, B, B // 2, seed=5, n_steps=n)
    eps = make_eps(c, seed=6)
    tabs = c.device_tables()
    one = make_policy(D, A, arch, n_critics, learned, seed=1)
    stats_one, am_one = run_update(one, c, tabs, eps, n)
    again = make_policy(D, A, arch, n_critics, learned, seed=1)
    stats_again, am_again = run_update(again, c, tabs, eps, n)
    many = make_policy(D, A, arch, n_critics, learned, seed=1)
    parts = [run_update(many, c, tabs, eps[s:s + 1], 1, idx=c.idx[s:s + 1]) for s in range(n)]
    assert np.array_equal(stats_one, np.concatenate([x[0] for x in parts]), equal_nan=True)
    assert np.array_equal(stats_one, stats_again, equal_nan=True)
    assert np.array_equal(am_one, np.concatenate([x[1] for x in parts])) and np.array_equal(am_one, am_again)
    assert np.isfinite(stats_one[:, :3]).all() and np.isnan(stats_one[:, 3]).all() == (not learned)
    for a, b in ((one, many), (one, again)):
        for k in ("_online", "_target", "exp_avg", "exp_avg_sq", "ent_state"):
            assert th.equal(getattr(a, k), getattr(b, k)), k
