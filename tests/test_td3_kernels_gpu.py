"""The TD3 kernels of csrc/td3.hip and a whole general-path step (`TD3Policy.update`) against torch restatements on the CPU
from the same float32 inputs.

The kernels that move and clamp values (batch assembly, target input, actor input, the actor seed's elementwise product)
have one right answer and are compared bit for bit with the same float32 operations in torch. Sums (the losses) and
everything behind a GEMM are compared with float64: the device's deviation from float64 may be at most 4 x the deviation of
torch's own float32 evaluation, floored at half a float32 epsilon, one scale per phase of the step (the largest deviation
over the phase's outputs: a single float32 scalar can land on its float64 value by chance). Parameters after Adam are held
to a float64 Adam applied to the kernel's OWN gradient (Adam divides by |g| + eps, so near-zero gradients amplify gradient
errors), and the actor phase is restated from the device's own updated critic, for the same reason.
"""
import numpy as np
import pytest
import torch as th
from torch.nn import functional as F

import imitation_amd as p
from imitation_amd import _lib as L
from imitation_amd import dqn

pytestmark = pytest.mark.gpu

GAMMA, LR, TAU, CLIP, SIGMA = 0.99, 1e-3, 0.005, 0.5, 0.4
N_RING, N_EXP = 40, 24
SHAPES = [(3, 1), (17, 6)]
BATCHES = [1, 7, 100]
HALF_EPS = float(np.finfo(np.float32).eps) / 2


def n_new_values(B):
    return sorted({0, B // 2, B})


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def dev_t(x):
    return th.from_numpy(np.ascontiguousarray(x)).to("cuda")


class Case:
    """Tables, one index row per step, noise; `n_new` rows come from the ring."""

    def __init__(self, D, A, B, n_new, seed=0, n_steps=1):
        g = np.random.default_rng(seed)
        self.D, self.A, self.B, self.n_new, self.n_steps = D, A, B, n_new, n_steps
        self.tables = []
        for n, reward in ((N_RING, 0.0), (N_EXP, 1.0)):
            self.tables.append(dict(obs=g.normal(size=(n, D)).astype(np.float32),
                                    next_obs=g.normal(size=(n, D)).astype(np.float32),
                                    action=g.uniform(-1, 1, size=(n, A)).astype(np.float32),
                                    reward=np.full(n, reward, np.float32), done=(g.uniform(size=n) < 0.4).astype(np.float32)))
        self.idx = np.concatenate([g.integers(0, N_RING, size=(n_steps, n_new)),
                                   g.integers(0, N_EXP, size=(n_steps, B - n_new))], axis=1).astype(np.int64)
        self.noise = (SIGMA * g.normal(size=(n_steps, B, A))).astype(np.float32)

    def batch(self, step=0):
        i = self.idx[step]
        r, e = self.tables
        return {k: np.concatenate([r[k][i[:self.n_new]], e[k][i[self.n_new:]]]) for k in r}

    def device_tables(self):
        """(ring, expert); a table no row comes from is absent (None)."""
        tabs = []
        for t, used in zip(self.tables, (self.n_new > 0, self.n_new < self.B)):
            if not used:
                tabs.append(None)
                continue
            tab = dqn._Table(len(t["obs"]), self.D, "cuda", self.A)
            tab.write(0, t["obs"], t["next_obs"], t["action"], t["reward"], t["done"])
            tabs.append(tab)
        return tabs


def table_args(t):
    if t is None:
        return (None,) * 5 + (0,)
    return (L.ptr(t.obs), L.ptr(t.next_obs), L.ptr(t.action), L.ptr(t.reward), L.ptr(t.done), t.rows)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("D,A", SHAPES)
def test_batch_assembly_moves_the_rows_bit_for_bit(D, A, B, pad):
    ld = D + A + pad
    for n_new in n_new_values(B):
        c = Case(D, A, B, n_new, seed=B + n_new)
        ring, expert = c.device_tables()
        out = dict(X=th.full((B, ld), 7.0, device="cuda"), S=th.empty(B, D, device="cuda"), S2=th.empty(B, D, device="cuda"),
                   rew=th.empty(B, device="cuda"), done=th.empty(B, device="cuda"))
        idx = dev_t(c.idx[0])
        L.call("ia_td3_assemble", *table_args(ring), *table_args(expert), L.ptr(idx), B, n_new, D, A, ld,
               *(L.ptr(out[k]) for k in ("X", "S", "S2", "rew", "done")), L.stream())
        b = c.batch()
        want_x = np.concatenate([b["obs"], b["action"], np.zeros((B, pad), np.float32)], axis=1)
        for k, w in (("X", want_x), ("S", b["obs"]), ("S2", b["next_obs"]), ("rew", b["reward"]), ("done", b["done"])):
            assert np.array_equal(out[k].cpu().numpy(), w), (k, n_new)


def test_batch_assembly_refuses_a_missing_table_and_marks_a_bad_index():
    c = Case(3, 1, 7, 3)
    ring, expert = c.device_tables()
    out = [th.zeros(7, 4, device="cuda"), th.zeros(7, 3, device="cuda"), th.zeros(7, 3, device="cuda"),
           th.zeros(7, device="cuda"), th.zeros(7, device="cuda")]
    args = lambda r, e, idx: (*table_args(r), *table_args(e), L.ptr(idx), 7, 3, 3, 1, 4, *(L.ptr(t) for t in out), L.stream())
    idx = dev_t(c.idx[0])
    assert L.load().ia_td3_assemble(*args(None, expert, idx)) == L.ERR_ARG
    assert L.load().ia_td3_assemble(*args(ring, None, idx)) == L.ERR_ARG
    bad = c.idx[0].copy()
    bad[1], bad[5] = N_RING, -1   # one past the ring, below the expert table: NaN rows, nothing read out of bounds
    bad_dev = dev_t(bad)
    L.call("ia_td3_assemble", *args(ring, expert, bad_dev))
    x = out[0].cpu().numpy()
    assert np.isnan(x[[1, 5]]).all() and not np.isnan(np.delete(x, [1, 5], axis=0)).any()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("D,A", SHAPES)
def test_target_input_clamps_bit_for_bit(D, A, B):
    g = np.random.default_rng(B)
    s2 = g.normal(size=(B, D)).astype(np.float32)
    mu = np.tanh(1.5 * g.normal(size=(B, A))).astype(np.float32)
    noise = (SIGMA * g.normal(size=(B, A))).astype(np.float32)
    ld = D + A
    x2 = th.empty(B, ld, device="cuda")
    ins = [dev_t(s2), dev_t(mu), dev_t(noise)]   # (held: a temporary's block would be handed to the next upload)
    L.call("ia_td3_target_input", *(L.ptr(t) for t in ins), B, D, A, ld, CLIP, L.ptr(x2), L.stream())
    nz = th.from_numpy(noise).clamp(-CLIP, CLIP)
    act = (th.from_numpy(mu) + nz).clamp(-1, 1)
    want = th.cat([th.from_numpy(s2), act], dim=1).numpy()
    assert np.array_equal(x2.cpu().numpy(), want)
    if B * A >= 42:   # both clamps bind, and not everywhere
        assert 0 < (np.abs(noise) > CLIP).sum() < noise.size and 0 < (np.abs(want[:, D:]) == 1).sum() < B * A


@pytest.mark.parametrize("n_critics", [1, 2])
@pytest.mark.parametrize("B", BATCHES + [300])
def test_critic_loss_against_float64_and_repeats_bit_for_bit(B, n_critics):
    g = np.random.default_rng(B + n_critics)
    q = g.normal(size=(n_critics, B)).astype(np.float32)
    qt = g.normal(size=(n_critics, B)).astype(np.float32)
    rew = (g.uniform(size=B) < 0.5).astype(np.float32)
    done = (np.arange(B) % 3 == 0).astype(np.float32)   # both values occur from two rows on

    def ref(dtype):
        f = lambda x: th.from_numpy(x).to(dtype)
        cur = f(q).clone().requires_grad_()
        y = f(rew) + (1 - f(done)) * GAMMA * f(qt).min(dim=0).values
        loss = sum(F.mse_loss(cur[i], y) for i in range(n_critics))
        loss.backward()
        return float(loss.detach()), cur.grad.numpy(), y.numpy()

    runs = []
    ins = [dev_t(q), dev_t(qt), dev_t(rew), dev_t(done)]
    for _ in range(2):
        dq, y, loss = th.empty(n_critics, B, device="cuda"), th.empty(B, device="cuda"), th.empty(1, device="cuda")
        L.call("ia_td3_critic_loss", *(L.ptr(t) for t in ins), B, n_critics, GAMMA, L.ptr(dq), L.ptr(y), L.ptr(loss),
               L.stream())
        runs.append((float(loss.cpu()), dq.cpu().numpy(), y.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    (l64, g64, y64), (l32, g32, y32) = ref(th.float64), ref(th.float32)
    dev = max(abs(l32 - l64) / abs(l64), rel(g32, g64), rel(y32, y64), HALF_EPS)
    got = (abs(runs[0][0] - l64) / abs(l64), rel(runs[0][1], g64), rel(runs[0][2], y64))
    print(f"critic loss B {B} critics {n_critics}: torch32 {dev:.3e}, device {got}")
    assert max(got) <= 4 * dev, (got, dev)
    if B > 1:
        assert (done == 1).any() and (done == 0).any()


@pytest.mark.parametrize("B", BATCHES + [300])
@pytest.mark.parametrize("D,A", SHAPES)
def test_actor_input_and_seed(D, A, B):
    g = np.random.default_rng(B)
    ld = D + A
    x = g.normal(size=(B, ld)).astype(np.float32)
    mu = np.tanh(g.normal(size=(B, A))).astype(np.float32)
    dx = g.normal(size=(B, ld)).astype(np.float32)
    q1 = g.normal(size=B).astype(np.float32)
    xd, mud = dev_t(x), dev_t(mu)
    L.call("ia_td3_actor_input", L.ptr(mud), B, D, A, ld, L.ptr(xd), L.stream())
    assert np.array_equal(xd.cpu().numpy(), np.concatenate([x[:, :D], mu], axis=1))
    runs = []
    ins = [dev_t(q1), dev_t(dx), mud]
    for _ in range(2):
        dmu, loss = th.empty(B, A, device="cuda"), th.empty(1, device="cuda")
        L.call("ia_td3_actor_seed", *(L.ptr(t) for t in ins), B, D, A, ld, L.ptr(dmu), L.ptr(loss), L.stream())
        runs.append((float(loss.cpu()), dmu.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    inv_b = th.tensor(1.0) / th.tensor(float(B))
    m = th.from_numpy(mu)
    want = (th.from_numpy(dx[:, D:]) * -inv_b) * (1.0 - m * m)
    assert np.array_equal(runs[0][1], want.numpy())
    l64, l32 = -float(q1.astype(np.float64).mean()), -float(th.from_numpy(q1).mean())
    assert abs(runs[0][0] - l64) <= 4 * max(abs(l32 - l64), HALF_EPS * abs(l64))


# ---- a whole step ----------------------------------------------------------------------------------------------------------

def make_policy(D, A, arch, n_critics, seed):
    th.manual_seed(seed)
    pol = p.TD3Policy(p.Box(-np.inf, np.inf, (D,)), p.Box(-1, 1, (A,)), lambda _: LR, net_arch=list(arch), n_critics=n_critics)
    g = th.Generator().manual_seed(seed + 1)
    pol._target.add_(0.05 * th.randn(pol._target.shape, generator=g))   # targets that differ from the online nets
    pol.exp_avg.copy_(1e-3 * th.randn(pol.exp_avg.shape, generator=g))
    pol.exp_avg_sq.copy_(1e-6 * th.rand(pol.exp_avg_sq.shape, generator=g))
    pol.actor_adam_steps = pol.critic_adam_steps = 2
    return pol.to("cuda")


def stack_forward(flat, dims, x, squash):
    off = 0
    for i in range(len(dims) - 1):
        W = flat[off:off + dims[i + 1] * dims[i]].reshape(dims[i + 1], dims[i])
        off += W.numel()
        b = flat[off:off + dims[i + 1]]
        off += dims[i + 1]
        x = F.linear(x, W, b)
        if i < len(dims) - 2:
            x = F.relu(x)
    return th.tanh(x) if squash else x


def critic_phase(state, c, dtype, step=0):
    """loss, flat critic gradient of [SB3 TD3.train]'s critic half in `dtype` from the float32 state."""
    f = lambda x: th.as_tensor(x).to(dtype)
    b = c.batch(step)
    a_dims, c_dims, nc, nq = state["a_dims"], state["c_dims"], state["nc"], state["nq"]
    crit = f(state["critic"]).clone().requires_grad_()
    with th.no_grad():
        nz = f(c.noise[step]).clamp(-CLIP, CLIP)
        na = (stack_forward(f(state["actor_t"]), a_dims, f(b["next_obs"]), True) + nz).clamp(-1, 1)
        x2 = th.cat([f(b["next_obs"]), na], dim=1)
        qt = th.cat([stack_forward(f(state["critic_t"])[i * nq:(i + 1) * nq], c_dims, x2, False) for i in range(nc)], dim=1)
        y = f(b["reward"]).reshape(-1, 1) + (1 - f(b["done"]).reshape(-1, 1)) * GAMMA * qt.min(dim=1, keepdim=True).values
    x = th.cat([f(b["obs"]), f(b["action"])], dim=1)
    loss = sum(F.mse_loss(stack_forward(crit[i * nq:(i + 1) * nq], c_dims, x, False), y) for i in range(nc))
    loss.backward()
    return float(loss.detach()), crit.grad.numpy().astype(np.float64)


def actor_phase(state, critic_now, c, dtype, step=0):
    f = lambda x: th.as_tensor(x).to(dtype)
    b = c.batch(step)
    act = f(state["actor"]).clone().requires_grad_()
    obs = f(b["obs"])
    q1 = stack_forward(f(critic_now)[:state["nq"]], state["c_dims"], th.cat([obs, stack_forward(act, state["a_dims"], obs, True)], 1),
                       False)
    loss = -q1.mean()
    loss.backward()
    return float(loss.detach()), act.grad.numpy().astype(np.float64)


def torch_adam(params, grad, m, v, t_done, dtype):
    q = th.nn.Parameter(th.as_tensor(params).to(dtype))
    opt = th.optim.Adam([q], lr=LR)
    opt.state[q] = dict(step=th.tensor(float(t_done)), exp_avg=th.as_tensor(m).to(dtype).clone(),
                        exp_avg_sq=th.as_tensor(v).to(dtype).clone())
    q.grad = th.as_tensor(grad).to(dtype)
    opt.step()
    st = opt.state[q]
    return [x.detach().numpy().astype(np.float64) for x in (q, st["exp_avg"], st["exp_avg_sq"])]


def snapshot(pol):
    na = pol.actor.numel()
    h = lambda t: t.detach().cpu().numpy().copy()
    return dict(actor=h(pol._online[:na]), critic=h(pol._online[na:]), actor_t=h(pol._target[:na]), critic_t=h(pol._target[na:]),
                m=h(pol.exp_avg), v=h(pol.exp_avg_sq), a_dims=pol.actor.stacks[0].dims, c_dims=pol.critic.stacks[0].dims,
                nc=pol.critic.n_critics, nq=pol.critic.stacks[0].numel, na=na)


def run_update(pol, c, tabs, n_steps, n_updates, policy_delay, idx=None, noise=None):
    stats = th.full((n_steps, 2), float("nan"), device="cuda")
    idx_dev, noise_dev = dev_t(c.idx if idx is None else idx), dev_t(c.noise if noise is None else noise)
    steps = pol.update(tabs[0], tabs[1], idx_dev, noise_dev, c.n_new, n_steps, c.B, GAMMA, TAU, policy_delay, CLIP, n_updates,
                       LR, stats)
    return stats.cpu().numpy(), steps


STEP_CASES = [(3, 1, 1, 2, (32, 24)), (3, 1, 7, 1, (32, 24)), (17, 6, 7, 2, (32, 24)), (17, 6, 100, 2, (32, 24)),
              (17, 6, 100, 1, (48,)), (3, 1, 100, 2, (400, 300))]


@pytest.mark.parametrize("D,A,B,n_critics,arch", STEP_CASES)
def test_a_whole_step_against_float64_autograd(D, A, B, n_critics, arch):
    for n_new in n_new_values(B):
        c = Case(D, A, B, n_new, seed=11 + n_new)
        pol = make_policy(D, A, arch, n_critics, seed=B)
        tabs = c.device_tables()
        s0 = snapshot(pol)
        na = s0["na"]
        stats, steps = run_update(pol, c, tabs, 1, n_updates=0, policy_delay=1)
        assert steps == [True]
        w = pol._workspace(B)
        s1 = snapshot(pol)
        grads_c, grads_a = w["grads_c"].cpu().numpy(), w["grads_a"].cpu().numpy()
        # critic half
        (l64, g64), (l32, g32) = critic_phase(s0, c, th.float64), critic_phase(s0, c, th.float32)
        dev = max(abs(l32 - l64) / abs(l64), rel(g32, g64), HALF_EPS)
        got = (abs(stats[0, 0] - l64) / abs(l64), rel(grads_c, g64))
        print(f"step D {D} A {A} B {B} critics {n_critics} arch {arch} n_new {n_new}: critic torch32 {dev:.3e} device {got}")
        assert max(got) <= 4 * dev, ("critic", got, dev)
        want = torch_adam(s0["critic"], grads_c, s0["m"][na:], s0["v"][na:], 2, th.float64)
        t32 = torch_adam(s0["critic"], grads_c, s0["m"][na:], s0["v"][na:], 2, th.float32)
        for name, gotv, wv, tv in zip(("params", "exp_avg", "exp_avg_sq"), (s1["critic"], s1["m"][na:], s1["v"][na:]), want, t32):
            assert rel(gotv, wv) <= 4 * max(rel(tv, wv), HALF_EPS), ("critic adam", name, rel(gotv, wv), rel(tv, wv))
        # actor half, from the device's own updated critic
        (a64, ga64), (a32, ga32) = actor_phase(s0, s1["critic"], c, th.float64), actor_phase(s0, s1["critic"], c, th.float32)
        dev = max(abs(a32 - a64) / abs(a64), rel(ga32, ga64), HALF_EPS)
        got = (abs(stats[0, 1] - a64) / abs(a64), rel(grads_a, ga64))
        print(f"    actor torch32 {dev:.3e} device {got}")
        assert max(got) <= 4 * dev, ("actor", got, dev)
        want = torch_adam(s0["actor"], grads_a, s0["m"][:na], s0["v"][:na], 2, th.float64)
        t32 = torch_adam(s0["actor"], grads_a, s0["m"][:na], s0["v"][:na], 2, th.float32)
        for name, gotv, wv, tv in zip(("params", "exp_avg", "exp_avg_sq"), (s1["actor"], s1["m"][:na], s1["v"][:na]), want, t32):
            assert rel(gotv, wv) <= 4 * max(rel(tv, wv), HALF_EPS), ("actor adam", name, rel(gotv, wv), rel(tv, wv))
        # both target updates, from the device's own updated online nets
        for k in ("actor", "critic"):
            on, t0 = s1[k].astype(np.float64), s0[k + "_t"].astype(np.float64)
            w64 = t0 * (1 - TAU) + TAU * on
            w32 = (th.from_numpy(s0[k + "_t"]) * (1 - TAU) + TAU * th.from_numpy(s1[k])).numpy()
            assert rel(s1[k + "_t"], w64) <= 4 * max(rel(w32, w64), HALF_EPS), k
            assert not np.array_equal(s1[k + "_t"], s0[k + "_t"])


def test_a_delayed_step_leaves_actor_and_targets_alone():
    c = Case(3, 1, 7, 3)
    pol = make_policy(3, 1, (32, 24), 2, seed=3)
    s0 = snapshot(pol)
    stats, steps = run_update(pol, c, c.device_tables(), 1, n_updates=0, policy_delay=2)
    s1 = snapshot(pol)
    assert steps == [False] and np.isnan(stats[0, 1]) and np.isfinite(stats[0, 0])
    for k in ("actor", "actor_t", "critic_t"):
        assert np.array_equal(s0[k], s1[k]), k
    assert not np.array_equal(s0["critic"], s1["critic"]) and (pol.actor_adam_steps, pol.critic_adam_steps) == (2, 3)


@pytest.mark.parametrize("D,A,B,n_critics,arch", [(3, 1, 7, 2, (32, 24)), (17, 6, 100, 1, (48,))])
def test_one_step_calls_equal_one_call_of_n_steps_bit_for_bit(D, A, B, n_critics, arch):
    n = 3
    c = Case(D, A, B, B // 2, seed=5, n_steps=n)
    tabs = c.device_tables()
    one = make_policy(D, A, arch, n_critics, seed=1)
    stats_one, steps_one = run_update(one, c, tabs, n, n_updates=4, policy_delay=2)
    again = make_policy(D, A, arch, n_critics, seed=1)
    stats_again, _ = run_update(again, c, tabs, n, n_updates=4, policy_delay=2)
    many = make_policy(D, A, arch, n_critics, seed=1)
    stats_many, steps_many = [], []
    for s in range(n):
        st, up = run_update(many, c, tabs, 1, n_updates=4 + s, policy_delay=2, idx=c.idx[s:s + 1], noise=c.noise[s:s + 1])
        stats_many.append(st)
        steps_many += up
    assert steps_one == steps_many == [False, True, False]
    assert np.array_equal(stats_one, np.concatenate(stats_many), equal_nan=True)
    assert np.array_equal(stats_one, stats_again, equal_nan=True)
    for a, b in ((one, many), (one, again)):
        for k in ("_online", "_target", "exp_avg", "exp_avg_sq"):
            assert th.equal(getattr(a, k), getattr(b, k)), k
