"""The DQN kernels of csrc/dqn.hip against torch float64 autograd on the CPU of exactly the step they compute, from the
same float32 inputs.

Tolerances. A step has three outputs here (loss, gradient norm, clipped gradient); its "deviation" is the largest of their
relative deviations (|x32 - x64| / |x64| for the scalars, relative L2 for the gradient) between torch's float32 CPU
evaluation and the float64 one, computed per case; the device is allowed 4 x that on each output. One scale per step
rather than per output because a single float32 scalar can land on its float64 value by chance, which says nothing about
the arithmetic; the sums are at most 256 rows and 64 columns long, so order effects live on the same scale. Parameters
and Adam moments are compared against a float64 Adam applied to the kernel's OWN clipped gradient (Adam divides by
|g| + eps, so near-zero gradients amplify gradient errors: this isolates the optimiser), within 4 x the deviation of
torch's own float32 Adam from the float64 one on that gradient. The fused update against the general path: twice the
step tolerance (two float32 implementations each within a tolerance of float64 differ by at most twice it).

`ia_dqn_update` exposes no Q-values, so `ia_dqn_q_values` (the same forward code) is held to float64 directly.

The grid crosses H, (D, A) and the batch size; row source, dones, parameter scale, target and clip threshold cycle over
the eight batch sizes (every value of each is asserted to occur for every (H, D, A)); they are not fully crossed.
"""
import ctypes as C

import numpy as np
import pytest
import torch as th
from torch.nn import functional as F

import imitation_amd as p
from imitation_amd import _lib as L
from imitation_amd import dqn

pytestmark = pytest.mark.gpu

GAP_MARGIN = 1e-3
GAMMA, LR = 0.99, 1e-3
SHAPES = [(1, 2), (3, 3), (4, 2), (17, 5), (64, 16)]
BATCHES = [1, 2, 7, 16, 17, 32, 33, 256]
N_RING, N_EXP = 40, 24


def n_params(D, H, A):
    return H * D + H + H * H + H + A * H + A


def split(flat, D, H, A):
    out, off = [], 0
    for shape in ((H, D), (H,), (H, H), (H,), (A, H), (A,)):
        n = int(np.prod(shape))
        out.append(flat[off:off + n].reshape(shape))
        off += n
    return out


def forward(ps, x):
    W1, b1, W2, b2, W3, b3 = ps
    return F.linear(F.relu(F.linear(F.relu(F.linear(x, W1, b1)), W2, b2)), W3, b3)


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


class Case:
    """One update problem: parameters, tables, indices. `source`: 0 ring only, 1 expert only, 2 mixed; `dones`: 0 none,
    1 all, 2 mixed; `scale` multiplies the parameters (|delta| on both sides of 1 needs Q-values beyond the rewards)."""

    def __init__(self, H, D, A, B, seed, source=2, dones=2, scale=1.0, target_equal=False, n_steps=1):
        g = np.random.default_rng(seed)
        self.H, self.D, self.A, self.B, self.n_steps = H, D, A, B, n_steps
        self.dones, self.target_equal = dones, target_equal
        pieces = []
        for shape, fan in (((H, D), D), ((H,), D), ((H, H), H), ((H,), H), ((A, H), H), ((A,), H)):
            pieces.append(g.uniform(-1, 1, size=shape).reshape(-1) / np.sqrt(fan))
        self.params = (np.concatenate(pieces) * scale).astype(np.float32)
        self.tparams = self.params.copy() if target_equal else \
            (self.params + 0.1 * scale * g.normal(size=self.params.shape) / np.sqrt(H)).astype(np.float32)
        P = len(self.params)
        self.m = (1e-3 * g.normal(size=P)).astype(np.float32)
        self.v = (1e-6 * g.uniform(size=P)).astype(np.float32)
        self.adam_steps = 2
        self.tables = []
        for n, reward in ((N_RING, 0.0), (N_EXP, 1.0)):
            d = {0: np.zeros(n), 1: np.ones(n), 2: (g.uniform(size=n) < 0.4)}[dones].astype(np.float32)
            self.tables.append(dict(obs=g.normal(size=(n, D)).astype(np.float32),
                                    next_obs=g.normal(size=(n, D)).astype(np.float32),
                                    action=g.integers(0, A, size=n).astype(np.int64),
                                    reward=np.full(n, reward, np.float32), done=d))
        self.n_new = {0: B, 1: 0, 2: B // 2}[source]
        self.idx = np.concatenate([g.integers(0, N_RING, size=(n_steps, self.n_new)),
                                   g.integers(0, N_EXP, size=(n_steps, B - self.n_new))], axis=1).astype(np.int64)

    def batch(self, step=0):
        i = self.idx[step]
        r, e = self.tables
        return {k: np.concatenate([r[k][i[:self.n_new]], e[k][i[self.n_new:]]]) for k in r}

    def policy(self):
        """A `DQNPolicy` on the device holding this state, and the two device tables."""
        pol = p.DQNPolicy(p.Box(-np.inf, np.inf, (self.D,)), p.Discrete(self.A), lambda _: LR,
                          net_arch=[self.H, self.H]).to("cuda")
        pol.q_net._flat.copy_(th.from_numpy(self.params))
        pol.q_net_target._flat.copy_(th.from_numpy(self.tparams))
        pol.exp_avg.copy_(th.from_numpy(self.m))
        pol.exp_avg_sq.copy_(th.from_numpy(self.v))
        pol.adam_steps = self.adam_steps
        tabs = []
        for t in self.tables:
            tab = dqn._Table(len(t["obs"]), self.D, "cuda")
            tab.write(0, t["obs"], t["next_obs"], t["action"], t["reward"], t["done"])
            tabs.append(tab)
        return pol, tabs


def ref_step(c, dtype, max_norm, params=None, step=0):
    """torch autograd of one gradient step in `dtype`: loss, gradient norm, clipped flat gradient, |delta|."""
    b = c.batch(step)
    f = lambda x: th.as_tensor(x).to(dtype)
    ps = [t.clone().requires_grad_() for t in split(f(c.params if params is None else params), c.D, c.H, c.A)]
    with th.no_grad():
        nq = forward(split(f(c.tparams), c.D, c.H, c.A), f(b["next_obs"])).max(dim=1).values.reshape(-1, 1)
        target = f(b["reward"]).reshape(-1, 1) + (1 - f(b["done"]).reshape(-1, 1)) * GAMMA * nq
    cur = th.gather(forward(ps, f(b["obs"])), dim=1, index=th.as_tensor(b["action"]).reshape(-1, 1))
    loss = F.smooth_l1_loss(cur, target)
    loss.backward()
    norm = th.nn.utils.clip_grad_norm_(ps, max_norm)
    grad = th.cat([q.grad.reshape(-1) for q in ps])
    return float(loss.detach()), float(norm), grad.numpy().astype(np.float64), (cur - target).detach().abs().reshape(-1).numpy()


def torch_adam(params, grad, m, v, t_done, dtype):
    """torch.optim.Adam's own step number t_done + 1 in `dtype` on the given state."""
    q = th.nn.Parameter(th.as_tensor(params).to(dtype))
    opt = th.optim.Adam([q], lr=LR)
    opt.state[q] = dict(step=th.tensor(float(t_done)), exp_avg=th.as_tensor(m).to(dtype).clone(),
                        exp_avg_sq=th.as_tensor(v).to(dtype).clone())
    q.grad = th.as_tensor(grad).to(dtype)
    opt.step()
    st = opt.state[q]
    return [x.detach().numpy().astype(np.float64) for x in (q, st["exp_avg"], st["exp_avg_sq"])]


def run(c, path, max_norm, n_steps=None, pol_tabs=None, idx=None):
    """`n_steps` steps of `path` ("fused" / "general") from the case's state: (stats, grad_out, params, m, v)."""
    pol, tabs = pol_tabs or c.policy()
    n_steps = n_steps or c.n_steps
    idx_dev = th.from_numpy(c.idx[:n_steps] if idx is None else idx).to("cuda")
    stats = th.full((n_steps, 2), np.nan, device="cuda")
    grad = th.full((len(c.params),), np.nan, device="cuda")
    fn = pol.update_fused if path == "fused" else pol.update_general
    fn(tabs[0], tabs[1], idx_dev, c.n_new, n_steps, c.B, GAMMA, max_norm, LR, stats, grad)
    th.cuda.synchronize()
    return [x.cpu().numpy() for x in (stats, grad, pol.q_net._flat, pol.exp_avg, pol.exp_avg_sq)]


def case_grid(H, D, A):
    """Every batch size, the other factors cycling so that each value meets each (H, D, A) several times."""
    for i, B in enumerate(BATCHES):
        k = i + H // 32 + D
        yield Case(H, D, A, B, seed=1000 * H + 10 * D + i, source=k % 3, dones=(k // 3 + i) % 3, scale=(1.0, 6.0)[i % 2],
                   target_equal=bool((i // 2) % 2)), (10.0, 0.05)[(i // 2 + D) % 2]


@pytest.mark.parametrize("D,A", SHAPES)
@pytest.mark.parametrize("H", [32, 64])
def test_fused_update_matches_float64_autograd(H, D, A):
    seen_small = seen_large = seen_clip = seen_noclip = False
    seen_source, seen_dones, seen_target = set(), set(), set()
    for c, max_norm in case_grid(H, D, A):
        seen_source.add("ring" if c.n_new == c.B else "expert" if c.n_new == 0 else "mixed")
        seen_dones.add(c.dones)
        seen_target.add(c.target_equal)
        l64, n64, g64, td = ref_step(c, th.float64, max_norm)
        l32, n32, g32, _ = ref_step(c, th.float32, max_norm)
        dev = max(abs(l32 - l64) / abs(l64), abs(n32 - n64) / abs(n64), rel(g32, g64))
        stats, grad, params, m, v = run(c, "fused", max_norm)
        got = (abs(stats[0, 0] - l64) / abs(l64), abs(stats[0, 1] - n64) / abs(n64), rel(grad, g64))
        print(f"H={H} D={D} A={A} B={c.B} n_new={c.n_new} max_norm={max_norm}: float32 deviation {dev:.3e}, "
              f"device loss / norm / grad {got[0]:.3e} {got[1]:.3e} {got[2]:.3e}")
        assert max(got) <= 4 * dev, (c.B, got, dev)
        seen_small |= bool((td < 1).any())
        seen_large |= bool((td >= 1).any())
        seen_clip |= n64 > max_norm
        seen_noclip |= n64 <= max_norm
        # Adam on the kernel's own gradient
        want = torch_adam(c.params, grad, c.m, c.v, c.adam_steps, th.float64)
        t32 = torch_adam(c.params, grad, c.m, c.v, c.adam_steps, th.float32)
        for name, w, t, g in zip(("params", "exp_avg", "exp_avg_sq"), want, t32, (params, m, v)):
            print(f"    {name}: float32 Adam deviation {rel(t, w):.3e}, device {rel(g, w):.3e}")
            assert rel(g, w) <= 4 * rel(t, w), (c.B, name, rel(g, w), rel(t, w))
    assert seen_small and seen_large and seen_clip and seen_noclip
    assert seen_source == {"ring", "expert", "mixed"} and seen_dones == {0, 1, 2} and seen_target == {False, True}


@pytest.mark.parametrize("H,D,A,B", [(64, 4, 2, 32), (32, 17, 5, 17), (64, 64, 16, 33)])
def test_steps_in_one_launch_equal_one_step_launches_bit_for_bit(H, D, A, B):
    c = Case(H, D, A, B, seed=7, n_steps=3)
    one = run(c, "fused", 0.05, n_steps=3)
    again = run(c, "fused", 0.05, n_steps=3)
    for x, y in zip(one, again):
        assert np.array_equal(x, y)
    pt = c.policy()
    stats = []
    for s in range(3):
        out = run(c, "fused", 0.05, n_steps=1, pol_tabs=pt, idx=c.idx[s:s + 1])
        stats.append(out[0])
    assert pt[0].adam_steps == c.adam_steps + 3
    assert np.array_equal(np.concatenate(stats), one[0])
    for x, y in zip(out[1:], one[1:]):
        assert np.array_equal(x, y)
    # and the three steps are the three steps: step 2's loss against float64 from the kernel's parameters after step 1
    pt = c.policy()
    run(c, "fused", 0.05, n_steps=1, pol_tabs=pt, idx=c.idx[0:1])
    mid = pt[0].q_net._flat.cpu().numpy()
    l64 = ref_step(c, th.float64, 0.05, params=mid, step=1)[0]
    l32 = ref_step(c, th.float32, 0.05, params=mid, step=1)[0]
    assert abs(one[0][1, 0] - l64) / abs(l64) <= 4 * max(abs(l32 - l64) / abs(l64), np.finfo(np.float32).eps / 2)


@pytest.mark.parametrize("H,D,A,B", [(64, 4, 2, 7), (32, 3, 3, 17), (64, 64, 16, 1), (32, 17, 5, 33)])
def test_rows_past_the_batch_change_nothing(H, D, A, B):
    """The last 16-row group is padded: poison every table row the indices do not name, and the index words behind the
    batch, and get the same bits."""
    c = Case(H, D, A, B, seed=11)
    clean = run(c, "fused", 10.0)
    pol, tabs = c.policy()
    for tab, used in ((tabs[0], c.idx[0, :c.n_new]), (tabs[1], c.idx[0, c.n_new:])):
        mask = th.ones(tab.rows, dtype=th.bool)
        mask[th.from_numpy(np.unique(used))] = False
        mask = mask.to("cuda")
        tab.obs[mask], tab.next_obs[mask], tab.reward[mask], tab.done[mask] = np.nan, np.nan, np.nan, np.nan
    poison_row = int(np.setdiff1d(np.arange(N_EXP), c.idx[0, c.n_new:])[0]) if c.n_new < B else 0
    padded = th.from_numpy(np.concatenate([c.idx[0], np.full(32, poison_row, np.int64)])).to("cuda")
    stats = th.full((1, 2), np.nan, device="cuda")
    grad = th.full((len(c.params),), np.nan, device="cuda")
    pol.update_fused(tabs[0], tabs[1], padded, c.n_new, 1, B, GAMMA, 10.0, LR, stats, grad)
    th.cuda.synchronize()
    got = [x.cpu().numpy() for x in (stats, grad, pol.q_net._flat, pol.exp_avg, pol.exp_avg_sq)]
    for x, y in zip(got, clean):
        assert np.isfinite(x).all() and np.array_equal(x, y)


@pytest.mark.parametrize("D,A", SHAPES)
@pytest.mark.parametrize("H", [32, 64])
def test_fused_update_matches_the_general_path(H, D, A):
    for c, max_norm in case_grid(H, D, A):
        if c.B not in (1, 7, 17, 32, 256):
            continue
        l64, n64, g64, _ = ref_step(c, th.float64, max_norm)
        l32, n32, g32, _ = ref_step(c, th.float32, max_norm)
        dev = max(abs(l32 - l64) / abs(l64), abs(n32 - n64) / abs(n64), rel(g32, g64))
        a, b = run(c, "fused", max_norm), run(c, "general", max_norm)
        got = (abs(a[0][0, 0] - b[0][0, 0]) / abs(l64), abs(a[0][0, 1] - b[0][0, 1]) / abs(n64), rel(a[1], b[1]))
        print(f"H={H} D={D} A={A} B={c.B}: float32 deviation {dev:.3e}, fused vs general loss / norm / grad "
              f"{got[0]:.3e} {got[1]:.3e} {got[2]:.3e}")
        assert max(got) <= 2 * 4 * dev, (c.B, got, dev)
        # the general path on its own against float64, and its Adam (`ia_dqn_adam_step`) on its own gradient
        gb = (abs(b[0][0, 0] - l64) / abs(l64), abs(b[0][0, 1] - n64) / abs(n64), rel(b[1], g64))
        assert max(gb) <= 4 * dev, (c.B, gb, dev)
        want = torch_adam(c.params, b[1], c.m, c.v, c.adam_steps, th.float64)
        t32 = torch_adam(c.params, b[1], c.m, c.v, c.adam_steps, th.float32)
        for name, w, t, g in zip(("params", "exp_avg", "exp_avg_sq"), want, t32, b[2:]):
            assert rel(g, w) <= 4 * rel(t, w), (c.B, name, rel(g, w), rel(t, w))


@pytest.mark.parametrize("H,D,A", [(32, 1, 2), (64, 4, 2), (32, 17, 5), (64, 64, 16)])
def test_q_values_and_first_arg_max(H, D, A):
    c = Case(H, D, A, 1, seed=3, scale=2.0)
    pol, _ = c.policy()
    g = np.random.default_rng(5)
    cand = g.normal(size=(4096, D)).astype(np.float32)
    ps64 = split(th.as_tensor(c.params).double(), D, H, A)
    q64 = forward(ps64, th.as_tensor(cand).double()).numpy()
    top = np.sort(q64, axis=1)
    obs_all = cand[(top[:, -1] - top[:, -2]) > GAP_MARGIN][:1024]   # inputs drawn so that every row qualifies
    assert len(obs_all) == 1024
    q64 = forward(ps64, th.as_tensor(obs_all).double()).numpy()
    q32 = forward(split(th.as_tensor(c.params), D, H, A), th.as_tensor(obs_all)).numpy()
    full = None
    for n in (1024, 1, 63, 64, 65):
        obs = th.from_numpy(obs_all[:n]).to("cuda")
        q, am = pol.q_net.q_values(obs)
        th.cuda.synchronize()
        q, am = q.cpu().numpy(), am.cpu().numpy()
        top = np.sort(q64[:n], axis=1)
        assert ((top[:, -1] - top[:, -2]) > GAP_MARGIN).all()
        assert am.dtype == np.int64 and np.array_equal(am, q64[:n].argmax(axis=1))
        if full is None:
            # accuracy on the 1 024 rows (one row's two to sixteen numbers say little: torch's float32 row can land on
            # the float64 one); the smaller n are then held to MORE than a tolerance: the same bits as these rows
            full = q
            dev = rel(q32, q64)
            print(f"H={H} D={D} A={A} n={n}: float32 deviation {dev:.3e}, device {rel(q, q64):.3e}")
            assert rel(q, q64) <= 4 * dev
        assert np.array_equal(q, full[:n])   # a row's result does not depend on the other rows or on n
    # ties go to the first maximum
    pol.q_net._flat.zero_()
    q, am = pol.q_net.q_values(th.from_numpy(obs_all[:5]).to("cuda"))
    assert am.cpu().tolist() == [0] * 5 and float(q.abs().max()) == 0.0


@pytest.mark.parametrize("B,A", [(1, 2), (7, 3), (256, 16), (300, 5)])
def test_td_loss_matches_float64(B, A):
    g = np.random.default_rng(B)
    q = (2 * g.normal(size=(B, A))).astype(np.float32)
    qt = (2 * g.normal(size=(B, A))).astype(np.float32)
    act = g.integers(0, A, size=B).astype(np.int64)
    rew = (g.uniform(size=B) < 0.5).astype(np.float32)
    done = (g.uniform(size=B) < 0.4).astype(np.float32)

    def ref(dtype):
        f = lambda x: th.as_tensor(x).to(dtype)
        qq = f(q).requires_grad_()
        target = f(rew) + (1 - f(done)) * GAMMA * f(qt).max(dim=1).values
        cur = th.gather(qq, 1, th.as_tensor(act).reshape(-1, 1)).reshape(-1)
        terms = F.smooth_l1_loss(cur, target, reduction="none")
        loss = F.smooth_l1_loss(cur, target)
        loss.backward()
        return float(loss.detach()), terms.detach().numpy().astype(np.float64), qq.grad.numpy().astype(np.float64), \
            (cur - target).detach().abs().numpy()

    l64, t64, d64, td = ref(th.float64)
    l32, t32, d32, _ = ref(th.float32)
    if B > 1:
        assert (td < 1).any() and (td >= 1).any()
    dev = max(abs(l32 - l64) / abs(l64), rel(t32, t64), rel(d32, d64))
    ins = [th.from_numpy(x).to("cuda") for x in (q, qt, act, rew, done)]   # (kept alive across the launch)
    dq, terms, loss = th.full((B, A), np.nan, device="cuda"), th.full((B,), np.nan, device="cuda"), th.zeros(1, device="cuda")
    L.call("ia_dqn_td_loss", *[L.ptr(x) for x in ins], B, A, GAMMA, L.ptr(dq), L.ptr(terms), L.ptr(loss), L.stream())
    th.cuda.synchronize()
    got = (abs(float(loss) - l64) / abs(l64), rel(terms.cpu().numpy(), t64), rel(dq.cpu().numpy(), d64))
    print(f"B={B} A={A}: float32 deviation {dev:.3e}, device loss / terms / dQ {got[0]:.3e} {got[1]:.3e} {got[2]:.3e}")
    assert max(got) <= 4 * max(dev, np.finfo(np.float32).eps / 2)
    assert np.array_equal(dq.cpu().numpy() != 0, (d64 != 0))   # non-zero in the taken action's column only


@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_polyak_update_is_the_float32_expression(tau):
    g = np.random.default_rng(0)
    n = 9360 + 7
    online, target = g.normal(size=n).astype(np.float32), g.normal(size=n).astype(np.float32)
    o, t = th.from_numpy(online).to("cuda"), th.from_numpy(target).to("cuda")
    L.call("ia_polyak_update", L.ptr(o), L.ptr(t), n, tau, L.stream())
    th.cuda.synchronize()
    want = online if tau == 1.0 else np.float32(tau) * online + (np.float32(1) - np.float32(tau)) * target
    assert want.dtype == np.float32 and np.array_equal(t.cpu().numpy(), want) and np.array_equal(o.cpu().numpy(), online)


def test_shapes_outside_the_fused_kernel_are_refused():
    lib = L.load()
    assert lib.ia_dqn_update_ok(64, 64, 16, 256) == 1 and lib.ia_dqn_update_ok(1, 32, 1, 1) == 1
    bad = [(65, 64, 2, 32), (4, 48, 2, 32), (4, 64, 17, 32), (4, 64, 2, 257), (0, 64, 2, 32), (4, 64, 2, 0)]
    c = Case(64, 4, 2, 8, seed=0)
    pol, tabs = c.policy()
    before = pol.q_net._flat.clone()
    idx = th.zeros(300, dtype=th.int64, device="cuda")
    stats = th.zeros(2, device="cuda")
    scal = (C.c_float * 2)(1e-3, 1.0)
    for D, H, A, B in bad:
        assert lib.ia_dqn_update_ok(D, H, A, B) == 0
        rc = lib.ia_dqn_update(D, H, A, B, 0, 1, L.ptr(pol.q_net._flat), L.ptr(pol.q_net_target._flat), L.ptr(pol.exp_avg),
                               L.ptr(pol.exp_avg_sq), None, None, None, None, None, L.ptr(tabs[1].obs),
                               L.ptr(tabs[1].next_obs), L.ptr(tabs[1].action), L.ptr(tabs[1].reward), L.ptr(tabs[1].done),
                               L.ptr(idx), GAMMA, 10.0, 0.9, 0.999, 1e-8, C.addressof(scal), L.ptr(stats), None, L.stream())
        assert rc == L.ERR_UNSUPPORTED, (D, H, A, B, rc)
    q = th.zeros(4, 2, device="cuda")
    am = th.zeros(4, dtype=th.int64, device="cuda")
    obs = th.zeros(4, 70, device="cuda")
    for D, H, A in ((65, 64, 2), (4, 48, 2), (4, 64, 17)):
        assert lib.ia_dqn_q_values(D, H, A, L.ptr(pol.q_net._flat), L.ptr(obs), 4, L.ptr(q), L.ptr(am),
                                   L.stream()) == L.ERR_UNSUPPORTED
    th.cuda.synchronize()
    assert th.equal(pol.q_net._flat, before)
    # the policy routes such shapes to the general path instead of failing
    wide = p.DQNPolicy(p.Box(-1, 1, (4,)), p.Discrete(2), lambda _: LR, net_arch=[48]).to("cuda")
    assert not wide.fused_ok(8) and pol.fused_ok(8) and not pol.fused_ok(257)
    # ... and, by measured cost, the batches at which the one-workgroup kernel loses to the general path's launches
    big = p.DQNPolicy(p.Box(-1, 1, (64,)), p.Discrete(16), lambda _: LR).to("cuda")
    assert [pol.fused_ok(b) for b in (32, 64, 80, 96, 256)] == [True, True, False, False, False]
    assert [big.fused_ok(b) for b in (16, 32, 48, 256)] == [True, True, False, False]
