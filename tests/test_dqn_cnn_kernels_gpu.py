"""Kernel level of DQN's `CnnPolicy`: `ia_dqn_assemble_u8` against NumPy fancy indexing, bit for bit; one gradient step
through `DQNPolicy.update_frames` against the float64 torch restatement (`tests/dqn_cnn_ref.py`) with the restatement's own
float32 run as the yardstick (the device may deviate from float64 by 8 x what float32 torch does, per tensor -- the margin
of `tests/test_sqil_gpu.py`); determinism; acting."""
import copy

import numpy as np
import pytest
import torch as th
from torch.nn import functional as F

import imitation_amd as p
from imitation_amd import _lib as L
from imitation_amd import dqn, spaces
from tests import dqn_cnn_ref

pytestmark = pytest.mark.gpu

GAMMA, LR = 0.99, 1e-3


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- ia_dqn_assemble_u8 -------------------------------------------------------------------------------------------------
def frame_table(rows, fb, rng, device="cuda"):
    t = dqn._Table(rows, fb, device, frames=True)
    host = dict(obs=rng.integers(0, 256, size=(rows, fb), dtype=np.uint8),
                next_obs=rng.integers(0, 256, size=(rows, fb), dtype=np.uint8),
                action=rng.integers(-2 ** 40, 2 ** 40, size=rows), reward=rng.normal(size=rows).astype(np.float32),
                done=(rng.uniform(size=rows) < 0.5).astype(np.float32))
    t.write(0, host["obs"], host["next_obs"], host["action"], host["reward"], host["done"])
    return t, host


def segment(m, rows, rng, edge):
    """`m` in-range rows of a table: row 0, the last row and a repeat wherever `m` has room for them."""
    idx = rng.integers(0, rows, size=m)
    if m == 1:
        idx[0] = (0, rows - 1)[edge]
    if m >= 2:
        idx[0], idx[m - 1] = 0, rows - 1
    if m >= 3:
        idx[1] = idx[2 % m] if m > 3 else 0
    return idx


def assemble(ring, expert, idx_dev, B, n_new, fb):
    n = max(B, 1)   # (the argument-contract test passes B <= 0)
    out = dict(obs=th.full((n, fb), 171, dtype=th.uint8, device="cuda"), nxt=th.full((n, fb), 171, dtype=th.uint8, device="cuda"),
               act=th.full((n,), -7, dtype=th.int64, device="cuda"), rew=th.full((n,), np.nan, device="cuda"),
               done=th.full((n,), np.nan, device="cuda"))
    tab = lambda t: ([None] * 5 + [0]) if t is None else [L.ptr(t.obs), L.ptr(t.next_obs), L.ptr(t.action), L.ptr(t.reward),
                                                          L.ptr(t.done), t.rows]
    rc = L.load().ia_dqn_assemble_u8(*tab(ring), *tab(expert), L.ptr(idx_dev), B, n_new, fb, L.ptr(out["obs"]),
                                     L.ptr(out["nxt"]), L.ptr(out["act"]), L.ptr(out["rew"]), L.ptr(out["done"]), L.stream())
    return rc, out


@pytest.mark.parametrize("B", [1, 7, 256])
@pytest.mark.parametrize("fb", [1, 16, 4551, 5184])
def test_assemble_matches_numpy_fancy_indexing(fb, B):
    rng = np.random.default_rng(1000 * fb + B)
    for rows in (3, 300):
        ring, ring_h = frame_table(rows, fb, rng)
        expert, expert_h = frame_table(rows + 1, fb, rng)   # (another row count: an index of the wrong table would show)
        for n_new in sorted({0, B // 2, B}):
            for edge in (0, 1):
                idx = np.concatenate([segment(n_new, rows, rng, edge), segment(B - n_new, rows + 1, rng, edge)]).astype(np.int64)
                assert idx[:n_new].max(initial=0) < rows and idx[n_new:].max(initial=0) < rows + 1 and idx.min() >= 0
                rc, out = assemble(ring if n_new > 0 else None, expert if n_new < B else None,
                                   th.from_numpy(idx).cuda(), B, n_new, fb)
                assert rc == 0
                for key, name in (("obs", "obs"), ("nxt", "next_obs"), ("act", "action"), ("rew", "reward"), ("done", "done")):
                    want = np.concatenate([ring_h[name][idx[:n_new]], expert_h[name][idx[n_new:]]])
                    got = out[key].cpu().numpy()
                    assert got.dtype == want.dtype and np.array_equal(got, want), (key, rows, n_new, edge)


def test_assemble_argument_contract():
    """Each violated precondition returns IA_ERR_ARG before anything is launched: the outputs keep their fill."""
    rng = np.random.default_rng(0)
    ring, _ = frame_table(3, 16, rng)
    expert, _ = frame_table(3, 16, rng)
    idx = th.zeros(4, dtype=th.int64, device="cuda")
    for r, e, B, n_new in ((ring, expert, 0, 0), (ring, expert, -1, 0), (ring, expert, 4, -1), (ring, expert, 4, 5),
                           (None, expert, 4, 2), (ring, None, 4, 2), (None, expert, 4, 4), (ring, None, 4, 0)):
        rc, out = assemble(r, e, idx, B, n_new, 16)
        assert rc == L.ERR_ARG, (B, n_new)
        th.cuda.synchronize()
        assert bool((out["obs"] == 171).all()) and bool((out["act"] == -7).all()) and bool(th.isnan(out["rew"]).all())


# ---- one gradient step against the float64 restatement --------------------------------------------------------------
STEP_CASES = {   # frames, n_actions, B, features_dim, max_grad_norm (0.5: clipping active; 10: inactive)
    "min_map_clipped": ((4, 36, 36), 3, 8, 512, 0.5),
    "wide_map_three_channels": ((3, 44, 48), 4, 7, 32, 10.0),
    "sb3_defaults": ((4, 84, 84), 6, 32, 512, 10.0),
}


class StepData:
    """One minibatch problem: a restatement policy (float32 initialisation), a learner ring and an expert table of random
    frames, an index row, rewards and dones under which both Huber branches occur."""

    def __init__(self, shape, n_actions, B, features_dim, seed=0, steps=1):
        rng = np.random.default_rng(seed)
        self.shape, self.A, self.B, self.fdim = shape, n_actions, B, features_dim
        self.osp, self.asp = spaces.Box(0, 255, shape, np.uint8), spaces.Discrete(n_actions)
        th.manual_seed(seed)
        self.ref = dqn_cnn_ref.CnnPolicy(self.osp, self.asp, lambda _: LR, features_extractor_kwargs=dict(features_dim=features_dim))
        with th.no_grad():   # (a target that differs from the online net, as between two target updates)
            for q in self.ref.q_net_target.parameters():
                q.add_(0.05 * th.randn_like(q) * q.abs().mean())
        fb, self.n_new = int(np.prod(shape)), B // 2
        self.tables = {}
        for name, rows in (("ring", 12), ("expert", 9)):
            self.tables[name] = dict(
                obs=rng.integers(0, 256, size=(rows, fb), dtype=np.uint8), next_obs=rng.integers(0, 256, size=(rows, fb), dtype=np.uint8),
                action=rng.integers(0, n_actions, size=rows), done=(rng.uniform(size=rows) < 0.3).astype(np.float32),
                # |TD| < 1 under the small rewards (either sign), >= 1 under the large ones (|Q| is well below 1 at
                # initialisation); the large ones share a sign, so their gradients add up and 0.5 clips
                reward=np.where(np.arange(rows) % 3 == 0, 0.1 * rng.choice([-1.0, 1.0], size=rows), 3.0).astype(np.float32))
        self.idx = np.stack([np.concatenate([rng.integers(0, 12, size=self.n_new), rng.integers(0, 9, size=B - self.n_new)])
                             for _ in range(steps)]).astype(np.int64)

    def batch(self, s=0):
        i, n = self.idx[s], self.n_new
        return {k: np.concatenate([self.tables["ring"][k][i[:n]], self.tables["expert"][k][i[n:]]]) for k in self.tables["ring"]}

    def reference_step(self, dtype, max_grad_norm):
        pol = copy.deepcopy(self.ref).to(dtype)
        opt = th.optim.Adam(pol.q_net.parameters(), lr=LR)
        b = self.batch()
        frames = lambda a: th.as_tensor(a.reshape((-1,) + self.shape))
        rew, done = (th.as_tensor(b[k]).to(dtype).reshape(-1, 1) for k in ("reward", "done"))
        with th.no_grad():
            nq = pol.q_net_target(frames(b["next_obs"])).max(dim=1)[0].reshape(-1, 1)
            target = rew + (1 - done) * GAMMA * nq
        cur = th.gather(pol.q_net(frames(b["obs"])), dim=1, index=th.as_tensor(b["action"]).long().reshape(-1, 1))
        loss = F.smooth_l1_loss(cur, target)
        opt.zero_grad()
        loss.backward()
        norm = th.nn.utils.clip_grad_norm_(pol.q_net.parameters(), max_grad_norm)
        names = [k for k, _ in pol.q_net.named_parameters()]
        out = {"loss": loss.item(), "grad_norm": float(norm), "abs_td": (cur - target).detach().abs().numpy()}
        out.update({f"grad/{k}": q.grad.detach().numpy().copy() for k, q in zip(names, pol.q_net.parameters())})
        opt.step()
        for k, q in zip(names, pol.q_net.parameters()):
            out[f"param/{k}"] = q.detach().numpy().copy()
            out[f"exp_avg/{k}"] = opt.state[q]["exp_avg"].numpy().copy()
            out[f"exp_avg_sq/{k}"] = opt.state[q]["exp_avg_sq"].numpy().copy()
        return out

    def device_policy(self):
        pol = p.CnnPolicy(self.osp, self.asp, lambda _: LR, features_extractor_kwargs=dict(features_dim=self.fdim)).to("cuda")
        pol.load_state_dict(self.ref.state_dict())
        return pol

    def device_tables(self):
        out = []
        for name in ("ring", "expert"):
            h = self.tables[name]
            t = dqn._Table(len(h["obs"]), h["obs"].shape[1], "cuda", frames=True)
            t.write(0, h["obs"], h["next_obs"], h["action"], h["reward"], h["done"])
            out.append(t)
        return out


_step_data = {}


def step_data(name):
    if name not in _step_data:
        shape, A, B, fdim, mgn = STEP_CASES[name]
        d = StepData(shape, A, B, fdim)
        _step_data[name] = (d, d.reference_step(th.float32, mgn), d.reference_step(th.float64, mgn))
    return _step_data[name]


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_update_frames_step_matches_the_float64_restatement(name):
    mgn = STEP_CASES[name][4]
    d, r32, r64 = step_data(name)
    assert (r64["abs_td"] < 1).any() and (r64["abs_td"] >= 1).any(), "both Huber branches must occur"
    assert (r64["grad_norm"] > mgn) if mgn < 1 else (r64["grad_norm"] < mgn), r64["grad_norm"]
    pol = d.device_policy()
    ring, expert = d.device_tables()
    stats, grad = th.empty(1, 2, device="cuda"), th.empty(pol.q_net._flat.numel(), device="cuda")
    pol.check_rows(d.idx, d.n_new, ring, expert)
    pol.update(ring, expert, th.from_numpy(d.idx).cuda(), d.n_new, 1, d.B, GAMMA, mgn, LR, stats, grad)
    got = {"loss": float(stats[0, 0]), "grad_norm": float(stats[0, 1])}
    q = pol.q_net
    for tag, flat in (("grad", grad), ("exp_avg", pol.exp_avg), ("exp_avg_sq", pol.exp_avg_sq), ("param", q._flat)):
        got.update({f"{tag}/{k}": v.cpu().numpy() for k, v in q.grad_to_torch(flat).items()})
    assert pol.adam_steps == 1
    worst = []
    for k in (k for k in r64 if k != "abs_td"):
        dref, dev = rel(r32[k], r64[k]), rel(got[k], r64[k])
        print(f"{name} {k}: dref {dref:.3e}, device {dev:.3e} ({dev / max(dref, 1e-300):.2f} x)")
        if dev > 8 * dref:
            worst.append((k, dev, dref))
    assert not worst, worst
    # the target net is read, never written
    for k, v in pol.q_net_target.state_dict().items():
        assert th.equal(v.cpu(), d.ref.q_net_target.state_dict()[k]), k


def _run_steps(d, pol, ring, expert, idx, calls):
    """`idx` [G, B] in `calls` equal `update` calls; returns everything a step leaves behind."""
    G = len(idx)
    stats, grad = th.empty(G, 2, device="cuda"), th.empty(pol.q_net._flat.numel(), device="cuda")
    idx_dev = th.from_numpy(idx).cuda()
    per = G // calls
    for c in range(calls):
        pol.update(ring, expert, idx_dev[c * per:(c + 1) * per], d.n_new, per, d.B, GAMMA, 10.0, LR, stats[c * per:(c + 1) * per], grad)
    return [t.clone() for t in (stats, grad, pol.q_net._flat, pol.exp_avg, pol.exp_avg_sq)]


def test_update_frames_repeats_bit_for_bit():
    d = StepData((3, 44, 48), 4, 7, 32, seed=2, steps=3)
    ring, expert = d.device_tables()
    once = _run_steps(d, d.device_policy(), ring, expert, d.idx[:1], 1)
    again = _run_steps(d, d.device_policy(), ring, expert, d.idx[:1], 1)
    for a, b in zip(once, again):
        assert th.equal(a, b)
    pol = d.device_policy()
    three_in_one = _run_steps(d, pol, ring, expert, d.idx, 1)
    assert pol.adam_steps == 3
    one_by_one = _run_steps(d, d.device_policy(), ring, expert, d.idx, 3)
    for a, b in zip(three_in_one, one_by_one):
        assert th.equal(a, b)
    assert not th.equal(three_in_one[2], once[2]) and bool(th.isfinite(three_in_one[2]).all())


@pytest.mark.parametrize("n_envs", [1, 4])
def test_q_values_rows_do_not_depend_on_the_batch(n_envs):
    d, _, _ = step_data("min_map_clipped")
    pol = d.device_policy()
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, size=(16,) + d.shape, dtype=np.uint8)
    with th.no_grad():
        q32 = d.ref.q_net(th.as_tensor(frames[:n_envs])).numpy()
        q64 = copy.deepcopy(d.ref).double().q_net(th.as_tensor(frames[:n_envs])).numpy()
    dref = rel(q32, q64)
    q, am = pol.q_values(frames[:n_envs])
    big = pol.q_net.forward(th.from_numpy(frames).cuda())["q"][:n_envs].cpu().numpy()
    assert q.shape == (n_envs, d.A) and q.dtype == np.float32 and am.dtype == np.int64
    for what, dev in (("against the larger batch's rows", rel(q, big)), ("against float64", rel(q, q64)),
                      ("larger batch against float64", rel(big, q64))):
        print(f"q_values n_envs={n_envs} {what}: dref {dref:.3e}, device {dev:.3e} ({dev / dref:.2f} x)")
        assert dev <= 8 * dref, what
    assert np.array_equal(am, np.argmax(q, axis=1))   # (NumPy's arg-max is the first maximum)
    one, am_one = pol.q_values(frames[0])             # a single unbatched frame
    assert one.shape == (1, d.A) and am_one.shape == (1,)
