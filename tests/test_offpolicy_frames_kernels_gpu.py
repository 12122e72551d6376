"""The frame path's kernels (csrc/offpolicy_frames.hip) one by one: `ia_offpolicy_frames_step`, `ia_offpolicy_frames_reward`,
`ia_disc_gather_frames`, `ia_gather_frame_rows`.

Data movement is compared bit for bit with NumPy, the CNN input `X` bit for bit with `bytes.float() / 255` permuted to
channel-last. Every output lies between canary rows, which must stay untouched, and every row of an output the launch does
not name must keep its canary too. Out-of-range indices are tried against tables DECLARED smaller than their backing
allocation, so a broken guard shows as a wrong value, not as a fault. The reward epilogue and one discriminator minibatch
(forward and parameter gradients) are compared with float64 torch on the CPU from the same bytes, within 8 x the deviation of
torch's own float32 CPU result from that float64 result, computed here."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import _lib as L
from imitation_amd import ops, spaces

pytestmark = pytest.mark.gpu

SHAPES = [(4, 36, 36),   # 5184 bytes: two chunks, rows 16-byte aligned
          (3, 44, 48),   # 6336 bytes
          (3, 5, 7),     # 105 bytes: odd, rows on the byte path
          (1, 1, 1)]
FLAGS = [(1, 0), (0, 1), (1, 1)]   # (use_state, use_next_state)
PAD = 2                            # canary rows on either side
U8_CANARY, I64_CANARY, F32_CANARY = 0xA5, -77, -12345.0
DEV = "cuda"


def guarded(rows, width, dtype, canary):
    """(whole, view): `view` = rows [PAD, PAD + rows) of `whole`, everything filled with `canary`."""
    shape = (rows + 2 * PAD,) + ((width,) if width else ())
    whole = th.full(shape, canary, dtype=dtype, device=DEV)
    return whole, whole[PAD:PAD + rows]


def canaries_intact(whole, canary):
    w = whole.cpu()
    return bool((w[:PAD] == canary).all() and (w[-PAD:] == canary).all())


def x_ref(obs, nxt, shape, us, un):
    """`bytes.float() / 255` as the device evaluates it (what `preprocess` feeds the CNN on the host path), state channels
    first, channel-last."""
    n = len(obs)
    parts = [th.from_numpy(a.reshape((n,) + shape)).to(DEV).float() / 255 for on, a in ((us, obs), (un, nxt)) if on]
    return th.cat(parts, dim=1).permute(0, 2, 3, 1).contiguous().cpu()


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


class Step:
    """One `ia_offpolicy_frames_step` problem: pinned record, guarded ring / tile / X, the argument record."""

    def __init__(self, shape, n, us, un, seed=0):
        r = np.random.default_rng(seed)
        self.shape, self.n = shape, n
        FB = int(np.prod(shape))
        Cc, H, W = shape
        self.obs, self.nxt = (r.integers(0, 256, size=(n, FB), dtype=np.uint8) for _ in range(2))
        self.act = r.integers(0, 5, size=n).astype(np.int64)
        self.dones = (r.uniform(size=n) < 0.5).astype(np.uint8)
        self.ring_done = (self.dones * (r.uniform(size=n) < 0.5)).astype(np.float32)
        self.pinned = [th.from_numpy(a).pin_memory() for a in (self.obs, self.nxt, self.act, self.dones, self.ring_done)]
        self.ring_rows, self.tile_rows = 3 * n, 4 * n
        self.ring_row, self.tile_row = self.ring_rows - n, 2 * n       # the step ends on the ring's last row
        g = lambda rows, width, dt, c: guarded(rows, width, dt, c)
        self.ring_obs, self.ring_next = g(self.ring_rows, FB, th.uint8, U8_CANARY), g(self.ring_rows, FB, th.uint8, U8_CANARY)
        self.ring_act, self.ring_rew = g(self.ring_rows, 0, th.int64, I64_CANARY), g(self.ring_rows, 0, th.float32, F32_CANARY)
        self.ring_done_out = g(self.ring_rows, 0, th.float32, F32_CANARY)
        self.tile_obs, self.tile_next = g(self.tile_rows, FB, th.uint8, U8_CANARY), g(self.tile_rows, FB, th.uint8, U8_CANARY)
        self.tile_act, self.tile_dones = g(self.tile_rows, 0, th.int64, I64_CANARY), g(self.tile_rows, 0, th.uint8, U8_CANARY)
        self.X = g(n, H * W * Cc * (us + un), th.float32, F32_CANARY)
        self.rewards_host = th.full((n + 2 * PAD,), F32_CANARY).pin_memory()
        self.lut = ops._byte_lut(th.device(DEV))
        a = self.args = L.OffpolicyFramesArgs()
        a.obs, a.next_obs, a.act, a.dones, a.ring_done = (t.data_ptr() for t in self.pinned)
        a.n, a.C, a.H, a.W, a.use_state, a.use_next_state = n, Cc, H, W, us, un
        a.lut, a.X = self.lut.data_ptr(), self.X[1].data_ptr()
        a.ring_obs, a.ring_next_obs = self.ring_obs[1].data_ptr(), self.ring_next[1].data_ptr()
        a.ring_action, a.ring_reward = self.ring_act[1].data_ptr(), self.ring_rew[1].data_ptr()
        a.ring_done_out, a.ring_row, a.ring_rows = self.ring_done_out[1].data_ptr(), self.ring_row, self.ring_rows
        a.tile_obs, a.tile_next_obs = self.tile_obs[1].data_ptr(), self.tile_next[1].data_ptr()
        a.tile_act, a.tile_dones = self.tile_act[1].data_ptr(), self.tile_dones[1].data_ptr()
        a.tile_row, a.tile_rows = self.tile_row, self.tile_rows
        a.rewards_host = self.rewards_host.data_ptr() + 4 * PAD

    def launch(self):
        L.check(L.load().ia_offpolicy_frames_step(C.byref(self.args), L.stream()), "ia_offpolicy_frames_step")
        th.cuda.synchronize()


def rows_written(view, lo, n, want, canary):
    """Rows [lo, lo + n) of `view` equal `want`, every other row still holds its canary."""
    got = view.cpu().numpy()
    mask = np.ones(len(got), bool)
    mask[lo:lo + n] = False
    return np.array_equal(got[lo:lo + n], want) and bool((got[mask] == canary).all())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 4, 17])
@pytest.mark.parametrize("us,un", FLAGS)
def test_step_store(shape, n, us, un):
    s = Step(shape, n, us, un, seed=n)
    s.launch()
    for (whole, view), want, canary in ((s.ring_obs, s.obs, U8_CANARY), (s.ring_next, s.nxt, U8_CANARY),
                                        (s.ring_act, s.act, I64_CANARY), (s.ring_done_out, s.ring_done, F32_CANARY)):
        assert rows_written(view, s.ring_row, n, want, canary) and canaries_intact(whole, canary)
    for (whole, view), want, canary in ((s.tile_obs, s.obs, U8_CANARY), (s.tile_next, s.nxt, U8_CANARY),
                                        (s.tile_act, s.act, I64_CANARY), (s.tile_dones, s.dones, U8_CANARY)):
        assert rows_written(view, s.tile_row, n, want, canary) and canaries_intact(whole, canary)
    want = x_ref(s.obs, s.nxt, shape, us, un)
    assert th.equal(s.X[1].cpu().reshape(want.shape), want)
    assert canaries_intact(s.X[0], F32_CANARY)
    # the step store leaves the rewards alone
    assert bool((s.ring_rew[0].cpu() == F32_CANARY).all()) and bool((s.rewards_host == F32_CANARY).all())


def test_step_store_refuses_rows_past_a_table():
    s = Step((3, 5, 7), 4, 1, 1)
    lib = L.load()
    for field, value in (("ring_row", s.ring_rows - 3), ("tile_row", s.tile_rows - 3), ("ring_row", -1)):
        keep = getattr(s.args, field)
        setattr(s.args, field, value)
        assert lib.ia_offpolicy_frames_step(C.byref(s.args), L.stream()) == L.ERR_ARG
        assert lib.ia_offpolicy_frames_reward(C.byref(s.args), None, 0, s.ring_rew[1].data_ptr(), 3, 1, 0, 0,
                                              L.stream()) == L.ERR_ARG
        setattr(s.args, field, keep)
    th.cuda.synchronize()
    for whole in (s.ring_obs[0], s.tile_obs[0], s.tile_dones[0]):
        assert bool((whole.cpu() == U8_CANARY).all())


def _select64(use_action, use_done, n_actions, out, act, dones, softplus, dtype):
    """`CnnRewardNet._select` (+ GAIL's `-logsigmoid(-x)`) by torch on the CPU in `dtype`."""
    space = spaces.Box(0, 255, (3, 5, 7), np.uint8)
    net = p.modules.CnnRewardNet(space, spaces.Discrete(n_actions), use_action=use_action, use_done=use_done,
                                 hwc_format=False, hid_channels=(2,))
    o = th.from_numpy(out).to(dtype)
    if o.shape[1] == 1:
        o = o[:, 0]
    onehot = th.nn.functional.one_hot(th.from_numpy(act), n_actions).to(dtype)
    r = net._select(o, onehot, th.from_numpy(dones.astype(np.float32)).to(dtype))
    # (`_select` multiplies by a float32 selector: the products are exact in either width)
    r = r.to(dtype)
    return (-th.nn.functional.logsigmoid(-r) if softplus else r).numpy()


@pytest.mark.parametrize("use_action,use_done", [(1, 0), (1, 1), (0, 1), (0, 0)])
@pytest.mark.parametrize("softplus", [0, 1])
def test_reward_store(use_action, use_done, softplus):
    n, A = 17, 5
    s = Step((3, 5, 7), n, 1, 0, seed=3)
    s.launch()   # (fills the tile rows the reward launch reads its actions and dones from)
    n_out = (A if use_action else 1) * (2 if use_done else 1)
    r = np.random.default_rng(7)
    out = (4.0 * r.normal(size=(n, n_out))).astype(np.float32)
    out_d = th.from_numpy(out).to(DEV)
    L.check(L.load().ia_offpolicy_frames_reward(C.byref(s.args), out_d.data_ptr(), n_out, None, A, use_action, use_done,
                                                softplus, L.stream()), "ia_offpolicy_frames_reward")
    th.cuda.synchronize()
    got = s.ring_rew[1].cpu().numpy()
    assert (got[:s.ring_row] == F32_CANARY).all() and canaries_intact(s.ring_rew[0], F32_CANARY)
    host = s.rewards_host.numpy()
    assert (host[:PAD] == F32_CANARY).all() and (host[-PAD:] == F32_CANARY).all()
    assert np.array_equal(host[PAD:PAD + n], got[s.ring_row:])
    want64 = _select64(use_action, use_done, A, out, s.act, s.dones, softplus, th.float64)
    want32 = _select64(use_action, use_done, A, out, s.act, s.dones, softplus, th.float32)
    dref, dev = rel(want32, want64), rel(got[s.ring_row:], want64)
    print(f"reward epilogue action={use_action} done={use_done} softplus={softplus}: torch f32 {dref:.3e}, device {dev:.3e}")
    assert dev <= 8 * dref
    # nothing else was touched by the reward launch
    assert rows_written(s.ring_obs[1], s.ring_row, n, s.obs, U8_CANARY)
    assert rows_written(s.tile_act[1], s.tile_row, n, s.act, I64_CANARY)


def test_reward_store_takes_a_ready_vector():
    n = 4
    s = Step((1, 1, 1), n, 1, 1, seed=5)
    s.launch()
    rew = th.from_numpy(np.random.default_rng(1).normal(size=n).astype(np.float32)).to(DEV)
    lib = L.load()
    L.check(lib.ia_offpolicy_frames_reward(C.byref(s.args), None, 0, rew.data_ptr(), 3, 1, 1, 1, L.stream()), "reward")
    th.cuda.synchronize()
    assert np.array_equal(s.ring_rew[1].cpu().numpy()[s.ring_row:], rew.cpu().numpy())
    assert np.array_equal(s.rewards_host.numpy()[PAD:PAD + n], rew.cpu().numpy())
    # exactly one source; a CNN output of the wrong width
    out = th.zeros(n, 6, device=DEV)
    assert lib.ia_offpolicy_frames_reward(C.byref(s.args), out.data_ptr(), 6, rew.data_ptr(), 3, 1, 1, 0, L.stream()) == L.ERR_ARG
    assert lib.ia_offpolicy_frames_reward(C.byref(s.args), None, 0, None, 3, 1, 1, 0, L.stream()) == L.ERR_ARG
    assert lib.ia_offpolicy_frames_reward(C.byref(s.args), out.data_ptr(), 5, None, 3, 1, 1, 0, L.stream()) == L.ERR_ARG


class Tables:
    """An expert table and a generator ring of uint8 transitions, backed by more rows than they declare."""

    def __init__(self, shape, seed=0, e_rows=7, g_rows=9, spare=3):
        r = np.random.default_rng(seed)
        FB = int(np.prod(shape))
        self.rows = (e_rows, g_rows)
        self.np, self.dev = [], []
        for rows in self.rows:
            t = dict(obs=r.integers(0, 256, size=(rows + spare, FB), dtype=np.uint8),
                     nxt=r.integers(0, 256, size=(rows + spare, FB), dtype=np.uint8),
                     act=r.integers(0, 4, size=rows + spare).astype(np.int64),
                     dones=(r.uniform(size=rows + spare) < 0.4).astype(np.uint8))
            self.np.append(t)
            self.dev.append({k: th.from_numpy(v).to(DEV) for k, v in t.items()})

    def gather(self, idx_e, idx_g, shape, us, un):
        mb = len(idx_e)
        Cc, H, W = shape
        Xw, X = guarded(2 * mb, H * W * Cc * (us + un), th.float32, F32_CANARY)
        aw, acts = guarded(2 * mb, 0, th.int64, I64_CANARY)
        dw, dones = guarded(2 * mb, 0, th.float32, F32_CANARY)
        ie, ig = (th.from_numpy(np.asarray(i, np.int64)).to(DEV) for i in (idx_e, idx_g))
        e, g = self.dev
        L.call("ia_disc_gather_frames", L.ptr(e["obs"]), L.ptr(e["nxt"]), L.ptr(e["act"]), L.ptr(e["dones"]), self.rows[0],
               L.ptr(g["obs"]), L.ptr(g["nxt"]), L.ptr(g["act"]), L.ptr(g["dones"]), self.rows[1], L.ptr(ie), L.ptr(ig), mb,
               H, W, Cc, us, un, L.ptr(ops._byte_lut(th.device(DEV))), L.ptr(X), L.ptr(acts), L.ptr(dones), L.stream())
        th.cuda.synchronize()
        return (Xw, X), (aw, acts), (dw, dones)

    def rows_of(self, key, idx_e, idx_g):
        return np.concatenate([self.np[0][key][np.asarray(idx_e)], self.np[1][key][np.asarray(idx_g)]])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mb", [1, 3, 16])
@pytest.mark.parametrize("us,un", FLAGS)
def test_disc_gather(shape, mb, us, un):
    t = Tables(shape, seed=mb)
    r = np.random.default_rng(mb + 10)
    idx_e, idx_g = r.integers(0, t.rows[0], size=mb), r.integers(0, t.rows[1], size=mb)
    idx_e[-1], idx_g[0] = t.rows[0] - 1, t.rows[1] - 1     # the last declared row of either table
    (Xw, X), (aw, acts), (dw, dones) = t.gather(idx_e, idx_g, shape, us, un)
    want = x_ref(t.rows_of("obs", idx_e, idx_g), t.rows_of("nxt", idx_e, idx_g), shape, us, un)
    assert th.equal(X.cpu().reshape(want.shape), want)
    assert np.array_equal(acts.cpu().numpy(), t.rows_of("act", idx_e, idx_g))
    assert np.array_equal(dones.cpu().numpy(), t.rows_of("dones", idx_e, idx_g).astype(np.float32))
    assert canaries_intact(Xw, F32_CANARY) and canaries_intact(aw, I64_CANARY) and canaries_intact(dw, F32_CANARY)


@pytest.mark.parametrize("shape", [(4, 36, 36), (3, 5, 7)])
def test_disc_gather_rows_outside_their_table(shape):
    t = Tables(shape, seed=1)
    idx_e = np.array([0, t.rows[0], 3, -1])                # (the row behind the declared table exists in the allocation)
    idx_g = np.array([t.rows[1] + 1, 2, 1 << 40, 8])
    bad = np.array([0, 1, 0, 1, 1, 0, 1, 0], bool)
    (Xw, X), (aw, acts), (dw, dones) = t.gather(idx_e, idx_g, shape, 1, 1)
    ok_e, ok_g = np.where(bad[:4], 0, idx_e), np.where(bad[4:], 0, idx_g)
    want = x_ref(t.rows_of("obs", ok_e, ok_g), t.rows_of("nxt", ok_e, ok_g), shape, 1, 1)
    got = X.cpu().reshape(want.shape)
    for i in range(8):
        if bad[i]:
            assert bool(th.isnan(got[i]).all()), i
            assert int(acts[i]) == I64_CANARY and float(dones[i]) == F32_CANARY, i
        else:
            assert th.equal(got[i], want[i]), i
            assert int(acts[i]) == int(t.rows_of("act", ok_e, ok_g)[i]), i
    assert canaries_intact(Xw, F32_CANARY) and canaries_intact(aw, I64_CANARY) and canaries_intact(dw, F32_CANARY)


@pytest.mark.parametrize("shape", SHAPES)
def test_row_gather_wraps_like_the_replay_buffer(shape):
    FB = int(np.prod(shape))
    r = np.random.default_rng(2)
    src_rows, spare, cap, at, n = 12, 2, 10, 7, 6
    src = dict(obs=r.integers(0, 256, size=(src_rows + spare, FB), dtype=np.uint8),
               nxt=r.integers(0, 256, size=(src_rows + spare, FB), dtype=np.uint8),
               act=r.integers(0, 4, size=src_rows + spare).astype(np.int64),
               dones=(r.uniform(size=src_rows + spare) < 0.4).astype(np.uint8))
    dev = {k: th.from_numpy(v).to(DEV) for k, v in src.items()}
    order = r.permutation(src_rows)[:n].astype(np.int64)
    order[2] = src_rows          # outside the declared tile (inside its allocation): that ring row keeps its canary
    outs = dict(obs=guarded(cap, FB, th.uint8, U8_CANARY), nxt=guarded(cap, FB, th.uint8, U8_CANARY),
                act=guarded(cap, 0, th.int64, I64_CANARY), dones=guarded(cap, 0, th.uint8, U8_CANARY))
    L.call("ia_gather_frame_rows", L.ptr(dev["obs"]), L.ptr(dev["nxt"]), L.ptr(dev["act"]), L.ptr(dev["dones"]), src_rows,
           L.ptr(th.from_numpy(order).to(DEV)), n, FB, L.ptr(outs["obs"][1]), L.ptr(outs["nxt"][1]), L.ptr(outs["act"][1]),
           L.ptr(outs["dones"][1]), at, cap, L.stream())
    th.cuda.synchronize()
    for k, canary in (("obs", U8_CANARY), ("nxt", U8_CANARY), ("act", I64_CANARY), ("dones", U8_CANARY)):
        want = np.full_like(outs[k][1].cpu().numpy(), canary)
        for i in range(n):   # `ReplayBuffer.store`: rows at, at + 1, ... wrapping at the capacity
            if i != 2:
                want[(at + i) % cap] = src[k][order[i]]
        assert np.array_equal(outs[k][1].cpu().numpy(), want), k
        assert canaries_intact(outs[k][0], canary), k
    lib = L.load()
    assert lib.ia_gather_frame_rows(L.ptr(dev["obs"]), L.ptr(dev["nxt"]), L.ptr(dev["act"]), L.ptr(dev["dones"]), src_rows,
                                    L.ptr(th.from_numpy(order).to(DEV)), cap + 1, FB, L.ptr(outs["obs"][1]),
                                    L.ptr(outs["nxt"][1]), L.ptr(outs["act"][1]), L.ptr(outs["dones"][1]), at, cap,
                                    L.stream()) == L.ERR_ARG


def _torch_logits(cnn, net, X_nchw, onehot, dones):
    h = X_nchw
    for name in cnn._convs:
        h = th.relu(getattr(cnn, name)(h))
    out = getattr(cnn, cnn._final)(h.mean(dim=(2, 3)))
    return net._select(out, onehot, dones)


def test_discriminator_minibatch_forward_and_gradient():
    """One minibatch as `_disc_update_frames` runs it -- `ia_disc_gather_frames`, `forward_nhwc`, the BCE, `backward()` --
    against float64 torch on the CPU from the same bytes."""
    shape, mb, A = (4, 36, 36), 3, 4
    th.manual_seed(3)
    space = spaces.Box(0, 255, shape, np.uint8)
    net = p.modules.CnnRewardNet(space, spaces.Discrete(A), use_state=True, use_action=True, use_next_state=True,
                                 use_done=True, hwc_format=False)
    host = copy.deepcopy(net)
    net = net.to(DEV)
    t = Tables(shape, seed=4)
    idx_e, idx_g = np.array([1, 6, 3]), np.array([8, 0, 5])
    (_, X), (_, acts), (_, dones) = t.gather(idx_e, idx_g, shape, 1, 1)
    X = X.reshape(2 * mb, shape[1], shape[2], 2 * shape[0])
    onehot = th.nn.functional.one_hot(acts, A).float()
    logits = net.forward_nhwc(X, onehot, dones)
    loss, _ = ops.bce_expert_first(logits, mb, 1.0)
    loss.backward()
    got = {"logits": logits.detach().cpu().numpy()}
    got.update({k: v.grad.cpu().numpy() for k, v in net.named_parameters()})
    labels = th.cat([th.ones(mb), th.zeros(mb)])
    ref = {}
    for dtype in (th.float32, th.float64):
        m = copy.deepcopy(host).to(dtype)
        # (the bytes are scaled in float32, as `preprocess` scales them, then widened)
        x = x_ref(t.rows_of("obs", idx_e, idx_g), t.rows_of("nxt", idx_e, idx_g), shape, 1, 1).permute(0, 3, 1, 2)
        assert th.equal(x, X.cpu().permute(0, 3, 1, 2))
        lg = _torch_logits(m.cnn, m, x.to(dtype), onehot.cpu().to(dtype), dones.cpu().to(dtype))
        th.nn.functional.binary_cross_entropy_with_logits(lg, labels.to(dtype)).backward()
        ref[dtype] = {"logits": lg.detach().numpy()}
        ref[dtype].update({k: v.grad.numpy() for k, v in m.named_parameters()})
    worst = []
    for k, want in ref[th.float64].items():
        dref, dev = rel(ref[th.float32][k], want), rel(got[k], want)
        print(f"disc minibatch {k}: torch f32 {dref:.3e}, device {dev:.3e}")
        if dev > 8 * dref:
            worst.append((k, dev, dref))
    assert not worst, worst
