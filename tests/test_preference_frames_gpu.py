"""`ia_pref_gather_frames` on the MI355X, bit for bit: the uint8 frame table gathered into the reward CNN's channel-last
fp32 input against torch's own ops on the device (`frames[idx].float() / 255.0`, the permute and the cat of
`CnnRewardNet.forward`, the channel-last copy of `Cnn.forward`). Every comparison is `torch.equal`.

Shapes: one pixel; rows that are no multiple of 16 bytes (5 x 7 x 1, 5 x 7 x 3: frames start at every alignment and X's
rows do too); the goldens' shapes; the tutorial's 84 x 84 x 4 (seven tiles a row). Indices repeat, are out of order, and
reach frame 0 and the table's last frame; the table holds exactly F * H * W * C bytes."""
import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from imitation_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (5, 7, 1), (5, 7, 3), (12, 20, 3), (9, 11, 4), (84, 84, 4)]
FLAGS = [(1, 0), (0, 1), (1, 1)]
N_ROWS = [1, 3, 130]
F = 7
SENTINEL = -7.25


def _table(H, W, C, chw, seed):
    """A table of exactly F * H * W * C bytes (its own allocation), random bytes, in the given layout."""
    g = th.Generator().manual_seed(seed)
    flat = th.empty(F * H * W * C, dtype=th.uint8, device="cuda")
    flat.copy_(th.randint(0, 256, (F * H * W * C,), generator=g, dtype=th.uint8))
    return flat.view((F, C, H, W) if chw else (F, H, W, C))


def _indices(n, use_next):
    """State frames of n rows: the last frame a row may name first (F - 1, or F - 2 when the next frame is read too, so
    the next frame is the table's last), frame 0, repeats, no order."""
    top = F - 2 if use_next else F - 1
    pattern = [top, 0, top, 3, 3, 1, 0, 2, top - 1, 1]
    return th.tensor((pattern * (n // len(pattern) + 1))[:n], dtype=th.int64, device="cuda")


def _reference(frames, idx, chw, use_state, use_next):
    """torch on the device: preprocess, `CnnRewardNet.forward`'s channel-first cat, `Cnn.forward`'s channel-last copy."""
    images = []
    for on, step in ((use_state, 0), (use_next, 1)):
        if on:
            x = frames[idx + step].float() / 255.0
            images.append(x if chw else x.permute(0, 3, 1, 2))
    return th.cat(images, dim=1).permute(0, 2, 3, 1).contiguous()


def _raw(frames, idx, H, W, C, chw, use_state, use_next, lut, front=0):
    """The C entry point writing into the middle of a sentinel-filled buffer: (X, floats before it, 64 floats after it)."""
    n, cin = idx.numel(), C * (use_state + use_next)
    size = n * H * W * cin
    buf = th.full((front + size + 64,), SENTINEL, device="cuda")
    X = buf[front:front + size]
    if lut is None:
        L.call("ia_pref_gather_frames", L.ptr(frames), L.ptr(idx), n, H, W, C, int(chw), use_state, use_next,
               X.data_ptr(), L.stream())
    else:
        L.call("ia_pref_gather_frames_lut", L.ptr(frames), frames.shape[0], L.ptr(idx), n, H, W, C, int(chw), use_state,
               use_next, L.ptr(lut), X.data_ptr(), L.stream())
    return X.view(n, H, W, cin), buf[:front], buf[front + size:]


@pytest.mark.parametrize("flags", FLAGS, ids=["state", "next", "both"])
@pytest.mark.parametrize("chw", [False, True], ids=["hwc", "chw"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_frames_equals_torch(shape, chw, flags):
    H, W, C = shape
    use_state, use_next = flags
    frames = _table(H, W, C, chw, seed=H * 100 + C)
    assert frames.numel() == F * H * W * C and frames.untyped_storage().nbytes() == F * H * W * C
    lut = ops._byte_lut(frames.device)
    for n in N_ROWS:
        idx = _indices(n, use_next)
        want = _reference(frames, idx, chw, use_state, use_next)
        got = ops.pref_gather_frames(frames, idx, bool(use_state), bool(use_next), chw)
        assert got.shape == want.shape and got.dtype == th.float32 and got.is_contiguous()
        assert th.equal(got, want), (n, int((got != want).sum()))
        X, _, tail = _raw(frames, idx, H, W, C, chw, use_state, use_next, lut)
        assert th.equal(X, want), n
        assert tail.numel() == 64 and bool((tail == SENTINEL).all()), n   # nothing written behind X


@pytest.mark.parametrize("chw", [False, True], ids=["hwc", "chw"])
@pytest.mark.parametrize("front", [1, 2, 3])
def test_gather_frames_into_unaligned_output(front, chw):
    """X starting 4, 8 and 12 bytes past a 16-byte boundary: the vector stores move, the values do not."""
    H, W, C = 9, 11, 4
    frames = _table(H, W, C, chw, seed=front)
    idx = _indices(3, True)
    X, head, tail = _raw(frames, idx, H, W, C, chw, 1, 1, ops._byte_lut(frames.device), front=front)
    assert th.equal(X, _reference(frames, idx, chw, 1, 1))
    assert bool((head == SENTINEL).all()) and bool((tail == SENTINEL).all())


@pytest.mark.parametrize("chw", [False, True], ids=["hwc", "chw"])
def test_all_byte_values(chw):
    """Frame 1 holds every byte value once; the op agrees with torch's device `x.float() / 255.0` on all 256, and the
    entry point without a table is IEEE division (`numpy`'s float32 quotient)."""
    H, W, C = 8, 8, 4
    frames = _table(H, W, C, chw, seed=0)
    frames[1].view(-1).copy_(th.arange(256, dtype=th.uint8))
    idx = th.tensor([1, 0], dtype=th.int64, device="cuda")
    got = ops.pref_gather_frames(frames, idx, True, True, chw)
    assert th.equal(got, _reference(frames, idx, chw, 1, 1))
    assert sorted(set((got[0, :, :, :C] * 255.0).round().long().reshape(-1).tolist())) == list(range(256))
    X, _, tail = _raw(frames, idx, H, W, C, chw, 1, 1, None)
    f = frames.cpu().numpy()
    parts = [(f[[1, 0]].astype(np.float32) / np.float32(255)), (f[[2, 1]].astype(np.float32) / np.float32(255))]
    if chw:
        parts = [q.transpose(0, 2, 3, 1) for q in parts]
    assert np.array_equal(X.cpu().numpy(), np.concatenate(parts, axis=3))
    assert bool((tail == SENTINEL).all())


def test_rows_outside_the_table_read_nothing():
    H, W, C = 5, 7, 3
    frames = _table(H, W, C, False, seed=3)
    idx = th.tensor([2, F - 1, -1, 0], dtype=th.int64, device="cuda")    # row 1's next frame and row 2's state: not there
    got = ops.pref_gather_frames(frames, idx, True, True, False)
    want = _reference(frames, th.tensor([2, 0], device="cuda"), False, 1, 1)
    assert th.equal(got[[0, 3]], want)
    assert bool(th.isnan(got[1]).all()) and bool(th.isnan(got[2]).all())


def test_bad_arguments_return_the_error_code():
    frames = _table(5, 7, 3, False, seed=4)
    idx = _indices(3, False)
    X = th.empty(3 * 5 * 7 * 6, device="cuda")
    fn = L.load().ia_pref_gather_frames
    st = L.stream()
    assert fn(L.ptr(frames), L.ptr(idx), 3, 5, 7, 3, 0, 0, 0, L.ptr(X), st) == L.ERR_ARG
    assert fn(L.ptr(frames), L.ptr(idx), 0, 5, 7, 3, 0, 1, 0, L.ptr(X), st) == L.ERR_ARG
    assert fn(L.ptr(frames), L.ptr(idx), 3, 0, 7, 3, 0, 1, 0, L.ptr(X), st) == L.ERR_ARG
    assert fn(L.ptr(frames), L.ptr(idx), 3, 5, -1, 3, 0, 1, 0, L.ptr(X), st) == L.ERR_ARG
    assert fn(L.ptr(frames), L.ptr(idx), 3, 5, 7, 0, 0, 1, 1, L.ptr(X), st) == L.ERR_ARG
    with pytest.raises(RuntimeError, match="ia_pref_gather_frames_lut failed with code -1"):
        ops.pref_gather_frames(frames, idx, False, False, False)
    with pytest.raises(ValueError, match="uint8"):
        ops.pref_gather_frames(frames.float(), idx, True, False, False)
