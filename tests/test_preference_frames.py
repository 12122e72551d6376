"""The frame table of preference comparisons on image fragments, host side: its index arithmetic against
`flatten_trajectories`, and which table `PreferenceDataset.device_table` picks."""
import numpy as np
import pytest

from imitation_amd import data_types as dt
from imitation_amd import preference_comparisons as pc


def _image_dataset(lens, shape=(5, 7, 3), seed=0, terminal_every=3):
    """Pairs of uint8 image fragments with the given lengths (pair i's two fragments share lens[i])."""
    r = np.random.default_rng(seed)
    pairs = []
    for i, L in enumerate(lens):
        pair = []
        for k in range(2):
            pair.append(dt.TrajectoryWithRew(obs=r.integers(0, 256, size=(L + 1, *shape), dtype=np.uint8),
                                             acts=r.integers(4, size=L).astype(np.int64),
                                             rews=r.normal(size=L).astype(np.float32), infos=None,
                                             terminal=(2 * i + k) % terminal_every == 0))
        pairs.append(tuple(pair))
    ds = pc.PreferenceDataset()
    ds.push(pairs, r.uniform(size=len(lens)).astype(np.float32))
    return ds


def _flat_dataset(lens, seed=0):
    r = np.random.default_rng(seed)
    pairs = [tuple(dt.TrajectoryWithRew(obs=r.normal(size=(L + 1, 6)).astype(np.float32),
                                        acts=r.normal(size=(L, 2)).astype(np.float32),
                                        rews=r.normal(size=L).astype(np.float32), infos=None, terminal=False)
                   for _ in range(2)) for L in lens]
    ds = pc.PreferenceDataset()
    ds.push(pairs, r.uniform(size=len(lens)).astype(np.float32))
    return ds


@pytest.mark.parametrize("lens", [[5] * 6, [1, 1, 1], [3, 1, 7, 2, 7, 4]], ids=["equal", "ones", "mixed"])
def test_frame_index_matches_flatten_trajectories(lens):
    ds = _image_dataset(lens)
    a = pc.frame_table_arrays(ds, discrete=True)
    frames = a["frames"]
    assert frames.dtype == np.uint8 and frames.shape == (2 * sum(L + 1 for L in lens), 5, 7, 3)
    assert np.array_equal(a["pair_len"], lens)
    flat_table = pc._FragmentTable(ds, "cpu", True)
    r = np.random.default_rng(1)
    for pairs in (np.arange(len(lens)), r.permutation(len(lens)), np.array([len(lens) - 1, 0, 0, len(lens) - 1]),
                  np.array([2])):
        idx, off = pc.frame_table_index(a["pair_len"], pairs)
        frags = [f for p in pairs for f in (ds.fragments1[p], ds.fragments2[p])]
        tr = dt.flatten_trajectories(frags)
        assert idx.dtype == np.int64 and idx.shape == (len(tr.obs),)
        assert idx.min() >= 0 and idx.max() + 1 < len(frames)
        assert np.array_equal(frames[idx], tr.obs)
        assert np.array_equal(frames[idx + 1], tr.next_obs)
        assert np.array_equal(a["acts"][idx], tr.acts)
        assert np.array_equal(a["dones"][idx].astype(bool), tr.dones)
        assert np.array_equal(a["gt"][idx], tr.rews)
        rows, off_flat = flat_table.batch(pairs)
        assert np.array_equal(off, off_flat) and off.dtype == off_flat.dtype
        assert len(rows) == len(idx)


def test_frame_index_reaches_first_and_last_frame():
    ds = _image_dataset([2, 4])
    a = pc.frame_table_arrays(ds, discrete=True)
    idx, off = pc.frame_table_index(a["pair_len"], np.array([0, 1]))
    assert idx[0] == 0 and idx[-1] + 1 == len(a["frames"]) - 1
    assert list(off) == [0, 2, 6]
    assert list(idx) == [0, 1, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14]


def test_device_table_picks_frames_for_images_only():
    img, flat = _image_dataset([3, 2]), _flat_dataset([3, 2])
    t = img.device_table("cpu", True)
    assert isinstance(t, pc._FrameTable)
    assert t.frames.dtype.is_floating_point is False and tuple(t.frames.shape) == (2 * (4 + 3), 5, 7, 3)
    assert t.frames.element_size() == 1 and t.acts.dtype.is_floating_point is False
    assert img.device_table("cpu", True) is t                           # cached
    assert isinstance(img.device_table("cpu", True, frames=False), pc._FragmentTable)   # a caller that reads flat rows
    assert isinstance(flat.device_table("cpu", False), pc._FragmentTable)
    # float images and uint8 vectors are not the image space
    r = np.random.default_rng(0)
    odd = pc.PreferenceDataset()
    odd.push([tuple(dt.TrajectoryWithRew(obs=r.uniform(size=(3, 5, 7, 3)).astype(np.float32),
                                         acts=np.zeros(2, np.int64), rews=np.zeros(2, np.float32), infos=None,
                                         terminal=False) for _ in range(2))], np.array([1.0], np.float32))
    assert isinstance(odd.device_table("cpu", True), pc._FragmentTable)


def test_frame_table_rejects_unequal_pair():
    ds = _image_dataset([3])
    ds.fragments2[0] = _image_dataset([2]).fragments1[0]
    with pytest.raises(ValueError, match="same length"):
        pc.frame_table_arrays(ds, discrete=True)
