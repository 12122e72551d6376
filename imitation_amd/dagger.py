"""DAgger behind the reference's surface (`algorithms/dagger.py`): beta schedules, `InteractiveTrajectoryCollector`,
`DAggerTrainer`, `SimpleDAggerTrainer`, `reconstruct_trainer` -- same names, arguments, defaults, errors, logger keys
and the same random draws in the same order (`rng.uniform` for the per-step mask, `rng.bytes(16)` per saved file,
torch's global generator for the learner's sample on the masked rows only).

Two differences in mechanism:

* The collection step. Every environment step needs the expert's deterministic action for all environments (the stored
  label) and the learner's sampled action for the environments the mask hands to the robot. When both are fused-shape
  policies of this package over the same spaces with the same hidden width, `SimpleDAggerTrainer` computes both in ONE
  launch (`ia_dagger_act`, csrc/dagger.hip) that reads the observations from pinned host memory and writes the two
  action tiles back there: one launch and one wait per step. Any other expert (a callable, a `PPO` outside those shapes)
  goes through `rollout.policy_to_callable` and two `predict` calls, exactly as the reference does. The choice follows
  from the policies' types and shapes alone; both paths produce the same bits.
* The aggregated dataset stays on the device across rounds: a growing table (`obs [cap, D]`, `acts [cap, A]`) that the
  fused step appends to as it goes and that trajectories read from disk are uploaded into once. Episodes still running
  when a round ends are never saved, and the dataset's order is by trajectory in sorted file-name order, round by
  round -- so the trainer keeps a host row map (dataset position -> table row) and hands BC the table plus the map
  (`BC.set_demonstrations_device`). The demonstration files are written as before: they are the public contract and
  what `reconstruct_trainer` resumes from.
"""
from __future__ import annotations

import abc
import ctypes as C
import logging
import os
import pathlib
import uuid
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch as th

from imitation_amd import _lib as L
from imitation_amd import data_types as dt
from imitation_amd import logger as imit_logger
from imitation_amd import rollout, serialize
from imitation_amd.policies import ActorCriticPolicy
from imitation_amd.ppo import OnPolicyAlgorithm
from imitation_amd.vec_env import VecEnv, VecEnvWrapper


class BetaSchedule(abc.ABC):
    """Computes beta (% of time demonstration action used) from training round."""

    @abc.abstractmethod
    def __call__(self, round_num: int) -> float:
        """The fraction of the time to take the demonstrator's action in round `round_num` (numbered from 0)."""


class LinearBetaSchedule(BetaSchedule):
    """Linearly-decreasing schedule for beta: 1 at round 0, 0 from `rampdown_rounds` on."""

    def __init__(self, rampdown_rounds: int) -> None:
        self.rampdown_rounds = rampdown_rounds

    def __call__(self, round_num: int) -> float:
        assert round_num >= 0
        return min(1, max(0, (self.rampdown_rounds - round_num) / self.rampdown_rounds))


class ExponentialBetaSchedule(BetaSchedule):
    """Exponentially decaying schedule for beta: `decay_probability ** round_num`."""

    def __init__(self, decay_probability: float):
        if not (0 < decay_probability <= 1):
            raise ValueError("decay_probability lies outside the range (0, 1].")
        self.decay_probability = decay_probability

    def __call__(self, round_num: int) -> float:
        assert round_num >= 0
        return self.decay_probability**round_num


def _parse_path(path) -> pathlib.Path:
    """`util.parse_path`: a resolved, absolute `pathlib.Path`."""
    if isinstance(path, bytes):
        path = path.decode()
    return pathlib.Path(path).resolve()


def reconstruct_trainer(scratch_dir, venv: VecEnv, custom_logger: Optional[imit_logger.HierarchicalLogger] = None,
                        device: Union[th.device, str] = "auto") -> "DAggerTrainer":
    """Reconstruct trainer from the latest snapshot (`checkpoint-latest.pt`) in `scratch_dir`. The environment and the
    logger cannot be serialised and are given anew. The aggregated dataset is read back from the demonstration files of
    the scratch directory (in the order it was built) the next time it is needed."""
    custom_logger = custom_logger or imit_logger.configure()
    scratch_dir = _parse_path(scratch_dir)
    checkpoint_path = scratch_dir / "checkpoint-latest.pt"
    trainer = th.load(checkpoint_path, map_location=th.device("cuda" if device == "auto" else device), weights_only=False)
    trainer.venv = venv
    trainer.logger = custom_logger
    return trainer


def _save_dagger_demo(trajectory: dt.TrajectoryWithRew, trajectory_index: int, save_dir, rng: np.random.Generator,
                      prefix: str = "") -> pathlib.Path:
    save_dir = _parse_path(save_dir)
    assert isinstance(trajectory, dt.TrajectoryWithRew)
    actual_prefix = f"{prefix}-" if prefix else ""
    randbits = int.from_bytes(rng.bytes(16), "big")
    random_uuid = uuid.UUID(int=randbits, version=4).hex
    filename = f"{actual_prefix}dagger-demo-{trajectory_index}-{random_uuid}.npz"
    npz_path = save_dir / filename
    assert not npz_path.exists(), "The following DAgger demonstration path already exists: {0}".format(npz_path)
    serialize.save(npz_path, [trajectory])
    logging.info(f"Saved demo at '{npz_path}'")
    return npz_path


class _EpisodeAccumulator:
    """The part of the reference's `TrajectoryAccumulator` the collector uses: per-environment partial episodes; a done
    step closes the episode on its terminal observation and the next one starts from the post-reset observation."""

    def __init__(self, first_obs: np.ndarray):
        self._obs = [[np.array(o)] for o in first_obs]
        self._acts: List[list] = [[] for _ in first_obs]
        self._rews: List[list] = [[] for _ in first_obs]
        self._infos: List[list] = [[] for _ in first_obs]

    def add_steps_and_auto_finish(self, acts, obs, rews, dones, infos) -> List[Tuple[int, dt.TrajectoryWithRew]]:
        out = []
        for i in range(len(obs)):
            done = bool(dones[i])
            self._acts[i].append(np.array(acts[i]))
            self._rews[i].append(rews[i])
            self._infos[i].append(infos[i])
            self._obs[i].append(np.array(infos[i]["terminal_observation"] if done else obs[i]))
            if done:
                # infos that only restate the episode's end (what the trajectory encodes) are dropped, as `rollout` does
                keep = rollout._has_content(self._infos[i])
                clean = [{k: v for k, v in f.items() if k != "terminal_observation"} for f in self._infos[i]]
                out.append((i, dt.TrajectoryWithRew(obs=np.stack(self._obs[i]), acts=np.stack(self._acts[i]),
                                                    rews=np.asarray(self._rews[i]),
                                                    infos=np.array(clean) if keep else None, terminal=True)))
                self._obs[i], self._acts[i], self._rews[i], self._infos[i] = [np.array(obs[i])], [], [], []
        return out


class InteractiveTrajectoryCollector(VecEnvWrapper):
    """DAgger VecEnvWrapper for querying and saving expert actions.

    Every call to `.step(actions)` accepts and saves expert actions to `self.save_dir`, but only forwards them to the
    wrapped VecEnv with probability `self.beta`; with probability `1 - self.beta` a "robot" action (from
    `get_robot_acts`) is forwarded instead, independently per environment and step. Finished episodes are saved at once
    as `dagger-demo-{index}-{uuid}.npz` through `serialize.save`; every saved action is the expert's.
    """

    def __init__(self, venv: VecEnv, get_robot_acts: Callable[[np.ndarray], np.ndarray], beta: float, save_dir,
                 rng: np.random.Generator) -> None:
        super().__init__(venv)
        self.get_robot_acts = get_robot_acts
        assert 0 <= beta <= 1
        self.beta = beta
        self.traj_accum: Optional[_EpisodeAccumulator] = None
        self.save_dir = save_dir
        self._last_obs: Optional[np.ndarray] = None
        self._done_before = True
        self._is_reset = False
        self._last_user_actions: Optional[np.ndarray] = None
        self.rng = rng

    def seed(self, seed: Optional[int] = None) -> List[Optional[int]]:
        """Seeds the collector's generator (the mask and file-name draws) and the wrapped VecEnv."""
        self.rng = np.random.default_rng(seed=seed)
        return list(self.venv.seed(seed))

    def reset(self) -> np.ndarray:
        obs = self.venv.reset()
        assert isinstance(obs, np.ndarray)
        self.traj_accum = _EpisodeAccumulator(obs)
        self._last_obs = obs
        self._is_reset = True
        self._last_user_actions = None
        return obs

    def _draw_mask(self) -> np.ndarray:
        return self.rng.uniform(0, 1, size=(self.num_envs,)) > self.beta

    def step_async(self, actions: np.ndarray) -> None:
        """Steps with a `1 - beta` chance per environment of executing `self.get_robot_acts` instead of `actions`."""
        assert self._is_reset, "call .reset() before .step()"
        assert self._last_obs is not None
        # Replace each given action with a robot action 100*(1-beta)% of the time.
        actual_acts = np.array(actions)
        mask = self._draw_mask()
        if np.sum(mask) != 0:
            actual_acts[mask] = self.get_robot_acts(self._last_obs[mask])
        self._last_user_actions = actions
        self.venv.step_async(actual_acts)

    def _on_saved(self, path: pathlib.Path, env_index: int) -> None:
        pass

    def step_wait(self):
        """Returns the wrapped step's result; stores the transition and saves every episode that ended."""
        next_obs, rews, dones, infos = self.venv.step_wait()
        assert isinstance(next_obs, np.ndarray)
        assert self.traj_accum is not None
        assert self._last_user_actions is not None
        self._last_obs = next_obs
        fresh_demos = self.traj_accum.add_steps_and_auto_finish(acts=self._last_user_actions, obs=next_obs, rews=rews,
                                                                dones=dones, infos=infos)
        for traj_index, (env_index, traj) in enumerate(fresh_demos):
            self._on_saved(_save_dagger_demo(traj, traj_index, self.save_dir, self.rng), env_index)
        return next_obs, rews, dones, infos


class DeviceDemoTable:
    """The aggregated dataset on the device: `obs [cap, D]` and `acts [cap, W]` fp32 tables that double when full, the
    number of rows in use, and the host row map -- dataset position p is table row `row_map[p]`. Rows are appended by
    the fused collection step (one block of `n_envs` rows per environment step, row `base + i` for environment i) or
    uploaded from trajectories; only rows named by the map belong to the dataset."""

    def __init__(self, obs_dim: int, act_width: int, device, capacity: int = 4096):
        self.device = th.device(device)
        self.obs = th.empty(capacity, obs_dim, device=self.device)
        self.acts = th.empty(capacity, act_width, device=self.device)
        self.rows = 0
        self._map_buf = np.zeros(0, dtype=np.int64)
        self.row_map = self._map_buf[:0]

    @property
    def capacity(self) -> int:
        return self.obs.shape[0]

    def reserve(self, extra: int) -> int:
        """Room for `extra` more rows (the tables move when they grow) -> the first of them."""
        need = self.rows + extra
        if need > self.capacity:
            cap = self.capacity
            while cap < need:
                cap *= 2
            for name in ("obs", "acts"):
                old = getattr(self, name)
                new = th.empty(cap, old.shape[1], device=self.device)
                new[:self.rows].copy_(old[:self.rows])
                setattr(self, name, new)
        return self.rows

    def upload(self, trajectory) -> np.ndarray:
        """The trajectory's transitions (observation before each action, the action) as new rows -> their row numbers."""
        k = len(trajectory.acts)
        base = self.reserve(k)
        obs = np.ascontiguousarray(np.asarray(trajectory.obs)[:-1].reshape(k, -1), dtype=np.float32)
        acts = np.ascontiguousarray(np.asarray(trajectory.acts).reshape(k, -1), dtype=np.float32)
        self.obs[base:base + k].copy_(th.from_numpy(obs))
        self.acts[base:base + k].copy_(th.from_numpy(acts))
        self.rows += k
        return np.arange(base, base + k, dtype=np.int64)

    def extend_map(self, rows: np.ndarray) -> None:
        """Appends dataset positions (amortised: the map's buffer doubles); the new rows must be rows in use."""
        rows = np.asarray(rows, dtype=np.int64)
        assert len(rows) == 0 or (rows.min() >= 0 and rows.max() < self.rows)
        k, n = len(self.row_map), len(rows)
        if k + n > len(self._map_buf):
            buf = np.empty(max(2 * len(self._map_buf), k + n, 1024), dtype=np.int64)
            buf[:k] = self._map_buf[:k]
            self._map_buf = buf
        self._map_buf[k:k + n] = rows
        self.row_map = self._map_buf[:k + n]


class EpisodeRowTracker:
    """Which table rows hold each environment's running episode when every environment step appends one block of
    `n_envs` rows (row `base + i` for environment i): `step(base)` after each append, `finish(i)` when environment i's
    episode ends -> the rows of its steps, in order. Rows of episodes that never finish are never handed out."""

    def __init__(self, n_envs: int):
        self._rows: List[List[int]] = [[] for _ in range(n_envs)]

    def step(self, base: int) -> None:
        for i, r in enumerate(self._rows):
            r.append(base + i)

    def finish(self, env_index: int) -> np.ndarray:
        rows, self._rows[env_index] = self._rows[env_index], []
        return np.asarray(rows, dtype=np.int64)


def build_row_map(file_names: Sequence[str], rows_of_file: Mapping[str, np.ndarray]) -> np.ndarray:
    """The dataset order of one round: its files in sorted name order, each file's rows in step order."""
    parts = [np.asarray(rows_of_file[f], dtype=np.int64) for f in sorted(file_names)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def _fused_policy(p) -> Optional[ActorCriticPolicy]:
    """The fused-shape MLP policy behind `p` (a policy, or an algorithm holding one), or None."""
    if isinstance(p, OnPolicyAlgorithm):
        p = p.policy
    if type(p).__module__.endswith("cnn_policy") or not isinstance(p, ActorCriticPolicy):
        return None
    if not getattr(p, "fused", False) or p.hidden not in (32, 64) or p.device.type != "cuda":
        return None
    return p


class _FusedStep:
    """One `ia_dagger_act` launch per environment step: observations, mask and the learner's draws go in through pinned
    host memory, the expert's labels and the executed actions (or the learner's logits, for a Discrete head sampled on
    the host) come back the same way; the host waits once. With a table the step also appends (observation, label)."""

    def __init__(self, expert: ActorCriticPolicy, learner: ActorCriticPolicy, n: int, table: Optional[DeviceDemoTable]):
        self.expert, self.learner, self.n, self.table = expert, learner, n, table
        D, A = learner.obs_dim, learner.act_dim
        self.discrete = learner.discrete
        self.host_sampling = learner.samples_on_host
        W = 1 if self.discrete else A
        pin = lambda *s, dtype=th.float32: th.zeros(*s, dtype=dtype).pin_memory()
        self.h_obs, self.h_mask, self.h_noise = pin(n, D), pin(n, dtype=th.uint8), pin(n, W)
        self.h_expert, self.h_actual = pin(n, W), pin(n, W)
        self.h_logits = pin(n, A) if self.host_sampling else None
        self._np = {k: getattr(self, k).numpy() for k in ("h_obs", "h_mask", "h_noise", "h_expert", "h_actual")}
        self._fn = L.load().ia_dagger_act

    @staticmethod
    def supported(expert, learner, venv) -> bool:
        e, l = _fused_policy(expert), _fused_policy(learner)
        if e is None or l is None or e is l:
            return False
        return (e.hidden == l.hidden and e.discrete == l.discrete and e.obs_dim == l.obs_dim and e.act_dim == l.act_dim
                and e.observation_space == l.observation_space and e.action_space == l.action_space
                and e.device == l.device and len(venv.observation_space.shape) == 1)

    def __call__(self, obs: np.ndarray, mask: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
        """-> (expert actions, executed actions, first table row of the step or -1), as `predict` returns them."""
        e, l, n = self.expert, self.learner, self.n
        # `predict` puts a policy in eval mode (the feature statistics are read, not updated): the expert every step,
        # the learner on the steps it is asked
        e.set_training_mode(False)
        k = int(mask.sum())
        self._np["h_obs"][:] = obs.reshape(n, -1)
        self._np["h_mask"][:] = mask
        if k:
            l.set_training_mode(False)
            if not self.host_sampling:   # the learner's draws: the masked rows only, as `forward` draws them
                self._np["h_noise"][mask] = l.sample_noise(k).numpy().reshape(k, -1)
        tab, base = self.table, -1
        if tab is not None:
            base = tab.reserve(n)
        enm, env_ = e._norm_ptrs()
        lnm, lnv = l._norm_ptrs()
        rc = self._fn(C.byref(e.desc), L.ptr(e._flat), L.ptr(e._flat_t), enm, env_, C.byref(l.desc), L.ptr(l._flat),
                      L.ptr(l._flat_t), lnm, lnv, self.h_obs.data_ptr(), n, self.h_mask.data_ptr(),
                      self.h_noise.data_ptr(), L.ptr(l._low), L.ptr(l._high), self.h_expert.data_ptr(),
                      self.h_actual.data_ptr(), None if self.h_logits is None else self.h_logits.data_ptr(),
                      None if tab is None else L.ptr(tab.obs), None if tab is None else L.ptr(tab.acts),
                      max(base, 0), 0 if tab is None else tab.capacity, L.stream())
        L.check(rc, "ia_dagger_act")
        th.cuda.current_stream().synchronize()
        if tab is not None:
            tab.rows += n
        shape = (n, *l.action_space.shape)
        if self.discrete:
            expert_acts = self._np["h_expert"].reshape(n).astype(np.int64).reshape(shape)
            actual = np.array(expert_acts)
            if k and self.host_sampling:   # [SB3 CategoricalDistribution.sample] on the masked rows' logits
                dist = th.distributions.Categorical(logits=self.h_logits[th.from_numpy(np.flatnonzero(mask))])
                actual[mask] = dist.sample().numpy().reshape((k, *l.action_space.shape))
            elif k:
                actual[mask] = self._np["h_actual"].reshape(n)[mask].astype(np.int64).reshape((k, *shape[1:]))
        else:
            expert_acts = self._np["h_expert"].reshape(shape).copy()
            actual = self._np["h_actual"].reshape(shape).copy()
        return expert_acts, actual, base


class _FusedCollector(InteractiveTrajectoryCollector):
    """The collector of the fused path: `expert_actions(obs)` draws the step's mask, runs the fused step and keeps the
    executed actions for the `step_async` that follows (which then neither draws nor asks the robot again)."""

    def __init__(self, *args, fused_step: _FusedStep, on_file: Optional[Callable[[pathlib.Path, np.ndarray], None]],
                 **kwargs):
        super().__init__(*args, **kwargs)
        self._fused_step = fused_step
        self._on_file = on_file
        self._tracker = EpisodeRowTracker(self.num_envs)
        self._pending = None

    def reset(self) -> np.ndarray:
        self._tracker = EpisodeRowTracker(self.num_envs)
        self._pending = None
        return super().reset()

    def expert_actions(self, obs: np.ndarray, states=None, episode_starts=None):
        assert self._is_reset, "call .reset() before .step()"
        mask = self._draw_mask()
        expert_acts, actual, base = self._fused_step(obs, mask)
        if base >= 0 and self._tracker is not None:
            self._tracker.step(base)
        self._pending = (expert_acts, actual, mask)
        return expert_acts, states

    def step_async(self, actions: np.ndarray) -> None:
        if self._pending is None:
            # a step whose actions did not come from `expert_actions`: the reference's composition; its rows were not
            # appended by the fused step, so the episode's file is uploaded when it is loaded
            self._tracker = None
            return super().step_async(actions)
        assert self._is_reset, "call .reset() before .step()"
        expert_acts, actual, mask = self._pending
        self._pending = None
        if actions is not expert_acts and not np.array_equal(np.asarray(actions), expert_acts):
            # the caller stores other actions than the expert's: this step's mask and the robot's actions are already
            # drawn and are used as they are (nothing is drawn twice); the table rows hold the expert's labels, so
            # files of this collector are uploaded from disk instead
            self._tracker = None
            robot = actual                       # (the fused step's executed tile: the learner's actions where masked)
            actual = np.array(actions)
            actual[mask] = robot[mask]
        self._last_user_actions = actions
        self.venv.step_async(actual)

    def _on_saved(self, path: pathlib.Path, env_index: int) -> None:
        if self._tracker is not None and self._on_file is not None and self._fused_step.table is not None:
            self._on_file(path, self._tracker.finish(env_index))


class NeedsDemosException(Exception):
    """Signals demos need to be collected for current round before continuing."""


class DAggerTrainer:
    """DAgger training class with low-level API suitable for interactive human feedback.

    BC with helpers for resuming training and interpolating between the demonstrator's and the learnt policy, in
    rounds: fresh demonstrations first, then `BC` on everything collected so far. Layout of `scratch_dir`:
    `checkpoint-NNN.pt`, `checkpoint-latest.pt`, `policy-NNN.pt`, `policy-latest.pt`, `demos/round-NNN/*.npz`.
    """

    DEFAULT_N_EPOCHS: int = 4
    """The default number of BC training epochs in `extend_and_update`."""

    def __init__(self, *, venv: VecEnv, scratch_dir, rng: np.random.Generator,
                 beta_schedule: Optional[Callable[[int], float]] = None, bc_trainer,
                 custom_logger: Optional[imit_logger.HierarchicalLogger] = None):
        self._logger = custom_logger or imit_logger.configure()
        if beta_schedule is None:
            beta_schedule = LinearBetaSchedule(15)
        self.beta_schedule = beta_schedule
        self.scratch_dir = _parse_path(scratch_dir)
        self.venv = venv
        self.round_num = 0
        self._last_loaded_round = -1
        self._all_demos: List[dt.TrajectoryWithRew] = []   # (re-upload mode only: see `device_table`)
        self.rng = rng
        # [SB3 check_for_correct_spaces]
        if bc_trainer.observation_space != venv.observation_space:
            raise ValueError(f"Observation spaces do not match: {bc_trainer.observation_space} != {venv.observation_space}")
        if bc_trainer.action_space != venv.action_space:
            raise ValueError(f"Action spaces do not match: {bc_trainer.action_space} != {venv.action_space}")
        self.bc_trainer = bc_trainer
        self.bc_trainer.logger = self.logger
        # The aggregated dataset lives in a device table (None: `bc_trainer` has no `set_demonstrations_device`, or
        # trains an image policy -- every round then flattens and hands over all demonstrations, as the reference does).
        # `device_table = False` before the first load selects that mode by hand (measurements, equivalence tests).
        self.device_table = hasattr(bc_trainer, "set_demonstrations_device") and not getattr(bc_trainer, "_image", False)
        self._table: Optional[DeviceDemoTable] = None
        self._file_rows: Dict[str, np.ndarray] = {}    # demonstration file -> table rows the fused step gave its steps

    def __getstate__(self):
        """State excluding what cannot be pickled (environment, logger) and the device table: the demonstration files
        are the durable copy, read back on the next load."""
        d = dict(self.__dict__)
        del d["venv"]
        del d["_logger"]
        d["_table"], d["_file_rows"], d["_all_demos"], d["_last_loaded_round"] = None, {}, [], -1
        return d

    @property
    def logger(self) -> imit_logger.HierarchicalLogger:
        return self._logger

    @logger.setter
    def logger(self, value: imit_logger.HierarchicalLogger) -> None:
        # DAgger and inner-BC logger should stay in sync
        self._logger = value
        self.bc_trainer.logger = value

    @property
    def policy(self):
        return self.bc_trainer.policy

    @property
    def batch_size(self) -> int:
        return self.bc_trainer.batch_size

    # ---- the aggregated dataset ------------------------------------------------------------------------------
    def _demo_table(self) -> DeviceDemoTable:
        if self._table is None:
            pol = self.policy
            self._table = DeviceDemoTable(pol.obs_dim, 1 if pol.discrete else pol.act_dim, pol.device)
        return self._table

    def _note_file_rows(self, path: pathlib.Path, rows: np.ndarray) -> None:
        self._file_rows[str(path)] = rows

    def _load_all_demos(self) -> Tuple[int, List[int]]:
        """Rounds not loaded yet, files in sorted name order -> (transitions in the dataset, files per round)."""
        num_demos_by_round = []
        for round_num in range(self._last_loaded_round + 1, self.round_num + 1):
            round_dir = self._demo_dir_path_for_round(round_num)
            demo_paths = self._get_demo_paths(round_dir)
            if self.device_table:
                table = self._demo_table()
                for p in demo_paths:   # rows the fused step wrote while collecting, else one upload of the file
                    rows = self._file_rows.pop(str(p), None)
                    table.extend_map(rows if rows is not None else table.upload(serialize.load(p)[0]))
            else:
                self._all_demos.extend(serialize.load(p)[0] for p in demo_paths)
            num_demos_by_round.append(len(demo_paths))
        if self.device_table:
            return len(self._demo_table().row_map), num_demos_by_round
        logging.info(f"Loaded {len(self._all_demos)} total")
        return sum(len(t) for t in self._all_demos), num_demos_by_round

    def _get_demo_paths(self, round_dir: pathlib.Path) -> List[pathlib.Path]:
        # listdir's order depends on the file system: sort by the file name
        filenames = sorted(os.listdir(round_dir))
        return [round_dir / f for f in filenames if f.endswith(".npz")]

    def _demo_dir_path_for_round(self, round_num: Optional[int] = None) -> pathlib.Path:
        if round_num is None:
            round_num = self.round_num
        return self.scratch_dir / "demos" / f"round-{round_num:03d}"

    def _try_load_demos(self) -> None:
        """Load the dataset for this round into self.bc_trainer."""
        demo_dir = self._demo_dir_path_for_round()
        demo_paths = self._get_demo_paths(demo_dir) if demo_dir.is_dir() else []
        if len(demo_paths) == 0:
            raise NeedsDemosException(
                f"No demos found for round {self.round_num} in dir '{demo_dir}'. "
                f"Maybe you need to collect some demos? See "
                f".create_trajectory_collector()",
            )
        if self._last_loaded_round < self.round_num:
            n_transitions, num_demos = self._load_all_demos()
            logging.info(f"Loaded {sum(num_demos)} new demos from {len(num_demos)} rounds")
            if n_transitions < self.batch_size:
                raise ValueError(
                    "Not enough transitions to form a single batch: "
                    f"self.batch_size={self.batch_size} > "
                    f"len(transitions)={n_transitions}",
                )
            if self.device_table:
                table = self._demo_table()
                self.bc_trainer.set_demonstrations_device(table.obs, table.acts, table.row_map)
            else:
                self.bc_trainer.set_demonstrations(dt.flatten_trajectories(self._all_demos))
            # The reference hands BC a `DataLoader`, and `BC.set_demonstrations` -> `make_data_loader` peeks at its
            # first batch (`util.get_first_iter_element`): one loader iterator (a base-seed draw) and one sampler pass
            # (a seed draw; its `randperm` runs on a private generator) -- two int64 draws from torch's global
            # generator per hand-over, before the first epoch draws its own.
            dt.ExpertIndexStream._draw_int64()
            dt.ExpertIndexStream._draw_int64()
            self._last_loaded_round = self.round_num
        elif self.device_table and self._table is not None:
            # (the tables may have moved since: a collector of this round appended to them)
            self.bc_trainer.set_demonstrations_device(self._table.obs, self._table.acts, self._table.row_map)

    def extend_and_update(self, bc_train_kwargs: Optional[Mapping[str, Any]] = None) -> int:
        """Loads new transitions (if necessary), trains BC and advances the round counter -> the new round number.
        Raises `NeedsDemosException` (and does neither) when the current round has no demonstrations yet. Defaults:
        `log_rollouts_venv = self.venv`; `n_epochs = DEFAULT_N_EPOCHS` unless `n_epochs` or `n_batches` is given."""
        if bc_train_kwargs is None:
            bc_train_kwargs = {}
        else:
            bc_train_kwargs = dict(bc_train_kwargs)
        user_keys = bc_train_kwargs.keys()
        if "log_rollouts_venv" not in user_keys:
            bc_train_kwargs["log_rollouts_venv"] = self.venv
        if "n_epochs" not in user_keys and "n_batches" not in user_keys:
            bc_train_kwargs["n_epochs"] = self.DEFAULT_N_EPOCHS
        logging.info("Loading demonstrations")
        self._try_load_demos()
        logging.info(f"Training at round {self.round_num}")
        self.bc_trainer.train(**bc_train_kwargs)
        self.round_num += 1
        logging.info(f"New round number is {self.round_num}")
        return self.round_num

    def create_trajectory_collector(self) -> InteractiveTrajectoryCollector:
        """A collector with the current round's beta, save directory and the learner as the robot."""
        save_dir = self._demo_dir_path_for_round()
        beta = self.beta_schedule(self.round_num)
        return InteractiveTrajectoryCollector(venv=self.venv,
                                              get_robot_acts=lambda acts: self.bc_trainer.policy.predict(acts)[0],
                                              beta=beta, save_dir=save_dir, rng=self.rng)

    def save_trainer(self) -> Tuple[pathlib.Path, pathlib.Path]:
        """Snapshot of the trainer (`checkpoint-NNN.pt`, `checkpoint-latest.pt`; reload with `reconstruct_trainer`) and
        a second copy of the policy on its own (`policy-NNN.pt`, `policy-latest.pt`) -> the two numbered paths."""
        self.scratch_dir.mkdir(parents=True, exist_ok=True)
        checkpoint_paths = [self.scratch_dir / f"checkpoint-{self.round_num:03d}.pt",
                            self.scratch_dir / "checkpoint-latest.pt"]
        for checkpoint_path in checkpoint_paths:
            th.save(self, checkpoint_path)
        policy_paths = [self.scratch_dir / f"policy-{self.round_num:03d}.pt", self.scratch_dir / "policy-latest.pt"]
        for policy_path in policy_paths:
            th.save(self.policy, policy_path)
        return checkpoint_paths[0], policy_paths[0]


class SimpleDAggerTrainer(DAggerTrainer):
    """Simpler subclass of DAggerTrainer for training with synthetic feedback."""

    def __init__(self, *, venv: VecEnv, scratch_dir, expert_policy, rng: np.random.Generator,
                 expert_trajs: Optional[Sequence[dt.TrajectoryWithRew]] = None, **dagger_trainer_kwargs):
        super().__init__(venv=venv, scratch_dir=scratch_dir, rng=rng, **dagger_trainer_kwargs)
        self.expert_policy = expert_policy
        # (a plain callable carries no spaces: it is taken as is, like `rollout.policy_to_callable` takes it)
        if hasattr(expert_policy, "observation_space") or not callable(expert_policy):
            if expert_policy.observation_space != self.venv.observation_space:
                raise ValueError("Mismatched observation space between expert_policy and venv")
            if expert_policy.action_space != self.venv.action_space:
                raise ValueError("Mismatched action space between expert_policy and venv")
        if expert_trajs is not None:
            # Save each initial expert trajectory into the "round 0" demonstration data directory.
            for traj_index, traj in enumerate(expert_trajs):
                _save_dagger_demo(traj, traj_index, self._demo_dir_path_for_round(), self.rng, prefix="initial_data")
        self._fused_step: Optional[_FusedStep] = None

    def __getstate__(self):
        d = super().__getstate__()
        d["_fused_step"] = None
        return d

    def _collection(self):
        """(collector, policy argument, deterministic flag) of one round's `generate_trajectories` call: the fused step
        when the expert and the learner are fused-shape policies of the same shapes, else the reference's composition."""
        if not _FusedStep.supported(self.expert_policy, self.policy, self.venv):
            return self.create_trajectory_collector(), self.expert_policy, not (
                callable(self.expert_policy) and not isinstance(self.expert_policy, (OnPolicyAlgorithm, ActorCriticPolicy)))
        table = self._demo_table() if self.device_table else None
        fs = self._fused_step
        if fs is None or fs.n != self.venv.num_envs or fs.table is not table:
            fs = self._fused_step = _FusedStep(_fused_policy(self.expert_policy), self.policy, self.venv.num_envs, table)
        collector = _FusedCollector(venv=self.venv, get_robot_acts=lambda acts: self.bc_trainer.policy.predict(acts)[0],
                                    beta=self.beta_schedule(self.round_num), save_dir=self._demo_dir_path_for_round(),
                                    rng=self.rng, fused_step=fs, on_file=self._note_file_rows)
        return collector, collector.expert_actions, False

    def train(self, total_timesteps: int, *, rollout_round_min_episodes: int = 3,
              rollout_round_min_timesteps: int = 500, bc_train_kwargs: Optional[dict] = None) -> None:
        """Rounds of dataset aggregation (the expert acts; with probability `1 - beta` per environment and step the
        learner's action is executed instead; the expert's action is what is stored) followed by `BC.train` on all data
        so far, until `total_timesteps` environment steps were collected (a lower bound: a round finishes its episodes).
        A round collects at least `max(rollout_round_min_timesteps, batch_size)` steps and
        `rollout_round_min_episodes` episodes."""
        total_timestep_count = 0
        round_num = 0
        while total_timestep_count < total_timesteps:
            collector, policy, deterministic = self._collection()
            round_episode_count = 0
            round_timestep_count = 0
            sample_until = rollout.make_sample_until(
                min_timesteps=max(rollout_round_min_timesteps, self.batch_size),
                min_episodes=rollout_round_min_episodes,
            )
            trajectories = rollout.generate_trajectories(policy=policy, venv=collector, sample_until=sample_until,
                                                         deterministic_policy=deterministic, rng=collector.rng)
            for traj in trajectories:
                self._logger.record_mean("dagger/mean_episode_reward", np.sum(traj.rews))
                round_timestep_count += len(traj)
                total_timestep_count += len(traj)
            round_episode_count += len(trajectories)
            self._logger.record("dagger/total_timesteps", total_timestep_count)
            self._logger.record("dagger/round_num", round_num)
            self._logger.record("dagger/round_episode_count", round_episode_count)
            self._logger.record("dagger/round_timestep_count", round_timestep_count)
            # `logger.dump` is called inside BC.train within the following fn call:
            self.extend_and_update(bc_train_kwargs)
            round_num += 1
