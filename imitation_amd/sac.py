"""SAC, the stochastic continuous-action learner SQIL can run on (`algorithms/sqil.py:42,77-83`; the reference's tutorial
`docs/tutorials/8a_train_sqil_sac.ipynb` and its SQIL tests use it): `SAC`, `SACPolicy` ("MlpPolicy") and `Actor` -- a
restatement of stable-baselines3 2.2.x from its documented behaviour ([SB3 sac/sac.py, sac/policies.py,
common/distributions.py SquashedDiagGaussianDistribution]). SB3 is installed nowhere this project runs: PARITY UNPINNED, like
`td3.py` and `dqn.py`; what is pinned is the agreement with the torch restatement `tests/sac_ref.py`.

Layout, as for `td3.py` (DESIGN sections 2 and 4.12): the host makes every random decision with SB3's call sequence -- row
indices from NumPy's GLOBAL stream, the Gaussian `eps` of the squashed policy from torch's GLOBAL CPU generator with the call
and shape `Normal.rsample` uses on a [B, A] float32 tensor (two draws per gradient step: observations, then next observations;
one [n_envs, A] draw per environment step in the policy branch). A `train` call draws the rows of all its steps, then the
`eps` of all its steps, uploads both once, enqueues every step (`SACPolicy.update`: no host synchronisation and no ATen
operator inside the loop) and reads back one block {critic_loss, actor_loss, ent_coef, ent_coef_loss} per step.
`log_ent_coef` and its Adam moments live on the device; alpha never crosses to the host inside a call. The networks run on the
fp32 MFMA stacks (`ia_mlp_forward` / `ia_mlp_backward`), the minibatch is `ia_td3_assemble`'s, the step around them is
csrc/sac.hip. The actor's two heads `mu` and `log_std` lie as ONE [2A, H] layer in the flat buffer, so one stack call yields
[mu | log_std]; `state_dict` and `parameters()` present SB3's names, shapes and order. The ring stores the SCALED action.

Not implemented (each raises `NotImplementedError`): gSDE (`use_sde`, `sde_*`), `CnnPolicy` / `MultiInputPolicy`,
`share_features_extractor=True`, optimisers other than Adam, tensorboard, `optimize_memory_usage`.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch as th
from torch import nn

from imitation_amd import _lib as L
from imitation_amd.networks import require_device
from imitation_amd.off_policy import _Table
from imitation_amd.policies import FlattenExtractor
from imitation_amd.td3 import (ContinuousCritic, ContinuousOffPolicyAlgorithm, ContinuousPolicy, _check_spaces, _Holder,
                               _Stack, create_mlp)

LOG_STD_MAX, LOG_STD_MIN = 2, -20   # [SB3 sac/policies.py]


def draw_eps(n: int, act_dim: int) -> th.Tensor:
    """Standard normal float32 [n, A] from torch's global CPU generator: `Normal.rsample`'s own call
    (`torch.distributions.utils._standard_normal`), what `ActorCriticPolicy.sample_noise` draws PPO's rollout noise with."""
    return th.distributions.utils._standard_normal((n, act_dim), dtype=th.float32, device="cpu")


class Actor(_Holder):
    """[SB3 sac.policies.Actor]: `latent_pi = create_mlp(features_dim, -1, net_arch, activation_fn)`, then the Linear heads
    `mu` and `log_std` of width A, created in that order. In the flat buffer the two heads are one [2A, H] layer
    ([mu.weight; log_std.weight], then [mu.bias; log_std.bias]); the views below give SB3's names and order."""

    def __init__(self, observation_space, action_space, net_arch: List[int], activation_fn=nn.ReLU):
        _check_spaces(observation_space, action_space, activation_fn)
        self.observation_space, self.action_space = observation_space, action_space
        self.obs_dim, self.act_dim = int(observation_space.shape[0]), int(action_space.shape[0])
        self.net_arch, self.activation_fn = [int(h) for h in net_arch], activation_fn
        act = L.ACT_RELU if activation_fn is nn.ReLU else L.ACT_TANH
        A, last = self.act_dim, (self.net_arch[-1] if self.net_arch else self.obs_dim)
        latent = create_mlp(self.obs_dim, -1, self.net_arch, activation_fn)
        mu, log_std = nn.Linear(last, A), nn.Linear(last, A)
        state = th.get_rng_state()
        head = nn.Linear(last, 2 * A)   # (a container only: the generator stays where SB3's three modules leave it)
        th.set_rng_state(state)
        with th.no_grad():
            head.weight.copy_(th.cat([mu.weight, log_std.weight]))
            head.bias.copy_(th.cat([mu.bias, log_std.bias]))
        seq = nn.Sequential(*latent, head)
        stack = _Stack(seq, "", [self.obs_dim] + self.net_arch + [2 * A], act)
        n_lat = sum(p.numel() for p in latent.parameters())
        # (name, shape, offset into the flat buffer) in SB3's order
        self._views: List[Tuple[str, Tuple[int, ...], int]] = []
        off = 0
        for k, v in latent.state_dict().items():
            self._views.append((f"latent_pi.{k}", tuple(v.shape), off))
            off += v.numel()
        wb = n_lat + 2 * A * last
        self._views += [("mu.weight", (A, last), n_lat), ("mu.bias", (A,), wb),
                        ("log_std.weight", (A, last), n_lat + A * last), ("log_std.bias", (A,), wb + A)]
        stack.names = [(k, shape) for k, shape, _ in self._views]
        self.stacks = [stack]
        self._flat = self._init_flat()

    def sb3_order(self) -> th.Tensor:
        """Indices into the flat buffer in the order of SB3's `parameters()` (the layout of its optimiser's state)."""
        return th.cat([th.arange(off, off + int(np.prod(shape))) for _, shape, off in self._views])

    def parameters(self):
        for _, shape, off in self._views:
            yield self._flat[off:off + int(np.prod(shape))].view(shape)

    def head(self, obs_dev: th.Tensor, hidden: Optional[th.Tensor] = None, out: Optional[th.Tensor] = None) -> th.Tensor:
        """[mu | log_std] [n, 2A] (log_std not yet clamped) of device rows `obs_dev[n, D]`."""
        require_device(self.device)
        n, s = obs_dev.shape[0], self.stacks[0]
        out = th.empty(n, 2 * self.act_dim, device=self.device) if out is None else out
        hidden = th.empty(max(1, n * s.hidden_per_row), device=self.device) if hidden is None else hidden
        L.call("ia_mlp_forward", C.byref(s.desc), L.ptr(self._flat), L.ptr(obs_dev), self.obs_dim, n, L.ptr(hidden),
               L.ptr(out), L.ACT_NONE, L.stream())
        return out

    def action_log_prob(self, obs_dev: th.Tensor, eps_dev: Optional[th.Tensor]) -> Tuple[th.Tensor, th.Tensor]:
        """[SB3 Actor.action_log_prob] on device rows with the given `eps` (None: the deterministic action, whose
        log-probability is that of eps = 0): (a [n, A] in [-1, 1], logp [n])."""
        n, A = obs_dev.shape[0], self.act_dim
        head = self.head(obs_dev)
        a, logp = th.empty(n, A, device=self.device), th.empty(n, device=self.device)
        L.call("ia_sac_sample", L.ptr(head), L.ptr(eps_dev), None, n, 0, A, A, L.ptr(a), L.ptr(logp), None, None, None, None,
               L.stream())
        return a, logp


class SACPolicy(ContinuousPolicy):
    """[SB3 sac.policies.SACPolicy]: `_build` makes the actor, the critic and the critic target (which loads the critic's
    state), in that order; there is no actor target. One Adam over the actor and one over the critic; the entropy
    coefficient and its optimiser belong to the algorithm in SB3 and are set up here by `SAC._setup_model`
    (`setup_ent_coef`), next to the buffers the step kernels read."""

    holders = ("actor", "critic", "critic_target")

    def __init__(self, observation_space, action_space, lr_schedule, net_arch=None, activation_fn=nn.ReLU,
                 use_sde: bool = False, log_std_init: float = -3, use_expln: bool = False, clip_mean: float = 2.0,
                 features_extractor_class=FlattenExtractor, features_extractor_kwargs=None, normalize_images: bool = True,
                 optimizer_class=th.optim.Adam, optimizer_kwargs=None, n_critics: int = 2,
                 share_features_extractor: bool = False):
        if use_sde:
            raise NotImplementedError("gSDE is not implemented")
        super().__init__(observation_space, action_space, lr_schedule, [256, 256] if net_arch is None else net_arch,
                         activation_fn, features_extractor_class, optimizer_class, optimizer_kwargs, n_critics,
                         share_features_extractor)
        # the entropy coefficient: [log_ent_coef, exp_avg, exp_avg_sq, alpha slot] as one device buffer
        self.ent_adam_steps = 0
        self.ent_learned = False
        self.ent_state = th.zeros(4)

    def _build(self, actor_arch: List[int], critic_arch: List[int]) -> None:
        # [SB3 SACPolicy._build]
        space, fn = (self.observation_space, self.action_space), self.activation_fn
        self.actor = Actor(*space, actor_arch, fn)
        self.critic = ContinuousCritic(*space, critic_arch, fn, self.n_critics)
        self.critic_target = ContinuousCritic(*space, critic_arch, fn, self.n_critics)

    def setup_ent_coef(self, learned: bool, init_value: float) -> None:
        """Learned: `log_ent_coef = log(ones(1) * init)` with fresh Adam moments; constant: the slot holds the value."""
        self.ent_learned = bool(learned)
        st = th.zeros(4)
        if learned:
            st[0] = th.log(th.ones(1) * init_value)[0]
            st[3] = th.exp(st[0])
        else:
            st[3] = th.tensor(float(init_value))
        self.ent_state = st.to(self.device)
        self.ent_adam_steps = 0

    @property
    def log_ent_coef(self) -> Optional[th.Tensor]:
        return self.ent_state[0:1] if self.ent_learned else None

    def to(self, device):
        self.ent_state = self.ent_state.to(device)
        return super().to(device)

    def optimizer_state(self) -> Dict[str, th.Tensor]:
        """Adam's moments per optimiser in the order of SB3's `parameters()` (the actor's are gathered out of the fused
        head layout), and the entropy coefficient's when it is learned."""
        na = self.actor.numel()
        order = self.actor.sb3_order().to(self.device)
        out = {"actor.exp_avg": self.exp_avg[:na][order], "actor.exp_avg_sq": self.exp_avg_sq[:na][order],
               "critic.exp_avg": self.exp_avg[na:], "critic.exp_avg_sq": self.exp_avg_sq[na:]}
        if self.ent_learned:
            out.update({"ent_coef.exp_avg": self.ent_state[1:2], "ent_coef.exp_avg_sq": self.ent_state[2:3]})
        return out

    # ---- [SB3 BasePolicy] actions ------------------------------------------------------------------------------------
    def actor_output(self, observation: np.ndarray, deterministic: bool = False) -> np.ndarray:
        """The squashed action of host observations (one upload of [obs], one of eps, one read-back): `tanh(mu)` when
        `deterministic`, else one [n, A] draw from torch's global generator, as [SB3 Actor.forward] makes."""
        obs = np.ascontiguousarray(observation, np.float32).reshape(-1, self.actor.obs_dim)
        require_device(self.device)
        eps = None
        if not deterministic:
            self.last_eps = draw_eps(len(obs), self.actor.act_dim)
            eps = self.last_eps.to(self.device)
        a, _ = self.actor.action_log_prob(th.from_numpy(obs).to(self.device), eps)
        return a.cpu().numpy()

    # ---- the update --------------------------------------------------------------------------------------------------
    def _extra_workspace(self, B: int, e, hid) -> Dict[str, Any]:
        a, nc = self.actor, self.critic.n_critics
        A, ld = a.act_dim, a.obs_dim + a.act_dim
        i8 = lambda *shape: th.zeros(*shape, dtype=th.int8, device=self.device)
        return dict(Xpi=e(B, ld), head=e(B, 2 * A), head2=e(B, 2 * A), dhead=e(B, 2 * A), logp=e(B), logp2=e(B), a=e(B, A),
                    ls=e(B, A), om=e(B, A), bound=i8(B, A), qpi=e(nc, B), seeds=e(nc, B), minq=e(B), argmin_t=i8(B),
                    argmin_pi=i8(B), dX=[e(B, ld) for _ in range(nc)], hid_a2=hid(a.stacks[0]))

    def update(self, ring: Optional[_Table], expert: Optional[_Table], idx_dev: th.Tensor, eps_dev: th.Tensor, n_new: int,
               n_steps: int, batch_size: int, gamma: float, tau: float, target_update_interval: int, target_entropy: float,
               lr: float, stats: th.Tensor, argmin_out: Optional[th.Tensor] = None, step0: int = 0) -> None:
        """`n_steps` gradient steps of [SB3 SAC.train]. `idx_dev` int64 [n_steps, B]; `eps_dev` float32 [n_steps, 2, B, A]
        (observations, next observations); `stats` float32 [n_steps, 4] = {critic_loss, actor_loss, ent_coef,
        ent_coef_loss}, columns 2 and 3 pre-filled by the caller for a constant coefficient; `argmin_out` int8
        [n_steps, 2, B] receives which critic attained the target's and the actor's minimum. Nothing in the loop
        synchronises with the device or calls ATen."""
        a, c, B, st = self.actor, self.critic, int(batch_size), L.stream()
        P, tables, critics_forward, critic_step, actor_step = self._begin_update(ring, expert, B, lr, st)
        D, A, nc, ld, splits = a.obs_dim, a.act_dim, c.n_critics, P["ld"], P["splits"]
        sa, sc = a.stacks[0], c.stacks[0]
        na, ncrit = sa.numel, sc.numel
        call, ref = L.call, C.byref
        hid_c, dX = P["hid_c"], [t.data_ptr() for t in P["dX"]] + [None]
        on_a, on_c, tg_c = self._online.data_ptr(), self._online.data_ptr() + 4 * na, self._target.data_ptr()
        ent = self.ent_state.data_ptr()
        lec, ent_m, ent_v, alpha = ent, ent + 4, ent + 8, ent + 12
        idx_ptr, eps_ptr, stats_ptr = idx_dev.data_ptr(), eps_dev.data_ptr(), stats.data_ptr()
        am_ptr = None if argmin_out is None else argmin_out.data_ptr()
        b1, b2 = float(self.betas[0]), float(self.betas[1])
        for s in range(n_steps):
            eps0, eps1 = eps_ptr + 4 * (2 * s) * B * A, eps_ptr + 4 * (2 * s + 1) * B * A
            am_t, am_pi = (P["argmin_t"], P["argmin_pi"]) if am_ptr is None else (am_ptr + 2 * s * B, am_ptr + (2 * s + 1) * B)
            call("ia_td3_assemble", *tables, idx_ptr + 8 * s * B, B, int(n_new), D, A, ld, P["X"], P["S"], P["S2"], P["rew"],
                 P["done"], st)
            # a_pi, logp = actor.action_log_prob(obs): [obs | a_pi] is the critics' input of the actor loss
            call("ia_mlp_forward", ref(sa.desc), on_a, P["S"], D, B, P["hid_a"], P["head"], L.ACT_NONE, st)
            call("ia_sac_sample", P["head"], eps0, P["S"], B, D, A, ld, P["Xpi"], P["logp"], P["a"], P["ls"], P["om"],
                 P["bound"], st)
            if self.ent_learned:   # alpha as it stands into the slot, then the coefficient's own Adam step
                self.ent_adam_steps += 1
                step_size, bc2 = self._adam_scalars(lr, self.ent_adam_steps)
                call("ia_sac_alpha_step", P["logp"], B, float(target_entropy), lec, ent_m, ent_v, b1, b2, self.eps, step_size,
                     bc2, alpha, stats_ptr + 16 * s + 8, st)
            # target: y = r + (1 - d) gamma (min_i Qt_i(s', a') - alpha logp')
            call("ia_mlp_forward", ref(sa.desc), on_a, P["S2"], D, B, P["hid_a2"], P["head2"], L.ACT_NONE, st)
            call("ia_sac_sample", P["head2"], eps1, P["S2"], B, D, A, ld, P["X2"], P["logp2"], None, None, None, None, st)
            critics_forward(tg_c, P["X2"], P["qt"])
            critics_forward(on_c, P["X"], P["q"])
            call("ia_sac_critic_loss", P["q"], P["qt"], P["logp2"], P["rew"], P["done"], alpha, B, nc, float(gamma), P["dq"],
                 None, am_t, stats_ptr + 16 * s, st)
            critic_step()
            # actor: loss = mean(alpha logp - min_i Q_i(s, a_pi)) with the updated critic
            critics_forward(on_c, P["Xpi"], P["qpi"])
            call("ia_sac_min_seed", P["qpi"], B, nc, P["seeds"], P["minq"], am_pi, st)
            for i in range(nc):
                call("ia_mlp_backward", ref(sc.desc), on_c + 4 * i * ncrit, P["Xpi"], ld, B, hid_c[i], P["seeds"] + 4 * i * B,
                     P["dhid_c"], P["scratch_c"], splits, dX[i], st)
            call("ia_sac_actor_seed", dX[0], dX[1] if nc == 2 else None, ld, D, P["a"], P["om"], eps0, P["ls"], P["bound"],
                 alpha, P["logp"], P["minq"], B, A, P["dhead"], stats_ptr + 16 * s + 4, st)
            actor_step(P["dhead"])
            # [SB3 SAC.train]: the step's index within the call (`step0`: this call's first step within a `train` call split)
            if (step0 + s) % target_update_interval == 0:
                call("ia_polyak_update", on_c, tg_c, nc * ncrit, float(tau), st)


MlpPolicy = SACPolicy


class SAC(ContinuousOffPolicyAlgorithm):
    """[SB3 sac.SAC]."""

    policy_aliases = {"MlpPolicy": SACPolicy}

    def __init__(self, policy, env, learning_rate=3e-4, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, train_freq=1, gradient_steps: int = 1,
                 action_noise=None, replay_buffer_class=None, replay_buffer_kwargs: Optional[Dict[str, Any]] = None,
                 optimize_memory_usage: bool = False, ent_coef="auto", target_update_interval: int = 1,
                 target_entropy="auto", use_sde: bool = False, sde_sample_freq: int = -1, use_sde_at_warmup: bool = False,
                 stats_window_size: int = 100, tensorboard_log=None, policy_kwargs: Optional[Dict[str, Any]] = None,
                 verbose: int = 0, seed: Optional[int] = None, device="auto", _init_setup_model: bool = True):
        if use_sde or sde_sample_freq != -1 or use_sde_at_warmup:
            raise NotImplementedError("gSDE is not implemented")
        if isinstance(policy, str) and policy not in self.policy_aliases:
            raise NotImplementedError(f"policy {policy!r}: only 'MlpPolicy' is implemented for SAC "
                                      "(no CNN or multi-input extractor)")
        if isinstance(ent_coef, str):
            if not ent_coef.startswith("auto"):
                raise ValueError(f"ent_coef {ent_coef!r}: a float, 'auto' or 'auto_<initial value>'")
            init = float(ent_coef.split("_")[1]) if "_" in ent_coef else 1.0
            assert init > 0.0, "The initial value of ent_coef must be greater than 0"
        self.ent_coef, self.target_update_interval, self.target_entropy = ent_coef, target_update_interval, target_entropy
        super().__init__(policy=policy, env=env, learning_rate=learning_rate, buffer_size=buffer_size,
                         learning_starts=learning_starts, batch_size=batch_size, tau=tau, gamma=gamma, train_freq=train_freq,
                         gradient_steps=gradient_steps, action_noise=action_noise, replay_buffer_class=replay_buffer_class,
                         replay_buffer_kwargs=replay_buffer_kwargs, optimize_memory_usage=optimize_memory_usage,
                         stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, policy_kwargs=policy_kwargs,
                         verbose=verbose, seed=seed, device=device)
        if _init_setup_model:
            self._setup_model()

    def _bind_policy(self) -> None:
        self.actor, self.critic, self.critic_target = self.policy.actor, self.policy.critic, self.policy.critic_target
        # [SB3 SAC._setup_model]
        if self.target_entropy == "auto":
            self.target_entropy = float(-np.prod(self.action_space.shape).astype(np.float32))
        else:
            self.target_entropy = float(self.target_entropy)
        if isinstance(self.ent_coef, str):
            init = float(self.ent_coef.split("_")[1]) if "_" in self.ent_coef else 1.0
            self.policy.setup_ent_coef(True, init)
        else:
            self.policy.setup_ent_coef(False, float(self.ent_coef))

    @property
    def log_ent_coef(self) -> Optional[th.Tensor]:
        return self.policy.log_ent_coef

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "SAC",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return super().learn(total_timesteps, callback, log_interval, tb_log_name, reset_num_timesteps, progress_bar)

    def draw_eps(self, gradient_steps: int, batch_size: int) -> th.Tensor:
        """The Gaussian noise of `gradient_steps` steps, float32 [steps, 2, B, A], from torch's global CPU generator: per
        step `Normal.rsample`'s own call on a [B, A] float32 tensor for the observations, then for the next observations,
        so the generator ends where SB3's does (one draw of the whole block would not: torch fills a tensor in pieces whose
        boundaries depend on its size)."""
        A = self.policy.actor.act_dim
        out = th.empty(gradient_steps, 2, batch_size, A)
        for s in range(gradient_steps):
            out[s, 0] = draw_eps(batch_size, A)
            out[s, 1] = draw_eps(batch_size, A)
        return out

    def train(self, gradient_steps: int, batch_size: int = 64) -> None:
        """[SB3 SAC.train]: the index draws of all `gradient_steps` minibatches (NumPy's global stream), then the `eps` of all
        of them (torch's global generator) -- the two streams are independent, so each ends where SB3's interleaved draws
        leave it -- one upload of each, the steps, one read-back."""
        lr, rows, n_new, idx_dev = self._begin_train(gradient_steps, batch_size)
        self.last_eps = eps = self.draw_eps(gradient_steps, batch_size)
        eps_dev = eps.to(self.device)
        learned = self.policy.ent_learned
        init = np.full((gradient_steps, 4), np.nan, np.float32)
        if not learned:
            init[:, 2] = np.float32(self.ent_coef)
        stats = th.from_numpy(init).to(self.device)
        argmin = th.zeros(gradient_steps, 2, batch_size, dtype=th.int8, device=self.device)
        self._run_updates(rows, idx_dev, lambda lo, hi: self.policy.update(
            self.replay_buffer.table, self.replay_buffer.expert_table(), idx_dev[lo:hi], eps_dev[lo:hi], n_new, hi - lo,
            batch_size, self.gamma, self.tau, self.target_update_interval, self.target_entropy, lr, stats[lo:hi],
            argmin[lo:hi], step0=lo))
        both = th.cat([stats.reshape(-1), argmin.reshape(-1).to(th.float32)]).cpu().numpy()   # ONE read-back
        self.last_train_stats = both[:gradient_steps * 4].reshape(gradient_steps, 4)
        self.last_argmin = both[gradient_steps * 4:].astype(np.int8).reshape(gradient_steps, 2, batch_size)
        self._n_updates += gradient_steps
        f64 = self.last_train_stats.astype(np.float64)
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        self.logger.record("train/ent_coef", np.mean(f64[:, 2]))
        self.logger.record("train/actor_loss", np.mean(f64[:, 1]))
        self.logger.record("train/critic_loss", np.mean(f64[:, 0]))
        if learned:
            self.logger.record("train/ent_coef_loss", np.mean(f64[:, 3]))
