"""CPU restatement (torch) of stable-baselines3 2.2.x's SAC -- `SquashedDiagGaussianDistribution`, `Actor`, `SACPolicy`, `SAC` --
written from SB3's documented behaviour ([SB3 sac/sac.py, sac/policies.py, common/distributions.py]) on top of
`tests/td3_ref.py` (critic, off-policy loop with action scaling and noise), `tests/sqil_ref.py` and `oracle/sb3_restated.py`.
SB3 itself is not installed anywhere this project runs: PARITY UNPINNED.

As in `td3_ref`, a class-level `dtype` switch runs the same code in float32 or float64. Parameters are initialised in float32
either way and the Gaussian `eps` is drawn in float32 with `Normal.rsample`'s own call and widened, so both runs consume
torch's generator alike and see the same noise. `SAC.train_log` records per gradient step: `eps` [2, B, A] (observations, next
observations), alpha, the three losses (`ent_coef_loss` None for a constant coefficient), the argmin of both `min` operations,
the Q-values those minima were taken over, the sampled dones and whether the target was updated; `SAC.action_log` as in
`td3_ref`, `SAC.act_eps_log` the `eps` of every environment step in the policy branch.
"""
from __future__ import annotations

import sys
import types
from typing import List, Optional

import numpy as np
import torch as th
from torch import nn
from torch.nn import functional as F

from oracle import sb3_restated as sb
from tests import td3_ref
from tests.sqil_ref import polyak_update
from tests.td3_ref import (ContinuousCritic, NormalActionNoise, VectorizedActionNoise, get_actor_critic_arch)  # noqa: F401

LOG_STD_MAX, LOG_STD_MIN = 2, -20


def standard_normal(shape) -> th.Tensor:
    """What `Normal.rsample` draws: float32 whatever the run's precision."""
    return th.distributions.utils._standard_normal(tuple(shape), dtype=th.float32, device="cpu")


class SquashedDiagGaussianDistribution:
    """[SB3 distributions.SquashedDiagGaussianDistribution] with `epsilon = 1e-6`."""

    def __init__(self, action_dim: int, epsilon: float = 1e-6):
        self.action_dim, self.epsilon = action_dim, epsilon
        self.last_eps: Optional[th.Tensor] = None

    def proba_distribution(self, mean_actions: th.Tensor, log_std: th.Tensor):
        self.distribution = th.distributions.Normal(mean_actions, log_std.exp())
        return self

    def sample(self) -> th.Tensor:
        d = self.distribution
        self.last_eps = standard_normal(d.loc.shape)   # Normal.rsample: loc + eps * scale
        self.gaussian_actions = d.loc + self.last_eps.to(d.loc.dtype) * d.scale
        return th.tanh(self.gaussian_actions)

    def mode(self) -> th.Tensor:
        self.gaussian_actions = self.distribution.mean
        return th.tanh(self.gaussian_actions)

    def log_prob(self, actions: th.Tensor, gaussian_actions: th.Tensor) -> th.Tensor:
        log_prob = self.distribution.log_prob(gaussian_actions).sum(dim=1)
        log_prob -= th.sum(th.log(1 - actions ** 2 + self.epsilon), dim=1)
        return log_prob

    def log_prob_from_params(self, mean_actions: th.Tensor, log_std: th.Tensor):
        self.proba_distribution(mean_actions, log_std)
        actions = self.sample()
        return actions, self.log_prob(actions, self.gaussian_actions)


class Actor(td3_ref._SquashingPolicy):
    def __init__(self, observation_space, action_space, net_arch, features_extractor, features_dim,
                 activation_fn=nn.ReLU, normalize_images: bool = True):
        super().__init__(observation_space, action_space, normalize_images=normalize_images, squash_output=True)
        self.features_extractor, self.features_dim = features_extractor, features_dim
        self.net_arch, self.activation_fn = net_arch, activation_fn
        action_dim = int(np.prod(action_space.shape))
        latent: List[nn.Module] = []   # [SB3 create_mlp(features_dim, -1, net_arch, activation_fn)]: no output layer
        last = features_dim
        for h in net_arch:
            latent += [nn.Linear(last, h), activation_fn()]
            last = h
        self.latent_pi = nn.Sequential(*latent)
        self.action_dist = SquashedDiagGaussianDistribution(action_dim)
        self.mu = nn.Linear(last, action_dim)
        self.log_std = nn.Linear(last, action_dim)

    def get_action_dist_params(self, obs: th.Tensor):
        features = self.extract_features(obs, self.features_extractor).to(self.mu.weight.dtype)
        latent_pi = self.latent_pi(features)
        return self.mu(latent_pi), th.clamp(self.log_std(latent_pi), LOG_STD_MIN, LOG_STD_MAX)

    def forward(self, obs: th.Tensor, deterministic: bool = False) -> th.Tensor:
        mean_actions, log_std = self.get_action_dist_params(obs)
        self.action_dist.proba_distribution(mean_actions, log_std)
        return self.action_dist.mode() if deterministic else self.action_dist.sample()

    def action_log_prob(self, obs: th.Tensor):
        mean_actions, log_std = self.get_action_dist_params(obs)
        return self.action_dist.log_prob_from_params(mean_actions, log_std)

    def _predict(self, observation: th.Tensor, deterministic: bool = False) -> th.Tensor:
        return self(observation, deterministic)


class SACPolicy(td3_ref._SquashingPolicy, sb.SACPolicy):
    def __init__(self, observation_space, action_space, lr_schedule, net_arch=None, activation_fn=nn.ReLU,
                 use_sde: bool = False, log_std_init: float = -3, use_expln: bool = False, clip_mean: float = 2.0,
                 features_extractor_class=sb.FlattenExtractor, features_extractor_kwargs=None, normalize_images: bool = True,
                 optimizer_class=th.optim.Adam, optimizer_kwargs=None, n_critics: int = 2,
                 share_features_extractor: bool = False):
        super().__init__(observation_space, action_space, features_extractor_class, features_extractor_kwargs,
                         optimizer_class=optimizer_class, optimizer_kwargs=optimizer_kwargs, squash_output=True,
                         normalize_images=normalize_images)
        assert not use_sde and not share_features_extractor
        if net_arch is None:
            net_arch = [256, 256]
        self.net_arch, self.activation_fn, self.n_critics = net_arch, activation_fn, n_critics
        self.actor_arch, self.critic_arch = get_actor_critic_arch(net_arch)
        self._build(lr_schedule)

    def _build(self, lr_schedule) -> None:
        self.actor = self.make_actor()
        self.actor.optimizer = self.optimizer_class(self.actor.parameters(), lr=lr_schedule(1), **self.optimizer_kwargs)
        self.critic = self.make_critic()
        self.critic.optimizer = self.optimizer_class(self.critic.parameters(), lr=lr_schedule(1), **self.optimizer_kwargs)
        self.critic_target = self.make_critic()
        self.critic_target.load_state_dict(self.critic.state_dict())
        self.critic_target.set_training_mode(False)

    def make_actor(self) -> Actor:
        fe = self.make_features_extractor()
        return Actor(self.observation_space, self.action_space, self.actor_arch, fe, fe.features_dim, self.activation_fn,
                     self.normalize_images)

    def make_critic(self) -> ContinuousCritic:
        fe = self.make_features_extractor()
        return ContinuousCritic(self.observation_space, self.action_space, self.critic_arch, fe, fe.features_dim,
                                self.activation_fn, self.normalize_images, self.n_critics)

    def forward(self, obs: th.Tensor, deterministic: bool = False) -> th.Tensor:
        return self._predict(obs, deterministic=deterministic)

    def _predict(self, observation: th.Tensor, deterministic: bool = False) -> th.Tensor:
        return self.actor(observation, deterministic)

    def set_training_mode(self, mode: bool) -> None:
        self.actor.set_training_mode(mode)
        self.critic.set_training_mode(mode)
        self.training = mode


MlpPolicy = SACPolicy


class SAC(td3_ref.OffPolicyAlgorithm):
    """[SB3 sac/sac.py]. `dtype`: the precision the networks, the entropy coefficient, their optimisers and the update run in."""

    policy_aliases = {"MlpPolicy": SACPolicy}
    dtype = th.float32

    def __init__(self, policy, env, learning_rate=3e-4, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, train_freq=1, gradient_steps: int = 1,
                 action_noise=None, replay_buffer_class=None, replay_buffer_kwargs=None, optimize_memory_usage: bool = False,
                 ent_coef="auto", target_update_interval: int = 1, target_entropy="auto", use_sde: bool = False,
                 sde_sample_freq: int = -1, use_sde_at_warmup: bool = False, stats_window_size: int = 100, policy_kwargs=None,
                 verbose: int = 0, seed: Optional[int] = None, device="cpu", _init_setup_model: bool = True):
        if isinstance(policy, str):
            policy = self.policy_aliases[policy]
        assert not use_sde
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma,
                         train_freq=train_freq, gradient_steps=gradient_steps, action_noise=action_noise,
                         replay_buffer_class=replay_buffer_class, replay_buffer_kwargs=replay_buffer_kwargs,
                         optimize_memory_usage=optimize_memory_usage, policy_kwargs=policy_kwargs,
                         stats_window_size=stats_window_size, verbose=verbose, device=device, seed=seed)
        self.target_entropy, self.ent_coef, self.target_update_interval = target_entropy, ent_coef, target_update_interval
        self.log_ent_coef = None
        self.ent_coef_optimizer = None
        self.action_log: List[tuple] = []
        self.act_eps_log: List[np.ndarray] = []
        self.train_log: List[dict] = []
        if _init_setup_model:
            self._setup_model()

    def _setup_model(self) -> None:
        super()._setup_model()
        if self.dtype is not th.float32:   # after the float32 initialisation: same draws from torch's generator
            self.policy.to(self.dtype)
            for net in (self.policy.actor, self.policy.critic):
                net.optimizer = self.policy.optimizer_class(net.parameters(), lr=self.lr_schedule(1),
                                                            **self.policy.optimizer_kwargs)
        self.actor, self.critic, self.critic_target = self.policy.actor, self.policy.critic, self.policy.critic_target
        if self.target_entropy == "auto":
            self.target_entropy = float(-np.prod(self.env.action_space.shape).astype(np.float32))
        else:
            self.target_entropy = float(self.target_entropy)
        if isinstance(self.ent_coef, str) and self.ent_coef.startswith("auto"):
            init_value = 1.0
            if "_" in self.ent_coef:
                init_value = float(self.ent_coef.split("_")[1])
                assert init_value > 0.0, "The initial value of ent_coef must be greater than 0"
            self.log_ent_coef = th.log(th.ones(1) * init_value).to(self.dtype).requires_grad_(True)
            self.ent_coef_optimizer = th.optim.Adam([self.log_ent_coef], lr=self.lr_schedule(1))
        else:
            self.ent_coef_tensor = th.tensor(float(self.ent_coef)).to(self.dtype)

    def _note_action(self, branch: str, action, buffer_action=None) -> None:
        self.action_log.append((branch, np.array(action), np.array(buffer_action)))
        if branch == "policy":
            self.act_eps_log.append(self.actor.action_dist.last_eps.numpy().copy())

    def _update_learning_rate(self, optimizers) -> None:
        lr = self.lr_schedule(self._current_progress_remaining)
        self.logger.record("train/learning_rate", lr)
        for optimizer in optimizers:
            for group in optimizer.param_groups:
                group["lr"] = lr

    def train(self, gradient_steps: int, batch_size: int = 64) -> None:
        self.policy.set_training_mode(True)
        optimizers = [self.actor.optimizer, self.critic.optimizer]
        if self.ent_coef_optimizer is not None:
            optimizers += [self.ent_coef_optimizer]
        self._update_learning_rate(optimizers)
        ent_coef_losses, ent_coefs, actor_losses, critic_losses = [], [], [], []
        dist = self.actor.action_dist
        for gradient_step in range(gradient_steps):
            replay_data = self.replay_buffer.sample(batch_size, env=self._vec_normalize_env)
            observations = replay_data.observations.to(self.dtype)
            next_observations = replay_data.next_observations.to(self.dtype)
            rewards, dones = replay_data.rewards.to(self.dtype), replay_data.dones.to(self.dtype)
            actions_pi, log_prob = self.actor.action_log_prob(observations)
            eps_obs = dist.last_eps.numpy().copy()
            log_prob = log_prob.reshape(-1, 1)
            ent_coef_loss = None
            if self.ent_coef_optimizer is not None and self.log_ent_coef is not None:
                ent_coef = th.exp(self.log_ent_coef.detach())
                ent_coef_loss = -(self.log_ent_coef * (log_prob + self.target_entropy).detach()).mean()
                ent_coef_losses.append(ent_coef_loss.item())
            else:
                ent_coef = self.ent_coef_tensor
            ent_coefs.append(ent_coef.item())
            if ent_coef_loss is not None and self.ent_coef_optimizer is not None:
                self.ent_coef_optimizer.zero_grad()
                ent_coef_loss.backward()
                self.ent_coef_optimizer.step()
            with th.no_grad():
                next_actions, next_log_prob = self.actor.action_log_prob(next_observations)
                eps_next = dist.last_eps.numpy().copy()
                next_q_all = th.cat(self.critic_target(next_observations, next_actions), dim=1)
                next_q_values, argmin_target = th.min(next_q_all, dim=1, keepdim=True)
                next_q_values = next_q_values - ent_coef * next_log_prob.reshape(-1, 1)
                target_q_values = rewards + (1 - dones) * self.gamma * next_q_values
            current_q_values = self.critic(observations, replay_data.actions)
            critic_loss = 0.5 * sum(F.mse_loss(current_q, target_q_values) for current_q in current_q_values)
            critic_losses.append(critic_loss.item())
            self.critic.optimizer.zero_grad()
            critic_loss.backward()
            self.critic.optimizer.step()
            q_values_pi = th.cat(self.critic(observations, actions_pi), dim=1)
            min_qf_pi, argmin_pi = th.min(q_values_pi, dim=1, keepdim=True)
            actor_loss = (ent_coef * log_prob - min_qf_pi).mean()
            actor_losses.append(actor_loss.item())
            self.actor.optimizer.zero_grad()
            actor_loss.backward()
            self.actor.optimizer.step()
            updated = gradient_step % self.target_update_interval == 0
            if updated:
                polyak_update(self.critic.parameters(), self.critic_target.parameters(), self.tau)
            self.train_log.append(dict(
                n_updates=self._n_updates + gradient_step + 1, lr=self.critic.optimizer.param_groups[0]["lr"],
                eps=np.stack([eps_obs, eps_next]), ent_coef=ent_coefs[-1], critic_loss=critic_losses[-1],
                actor_loss=actor_losses[-1], ent_coef_loss=None if ent_coef_loss is None else ent_coef_losses[-1],
                argmin_target=argmin_target.reshape(-1).numpy().astype(np.int8),
                argmin_pi=argmin_pi.reshape(-1).numpy().astype(np.int8),
                q_target=next_q_all.detach().numpy().astype(np.float64), q_pi=q_values_pi.detach().numpy().astype(np.float64),
                dones=dones.numpy().reshape(-1).copy(), target_updated=bool(updated)))
        self._n_updates += gradient_steps
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        self.logger.record("train/ent_coef", np.mean(ent_coefs))
        self.logger.record("train/actor_loss", np.mean(actor_losses))
        self.logger.record("train/critic_loss", np.mean(critic_losses))
        if len(ent_coef_losses) > 0:
            self.logger.record("train/ent_coef_loss", np.mean(ent_coef_losses))


def install_sb3_modules() -> None:
    """`td3_ref.install_sb3_modules()` plus `stable_baselines3.sac` (with `.policies`) from this restatement (in the calling
    process only)."""
    td3_ref.install_sb3_modules()
    me = sys.modules[__name__]
    root = sys.modules["stable_baselines3"]
    pol = types.ModuleType("stable_baselines3.sac.policies")
    pol.__dict__.update(SACPolicy=SACPolicy, MlpPolicy=MlpPolicy, Actor=Actor)
    m = types.ModuleType("stable_baselines3.sac")
    m.__dict__.update(SAC=SAC, SACPolicy=SACPolicy, MlpPolicy=MlpPolicy, policies=pol)
    for mod in (m, pol):
        mod._restated_in = me.__name__
        sys.modules[mod.__name__] = mod
    root.sac = m
    root.SAC = SAC
