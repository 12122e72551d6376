"""What the fixtures of GAIL with an off-policy generator (`tests/golden/make_golden_gail_offpolicy.py`) and their tests
share: the cases, the environment, the demonstrations and the seeding of a run, the taps that note what a run does (the same
instance-level wrappers on the reference's trainer and on this package's), and `run_case`, which runs THIS package's `GAIL`
on a case. `python -m tests.gail_offpolicy_golden CASE SEED OUT.npz` writes one such record (the tests use it to run a case
in a fresh process with `IA_OFFPOLICY_FUSED=0`)."""
import sys

import numpy as np

from imitation_amd.vec_env import SyntheticVecEnv

GAP_MARGIN = 1e-3
BRANCH = {"warmup": 0, "explore": 1, "greedy": 2, "policy": 3}
NOT_COMPARED_PREFIX = "time/"   # wall-clock values of a dump (also under `mean/gen/`, `raw/gen/`)

COMMON = dict(n_envs=4, horizon=8, rounds=3, gen_train_timesteps=32, demo_batch_size=16, n_disc=2, n_demo=48,
              buffer_size=64, learning_starts=20, train_freq=4, target_update_interval=16, learning_rate=1e-3, gamma=0.99,
              batch_size=8, net_arch=[32, 32], flags=[True, True, False, False])
CASES = {
    "gail_dqn": dict(algo="DQN", obs_dim=4, n_actions=2, exploration_fraction=0.5, exploration_final_eps=0.05),
    "gail_dqn_next_done": dict(algo="DQN", obs_dim=4, n_actions=2, exploration_fraction=0.5, exploration_final_eps=0.05,
                               flags=[True, True, True, True]),
    # (bounds other than [-1, 1]: the action the ring keeps -- SB3's scaled action -- differs from the environment's)
    # ([16, 16] towers: the six nets of a TD3 policy in two precisions would not fit the fixture otherwise)
    "gail_td3": dict(algo="TD3", obs_dim=5, act_dim=2, gradient_steps=2, low=-2.0, high=3.0, action_noise=0.1,
                     net_arch=[16, 16]),
}
EXACT_DQN = ("ring_obs", "ring_next_obs", "ring_action", "actions", "gen_obs", "gen_acts", "gen_next_obs")


def is_exact(cfg, key):
    """Keys every implementation must reproduce bit for bit: all index and branch records, and for Discrete actions the
    rows themselves (every decision there is an arg-max the fixtures' seeds keep away from ties). With Box actions the rows
    follow the actor's float32 output, which no two implementations round alike: they are float keys."""
    return cfg["algo"] == "DQN" and key in EXACT_DQN


def pool_params(rec):
    """The final parameters of a record as float keys: one per tensor (`final/<name>` for the learner's nets,
    `disc_final/<name>` for the discriminator's stack), except that a ONE-element tensor is keyed together with the weight
    of its layer (`...dense_final` = [weight | bias], `...qf0.4` likewise), and the input norm's statistics as
    `disc_norm/running_mean`, `disc_norm/running_var` (the integer `disc_norm_count` is an exact key). A relative deviation
    needs a norm to stand on: over eight seeds the reference's own float32-to-float64 deviation of the discriminator's
    one-element output bias alone lay anywhere between 7e-10 and 2.5e-7 (its value between 0.0009 and 0.16)."""
    out = {k: v for k, v in rec.items() if not k.startswith(("final/", "disc_final/"))}
    for prefix in ("final/", "disc_final/"):
        items = [(k, np.asarray(v)) for k, v in rec.items() if k.startswith(prefix)]
        names = dict(items)
        for k, v in items:
            if "normalize_input" in k:
                if k.endswith("count"):
                    out["disc_norm_count"] = np.int64(v.round())
                else:
                    out["disc_norm/" + k.rsplit(".", 1)[1]] = v.astype(np.float64)
            elif k.endswith(".bias") and v.size == 1:
                continue   # (keyed with its weight, below)
            elif k.endswith(".weight") and names.get(k[:-len("weight")] + "bias", np.zeros(2)).size == 1:
                out[k[:-len(".weight")]] = np.concatenate([v.reshape(-1), names[k[:-len("weight")] + "bias"].reshape(-1)]
                                                          ).astype(np.float64)
            else:
                out[k] = v.astype(np.float64)
    return out


def make_env(cfg, seed):
    if cfg["algo"] == "DQN":
        return SyntheticVecEnv(num_envs=cfg["n_envs"], obs_dim=cfg["obs_dim"], act_dim=2, horizon=cfg["horizon"],
                               seed=100 + seed, n_discrete=cfg["n_actions"], prefetch_noise=False)
    from tests.td3_golden import BoundsWrapper
    venv = SyntheticVecEnv(num_envs=cfg["n_envs"], obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], horizon=cfg["horizon"],
                           seed=100 + seed, prefetch_noise=False)
    return BoundsWrapper(venv, cfg["low"], cfg["high"])


def make_demos(cfg, seed):
    """Plain arrays (the caller wraps them in its own `Transitions`): obs, acts, next_obs, dones."""
    r = np.random.default_rng(500 + seed)
    n, D = cfg["n_demo"], cfg["obs_dim"]
    obs = r.normal(size=(n, D)).astype(np.float32)
    nxt = (0.9 * obs + 0.1 * r.normal(size=(n, D))).astype(np.float32)
    if cfg["algo"] == "DQN":
        acts = r.integers(0, cfg["n_actions"], size=n).astype(np.int64)
    else:
        acts = r.uniform(cfg["low"], cfg["high"], size=(n, cfg["act_dim"])).astype(np.float32)
    dones = np.zeros(n, bool)
    dones[cfg["horizon"] - 1::cfg["horizon"]] = True
    return obs, acts, nxt, dones


def rl_kwargs_of(cfg, noise_cls=None):
    kw = dict(learning_rate=cfg["learning_rate"], buffer_size=cfg["buffer_size"], learning_starts=cfg["learning_starts"],
              batch_size=cfg["batch_size"], gamma=cfg["gamma"], train_freq=cfg["train_freq"],
              policy_kwargs=dict(net_arch=list(cfg["net_arch"])))
    if cfg["algo"] == "DQN":
        kw.update(target_update_interval=cfg["target_update_interval"], exploration_fraction=cfg["exploration_fraction"],
                  exploration_final_eps=cfg["exploration_final_eps"])
    else:
        kw.update(gradient_steps=cfg["gradient_steps"])
        if cfg.get("action_noise"):
            A = cfg["act_dim"]
            kw["action_noise"] = noise_cls(np.zeros(A), cfg["action_noise"] * np.ones(A))
    return kw


def seed_everything(venv, seed):
    import torch as th
    th.manual_seed(seed)
    np.random.seed(seed + 1)
    venv.action_space.seed(seed + 2)


class Tap:
    """Instance-level wrappers on a trainer (the reference's or this package's; the code under test is untouched) that
    note every learner-ring write, every logger dump and, at each round's end, the rewards the round's writes left in the
    learner ring and the trainer's own replay ring."""

    def __init__(self, trainer, cfg, learner_rewards, gen_ring):
        self.trainer, self.cfg, self.rl = trainer, cfg, trainer.gen_algo
        self.learner_rewards, self.gen_ring = learner_rewards, gen_ring
        self.adds, self.dumps, self.rounds, self.round_rewards = [], [], [], []
        self._seen = 0
        rb, logger = self.rl.replay_buffer, trainer.logger
        orig_add, orig_dump = rb.add, logger.dump

        def add(obs, next_obs, action, reward, done, infos):
            timeouts = np.array([info.get("TimeLimit.truncated", False) for info in infos], np.float32)
            self.adds.append((rb.pos, np.array(obs, np.float32), np.array(next_obs, np.float32), np.array(action),
                              np.array(done, np.float32), timeouts))
            return orig_add(obs, next_obs, action, reward, done, infos)

        def dump(step=0):
            self.dumps.append((int(step), {k: float(v) for k, v in logger.name_to_value.items()}))
            return orig_dump(step)

        rb.add, logger.dump = add, dump

    def end_of_round(self, r):
        rew = self.learner_rewards()   # [positions, n_envs]
        self.round_rewards += [rew[a[0]].copy() for a in self.adds[self._seen:]]
        self._seen = len(self.adds)
        self.rounds.append(self.gen_ring())

    def record(self):
        n = self.cfg["n_envs"]
        out = dict(ring_pos=np.array([a[0] for a in self.adds], np.int64), ring_obs=np.stack([a[1] for a in self.adds]),
                   ring_next_obs=np.stack([a[2] for a in self.adds]),
                   ring_action=np.stack([a[3].reshape(n, -1) for a in self.adds]),
                   ring_done=np.stack([a[4] for a in self.adds]), ring_timeout=np.stack([a[5] for a in self.adds]),
                   ring_reward=np.stack(self.round_rewards).astype(np.float64), n_dumps=np.int64(len(self.dumps)))
        for k in ("obs", "acts", "next_obs", "dones", "idx", "n_data"):
            out[f"gen_{k}"] = np.stack([np.asarray(g[k]) for g in self.rounds])
        for j, (step, kv) in enumerate(self.dumps):
            keys = sorted(kv)
            out[f"dump{j}_step"] = np.int64(step)
            out[f"dump{j}_keys"] = np.array(keys)
            out[f"dump{j}_vals"] = np.array([kv[k] for k in keys], np.float64)
        return out


class Recorder(Tap):
    """`Tap` plus what this package's learners expose of their decisions (the reference's restated learners log the same
    things themselves)."""

    def __init__(self, trainer, cfg):
        rl = trainer.gen_algo
        n = cfg["n_envs"]
        super().__init__(trainer, cfg,
                         learner_rewards=lambda: rl.replay_buffer.table.reward.cpu().numpy().reshape(-1, n),
                         gen_ring=lambda: dict(trainer._gen_replay_buffer._arrays, idx=trainer._gen_replay_buffer._idx,
                                               n_data=trainer._gen_replay_buffer._n_data))
        self.actions, self.branches, self.eps, self.target_updates = [], [], [], []
        self.rows, self.train_at, self.losses, self.actor_losses = [], [], [], []
        orig = dict(sample=rl._sample_action, on_step=rl._on_step, train=rl.train)

        def sample_action(*a, **k):
            out = orig["sample"](*a, **k)
            self.actions.append(np.array(out[0] if isinstance(out, tuple) else out))
            self.branches.append(BRANCH[rl.last_action_branch])
            return out

        def on_step():
            orig["on_step"]()
            if cfg["algo"] == "DQN":
                self.eps.append(rl.exploration_rate)

        def train(*a, **k):
            before = rl._n_updates
            orig["train"](*a, **k)
            self.rows.append(rl.last_sample_rows.copy())
            steps = len(rl.last_sample_rows)
            # (DQN: the `_n_calls` of the call; TD3: the `_n_updates` of each step, which decides the actor's turn)
            self.train_at += [rl._n_calls] * steps if cfg["algo"] == "DQN" else list(range(before + 1, before + steps + 1))
            self.losses.append(rl.last_train_stats[:, 0].copy())
            if cfg["algo"] != "DQN":
                self.actor_losses.append(rl.last_train_stats[np.array(rl.last_actor_steps, bool), 1].copy())

        rl._sample_action, rl._on_step, rl.train = sample_action, on_step, train
        self.greedy_q = []
        if cfg["algo"] == "DQN":
            orig_polyak, orig_q = rl.policy.polyak_update, rl.policy.q_values

            def q_values(observation):
                q, am = orig_q(observation)
                self.greedy_q.append(q.copy())
                return q, am

            rl.policy.q_values = q_values

            def polyak(tau):
                self.target_updates.append(rl._n_calls)
                return orig_polyak(tau)

            rl.policy.polyak_update = polyak

    def record(self):
        rl, tr = self.rl, self.trainer
        out = super().record()
        out.update(actions=np.stack(self.actions), branches=np.array(self.branches, np.int64),
                   sample_rows=np.concatenate(self.rows), train_at=np.array(self.train_at, np.int64),
                   loss=np.concatenate(self.losses).astype(np.float64))
        if self.cfg["algo"] == "DQN":
            out.update(exploration_rate=np.array(self.eps, np.float64), target_updates=np.array(self.target_updates, np.int64),
                       greedy_q=np.concatenate(self.greedy_q).astype(np.float64))
        else:
            out["actor_loss"] = np.concatenate(self.actor_losses).astype(np.float64)
        for k, v in dict(num_timesteps=rl.num_timesteps, n_updates=rl._n_updates, episodes=rl._episode_num,
                         pos=rl.replay_buffer.pos, full=int(rl.replay_buffer.full), global_step=tr._global_step,
                         disc_step=tr._disc_step).items():
            out[f"counter/{k}"] = np.int64(v)
        for k, v in rl.policy.state_dict().items():
            out[f"final/{k}"] = v.cpu().numpy().astype(np.float64)
        for k, v in tr._reward_net.state_dict().items():
            out[f"disc_final/{k}"] = v.cpu().numpy().astype(np.float64)
        t = rl.replay_buffer.table   # the learner's ring as it lies in device memory
        for name in ("obs", "next_obs", "action", "reward", "done"):
            out[f"table_{name}"] = getattr(t, name).cpu().numpy()
        src = tr._step_source
        out["step_launches"] = np.int64(-1 if src is None else src.launches)
        out["reward_fn_calls"] = np.int64(tr.venv_wrapped.reward_fn_calls)
        return pool_params(out)


def build(cfg, seed, device="cuda"):
    """This package's GAIL on a case, seeded as the fixture's run was; returns (trainer, recorder)."""
    import tempfile

    import imitation_amd as p

    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = p.Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones)
    seed_everything(venv, seed)
    algo = getattr(p, cfg["algo"])
    rl = algo("MlpPolicy", venv, device=device, **rl_kwargs_of(cfg, p.NormalActionNoise))
    f = cfg["flags"]
    net = p.BasicRewardNet(venv.observation_space, venv.action_space, use_state=f[0], use_action=f[1], use_next_state=f[2],
                           use_done=f[3], normalize_input_layer=p.RunningNorm)
    trainer = p.GAIL(demonstrations=demos, demo_batch_size=cfg["demo_batch_size"], venv=venv, gen_algo=rl, reward_net=net,
                     n_disc_updates_per_round=cfg["n_disc"], gen_train_timesteps=cfg["gen_train_timesteps"],
                     custom_logger=p.configure_logger(tempfile.mkdtemp(), []), allow_variable_horizon=False)
    return trainer, Recorder(trainer, cfg)


def run_case(name, seed, device="cuda"):
    cfg = dict(COMMON, **CASES[name])
    trainer, rec = build(cfg, seed, device)
    init = {f"init/{k}": v.cpu().numpy() for k, v in trainer.gen_algo.policy.state_dict().items()}
    init.update({f"disc_init/{k}": v.cpu().numpy() for k, v in trainer._reward_net.state_dict().items()})
    trainer.train(cfg["rounds"] * cfg["gen_train_timesteps"], callback=rec.end_of_round)
    return dict(rec.record(), **init)


if __name__ == "__main__":
    np.savez(sys.argv[3], **run_case(sys.argv[1], int(sys.argv[2])))
