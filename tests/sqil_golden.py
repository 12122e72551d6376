"""What the SQIL fixtures' generator (`tests/golden/make_golden_sqil.py`) and their tests share: the cases, the
environment, the demonstrations and the seeding of a run, and `run_case`, which runs THIS package's `SQIL` on a case and
records what the fixtures record. `python -m tests.sqil_golden CASE OUT.npz` writes one such record (the tests use it to
run a case in a fresh process with `IA_DQN_FUSED=0`)."""
import sys

import numpy as np

from imitation_amd.vec_env import SyntheticVecEnv

GAP_MARGIN = 1e-3
BRANCH = {"warmup": 0, "explore": 1, "greedy": 2}
NOT_COMPARED = ("time/fps", "time/time_elapsed")   # wall-clock values of a dump

COMMON = dict(n_envs=4, horizon=8, n_demo=24, buffer_size=64, learning_starts=20, train_freq=4, target_update_interval=16,
              total_timesteps=200, learning_rate=1e-3, gamma=0.99, tau=1.0, max_grad_norm=10.0, gradient_steps=1,
              exploration_fraction=0.5, exploration_initial_eps=1.0, exploration_final_eps=0.05, log_interval=4)
CASES = {
    "sqil_cartpole_shape": dict(obs_dim=4, n_actions=2, net_arch=[64, 64], batch_size=8),
    "sqil_odd_batch": dict(obs_dim=5, n_actions=3, net_arch=[32, 32], batch_size=7, gradient_steps=3),
    "sqil_all_random": dict(obs_dim=4, n_actions=2, net_arch=[64, 64], batch_size=8, exploration_initial_eps=1.0,
                            exploration_final_eps=1.0),
    "sqil_general_arch": dict(obs_dim=5, n_actions=3, net_arch=[48], batch_size=8),
}


def make_env(cfg, seed):
    return SyntheticVecEnv(num_envs=cfg["n_envs"], obs_dim=cfg["obs_dim"], act_dim=2, horizon=cfg["horizon"],
                           seed=100 + seed, stagger=True, n_discrete=cfg["n_actions"], prefetch_noise=False)


def make_demos(cfg, seed):
    """Plain arrays (the caller wraps them in its own `Transitions`): obs, acts, next_obs, dones."""
    r = np.random.default_rng(500 + seed)
    n, D = cfg["n_demo"], cfg["obs_dim"]
    obs = r.normal(size=(n, D)).astype(np.float32)
    nxt = (0.9 * obs + 0.1 * r.normal(size=(n, D))).astype(np.float32)
    acts = r.integers(0, cfg["n_actions"], size=n).astype(np.int64)
    dones = r.uniform(size=n) < 0.2
    return obs, acts, nxt, dones


def rl_kwargs_of(cfg):
    return dict(learning_rate=cfg["learning_rate"], buffer_size=cfg["buffer_size"], learning_starts=cfg["learning_starts"],
                batch_size=cfg["batch_size"], tau=cfg["tau"], gamma=cfg["gamma"], train_freq=cfg["train_freq"],
                gradient_steps=cfg["gradient_steps"], target_update_interval=cfg["target_update_interval"],
                exploration_fraction=cfg["exploration_fraction"], exploration_initial_eps=cfg["exploration_initial_eps"],
                exploration_final_eps=cfg["exploration_final_eps"], max_grad_norm=cfg["max_grad_norm"],
                policy_kwargs=dict(net_arch=list(cfg["net_arch"])))


def seed_everything(venv, seed):
    import torch as th
    th.manual_seed(seed)
    np.random.seed(seed + 1)
    venv.action_space.seed(seed + 2)


class Recorder:
    """Hooks on a `SQIL` of this package that note what the fixtures hold (the code under test itself is untouched)."""

    def __init__(self, algo):
        import imitation_amd as p

        self.algo, rl = algo, algo.rl_algo
        self.adds, self.rows, self.actions, self.branches, self.eps = [], [], [], [], []
        self.target_updates, self.train_n_calls, self.train_lr, self.losses, self.greedy_q, self.dumps = [], [], [], [], [], []
        self.logger = p.logger.Logger(None, [])
        rl.set_logger(self.logger)
        rb, pol = rl.replay_buffer, rl.policy
        self.path_calls = {"fused": 0, "general": 0}   # which update path `DQNPolicy.update` actually took
        for path in ("fused", "general"):
            def counted(*a, _path=path, _fn=getattr(pol, "update_" + path), **k):
                self.path_calls[_path] += 1
                return _fn(*a, **k)
            setattr(pol, "update_" + path, counted)
        orig = dict(add=rb.add, sample=rl._sample_action, on_step=rl._on_step, polyak=pol.polyak_update, train=rl.train,
                    q=pol.q_values, dump=self.logger.dump)

        def add(obs, next_obs, action, reward, done, infos):
            self.adds.append((rb.pos, np.array(obs), np.array(next_obs), np.array(action), np.array(done, np.float32)))
            return orig["add"](obs, next_obs, action, reward, done, infos)

        def sample_action(*a, **k):
            out = orig["sample"](*a, **k)
            self.actions.append(np.array(out, np.int64))
            self.branches.append(BRANCH[rl.last_action_branch])
            return out

        def on_step():
            orig["on_step"]()
            self.eps.append(rl.exploration_rate)

        def polyak(tau):
            self.target_updates.append(rl._n_calls)
            return orig["polyak"](tau)

        def train(*a, **k):
            orig["train"](*a, **k)
            steps = len(rl.last_sample_rows)
            self.rows.append(rl.last_sample_rows.copy())
            self.train_n_calls += [rl._n_calls] * steps
            self.train_lr += [self.logger.name_to_value["train/learning_rate"]] * steps
            self.losses.append(rl.last_train_stats[:, 0].copy())

        def q_values(observation):
            q, am = orig["q"](observation)
            self.greedy_q.append(q.copy())
            return q, am

        def dump(step=0):
            self.dumps.append((int(step), {k: float(v) for k, v in self.logger.name_to_value.items()}))
            return orig["dump"](step)

        rb.add, rl._sample_action, rl._on_step, pol.polyak_update, rl.train = add, sample_action, on_step, polyak, train
        pol.q_values, self.logger.dump = q_values, dump

    def record(self):
        rl = self.algo.rl_algo
        rb = rl.replay_buffer
        out = dict(ring_pos=np.array([a[0] for a in self.adds], np.int64),
                   ring_obs=np.stack([a[1] for a in self.adds]), ring_next_obs=np.stack([a[2] for a in self.adds]),
                   ring_action=np.stack([a[3] for a in self.adds]), ring_done=np.stack([a[4] for a in self.adds]),
                   sample_rows=np.concatenate(self.rows), actions=np.stack(self.actions),
                   branches=np.array(self.branches, np.int64), exploration_rate=np.array(self.eps, np.float64),
                   target_updates=np.array(self.target_updates, np.int64),
                   train_n_calls=np.array(self.train_n_calls, np.int64), train_lr=np.array(self.train_lr, np.float64),
                   loss=np.concatenate(self.losses).astype(np.float64), n_dumps=np.int64(len(self.dumps)),
                   fused_calls=np.int64(self.path_calls["fused"]), general_calls=np.int64(self.path_calls["general"]))
        for name, t in (("obs", rb.table.obs), ("next_obs", rb.table.next_obs), ("action", rb.table.action),
                        ("reward", rb.table.reward), ("done", rb.table.done)):
            out[f"table_{name}"] = t.cpu().numpy()
        if self.greedy_q:
            out["greedy_q"] = np.concatenate(self.greedy_q).astype(np.float64)
        for j, (step, kv) in enumerate(self.dumps):
            keys = sorted(kv)
            out[f"dump{j}_step"] = np.int64(step)
            out[f"dump{j}_keys"] = np.array(keys)
            out[f"dump{j}_vals"] = np.array([kv[k] for k in keys], np.float64)
        for k, v in dict(num_timesteps=rl.num_timesteps, n_updates=rl._n_updates, n_calls=rl._n_calls,
                         episodes=rl._episode_num, pos=rb.pos, full=int(rb.full)).items():
            out[f"counter/{k}"] = np.int64(v)
        for k, v in rl.policy.state_dict().items():
            out[f"final/{k}"] = v.cpu().numpy().astype(np.float64)
        return out


def build(cfg, seed, device="cuda"):
    """This package's SQIL on a case, seeded as the fixture's run was; returns (algo, recorder)."""
    import imitation_amd as p

    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = p.Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones)
    seed_everything(venv, seed)
    algo = p.SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy", rl_kwargs=dict(rl_kwargs_of(cfg), device=device))
    return algo, Recorder(algo)


def run_case(name, seed, device="cuda"):
    cfg = dict(COMMON, **CASES[name])
    algo, rec = build(cfg, seed, device)
    init = {f"init/{k}": v.cpu().numpy() for k, v in algo.policy.state_dict().items()}
    algo.train(total_timesteps=cfg["total_timesteps"], log_interval=cfg["log_interval"])
    return dict(rec.record(), **init)


if __name__ == "__main__":
    np.savez(sys.argv[3], **run_case(sys.argv[1], int(sys.argv[2])))
