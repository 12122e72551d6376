"""Generates `tests/golden/exploration_*.npz` by running the REFERENCE's own `ExplorationWrapper`
(`imitation.policies.exploration_wrapper`) and `AgentTrainer` (`imitation.algorithms.preference_comparisons`), imported
unmodified under `oracle.ref_shim`, over the stub algorithm and the counting environments of
`tests/exploration_golden.py`. Runs only where the reference sources are present.
Usage: `python tests/golden/make_golden_exploration.py [CASE ...]` (no name: every case).

The shim has no `stable_baselines3.common.type_aliases` and its SB3 `Logger` has no `warn`, which the algorithm module
touches: this script adds both in its own process.

Each file holds the case's settings; per call of the wrapper which policy acted (0 wrapped, 1 random) and its actions;
every trajectory every `sample` returned (`obs`, `acts`, `rews`, `terminal`), in order; the number of calls of the stub
and of the reward function; the `log` / `warn` messages; and, after every `sample` (for the bare wrapper: after its last
call), the state of `rng` and of the action space's generator as decimal strings.

A case that explores is kept only if its trace holds at least `MIN_CALLS_EACH` calls of each policy and at least
`MIN_CHANGES` changes of policy: one that misses this gets another seed in the case table.
"""
import os
import sys
import types as _types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim  # noqa: E402
from tests import exploration_golden as eg  # noqa: E402


def install():
    ref_shim.install()
    from oracle import sb3_restated as sb
    ta = _types.ModuleType("stable_baselines3.common.type_aliases")
    ta.Schedule = object
    sys.modules["stable_baselines3.common.type_aliases"] = ta
    sys.modules["stable_baselines3.common"].type_aliases = ta
    if not hasattr(sb.Logger, "warn"):
        sb.Logger.warn = lambda self, *args, **kwargs: None
    from imitation.algorithms import preference_comparisons as pc
    from imitation.policies import exploration_wrapper
    from imitation.util import logger as imit_logger
    return _types.SimpleNamespace(ExplorationWrapper=exploration_wrapper.ExplorationWrapper, AgentTrainer=pc.AgentTrainer,
                                  make_logger=lambda folder: imit_logger.configure(folder, ["log"]))


def main():
    import tempfile
    names = sys.argv[1:] or list(eg.CASES)
    unknown = [n for n in names if n not in eg.CASES]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {list(eg.CASES)}")
    api = install()
    tmp = tempfile.mkdtemp()
    for name in names:
        cfg = eg.CASES[name]
        out = eg.run_case(cfg, api, os.path.join(tmp, name))
        policy = out["trace_policy"]
        n_random, n_changes = int(policy.sum()), int(np.count_nonzero(np.diff(policy)))
        if eg.explores(cfg):
            assert min(n_random, len(policy) - n_random) >= eg.MIN_CALLS_EACH and n_changes >= eg.MIN_CHANGES, \
                f"{name}: {len(policy) - n_random} wrapped and {n_random} random calls, {n_changes} changes: try another seed"
        else:
            assert len(policy) == 0, f"{name}: {len(policy)} exploratory calls where none were expected"
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, "wrapped", len(policy) - n_random, "random", n_random, "changes", n_changes, "stub calls",
              int(out["stub_calls"]), "messages", list(out["messages"]), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
