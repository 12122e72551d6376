"""`util/util.py`: host helpers shared by modules that must not import each other."""
from __future__ import annotations

import numpy as np


def make_seeds(rng: np.random.Generator) -> int:
    """`util/util.py` `make_seeds(rng)`: one seed below 2^31 - 1, one `integers` draw of shape `(1,)`."""
    return int(rng.integers(0, (1 << 31) - 1, (1,))[0])
