"""Cases of the horizons above 128 positions (tests/golden/make_golden_long.py makes their fixtures from the real
reference; tests/test_hip_long_horizon.py runs them).  Inputs are regenerable from the case names, as in cases.py."""
from __future__ import annotations

import numpy as np

from dynamics_aware_diffusion_amd.utils import synth
from tests.golden import cases

# (case, net, horizon, B, t): one forward + its fp64 run and a conditioned loop of the net's schedule length.  Level 0
# of the tiny net (dim 32, mults (1, 2, 4), gamma / beta jittered) at 256 positions — windowed tiles — and a horizon
# that pads up to 256 (200: zero rows 200..255 at level 0)
LONG_CASES = [
    ("hz_tiny_H256", "tiny", 256, 3, 5),
    ("hz_tiny_H200", "tiny", 200, 2, 9),
]

# (case, net, horizon, T, B, loss_type, predict_epsilon): loss.backward() through the reference at a long horizon
LONG_GRAD_CASES = [
    ("grads_tiny_H256", "tiny", 256, 20, 3, "l2", True),
]


def long_train_inputs(case: str, net: str, horizon: int, T: int, B: int):
    """(x_start, per-row timesteps, noise) as cases.train_inputs draws them, at `horizon` rows."""
    _, _, td, _, _ = cases.net_dims(net)
    x0 = np.clip(synth.normal_like(25, case + ".x0", (B, horizon, td)) * 0.5, -1, 1).astype(np.float32)
    u = synth.uniform(25, case + ".t", (B,), 1.0)
    t = np.minimum(((u + 1.0) * 0.5 * T).astype(np.int64), T - 1)
    t[0], t[-1] = 0, T - 1
    noise = synth.normal_like(25, case + ".noise", (B, horizon, td))
    return x0, t, noise
