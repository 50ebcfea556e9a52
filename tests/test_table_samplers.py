"""The samplers of the per-robot plant tables give the bytes they gave: `sample_grounds`, `sample_payloads`, `sample_actuators`,
`sample_delays`, `sample_noise` and `training_sigma` against tests/golden/table_samplers.npz, which
tests/golden/make_golden_table_samplers.py wrote from `tables()` below before the samplers came to share one draw.  Two seeds,
n = 1, 33, 257, the default ranges and others; every array equal in dtype, shape and value.  No device is needed."""
import os

import numpy as np

from iterative_learning_nmpc_amd import torque

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_samplers.npz")
SEEDS, SIZES = (3, 20241), (1, 33, 257)
DEFAULT = dict(grounds=dict(mu=(0.4, 1.0)), payloads={}, actuators={}, delays={}, noise={})      # grounds draws nothing by default
# the other ranges: a degenerate one (lo == hi), ends that are no float32 values, and columns that are not drawn at all
OTHER = dict(grounds=dict(mu=(0.3, 1.1), stiffness=(5e3, 2e4), tau_max=(20.0, 20.0)),
             payloads=dict(mass=(0.1, 2.5), offset=((-0.2, 0.3), (0.0, 0.0), (0.01, 0.07))),
             actuators=dict(kp=(10.0, 30.1), kd=(0.1, 0.3), damping=(0.0, 0.0), armature=(0.001, 0.0123)),
             delays=dict(steps=(1, 7)),
             noise=dict(sigma=dict(v_lin=0.3, joints=0.0), bias=dict(z=0.1, joint_rates=0.2)))


def tables():
    """every sampled table of the comparison by name"""
    out = {}
    for seed in SEEDS:
        for n in SIZES:
            for kind, kws in (("default", DEFAULT), ("other", OTHER)):
                key = lambda name: f"{name}_{kind}_s{seed}_n{n}"      # noqa: E731
                out[key("grounds")] = torque.sample_grounds(n, np.random.default_rng(seed), **kws["grounds"])
                out[key("payloads")] = torque.sample_payloads(n, seed, **kws["payloads"])
                out[key("actuators")] = torque.sample_actuators(n, seed, **kws["actuators"])
                out[key("delays")] = torque.sample_delays(n, seed, **kws["delays"])
                out[key("noise")] = torque.sample_noise(n, seed, **kws["noise"])
                out[key("training_sigma")] = torque.training_sigma(out[key("noise")])
    return out


def test_the_samplers_give_the_golden_bytes():
    got = tables()
    with np.load(GOLDEN) as want:
        assert sorted(got) == sorted(want.files)
        worst = 0.0
        for name in sorted(got):
            x, y = got[name], want[name]
            assert x.dtype == y.dtype and x.shape == y.shape, name
            worst = max(worst, float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()))
        print(f"  largest difference over {len(got)} tables: {worst:.3e}")
        for name in sorted(got):
            assert np.array_equal(got[name], want[name]), name
