#!/usr/bin/env python3
"""Writes tests/golden/implicit_settle.npz: the settling run of tests/contact_reference.drop() -- the quadruped dropped from 2 cm
onto the declared ground -- at 500 substeps of 2 ms through `implicit_reference.implicit_step_ref` in fp64 (the reference) and in
numpy float32 (what the number format costs).  Stored: the inputs, the state after the first 20 fp64 substeps
(tests/test_implicit_reference.py reproduces it), the end state (q, v) of both loops and the largest |v| over the last 20 % of each.
    python tests/golden/make_golden_implicit_settle.py
The loops take a quarter of a minute, so this runs by hand; tests/test_implicit_reference.py runs the fp64 loop once more."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import contact_reference as cr  # noqa: E402
from tests import implicit_reference as ir  # noqa: E402

DT, N_SUB = 2e-3, 500


def main():
    d = cr.drop()
    run = lambda **kw: ir.implicit_step_ref(d["m"], d["g"], d["q"], d["v"], DT, N_SUB, d["tau_ff"], d["q_des"], d["kp"], d["kd"], **kw)  # noqa: E731
    trace, trace32 = [], []
    q, v = run(trace=trace)[:2]
    q32, v32 = run(trace=trace32, dtype=np.float32)[:2]
    assert q32.dtype == np.float32
    out = dict(q0=d["q"], v0=d["v"], tau_ff=d["tau_ff"], q_des=d["q_des"], kp=d["kp"], kd=d["kd"], dt=DT, n_sub=N_SUB,
               q20=trace[19][0], v20=trace[19][1], q=q, v=v, q32=q32, v32=v32, tail=ir.tail_speed(trace), tail32=ir.tail_speed(trace32))
    np.savez(os.path.join(HERE, "implicit_settle.npz"), **out)
    print(f"tail |v| {out['tail']:.2e} (float32 {out['tail32']:.2e}), z {q[2]:.4f}, pitch {q[4]:.4f}; "
          f"float32 loop: |q - q64| {np.abs(q32 - q).max():.2e} |v - v64| {np.abs(v32 - v).max():.2e}")


if __name__ == "__main__":
    main()
