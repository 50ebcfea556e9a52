#!/usr/bin/env python3
"""Writes tests/golden/contact_settle.npz: the settling run of tests/contact_reference.drop() -- the quadruped dropped from
2 cm onto the declared ground, 2 000 substeps of 0.5 ms -- through `contact_step_ref` in fp64 over `fd_ref` (the reference) and
in numpy float32 over `aba` (what the number format costs).  Stored: the inputs, the state after the first 50 fp64 substeps
(tests/test_contact_reference.py reproduces it), and the end state (q, v, a, f, tau) of both loops.
    python tests/golden/make_golden_contact_settle.py
The fp64 loop takes about half a minute, so this runs by hand and not inside a test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import contact_reference as cr  # noqa: E402
from tests import fd_reference as fr       # noqa: E402


def main():
    d = cr.drop()
    run = lambda **kw: cr.contact_step_ref(d["m"], d["g"], d["q"], d["v"], d["dt"], d["n_sub"], d["tau_ff"], d["q_des"], d["kp"],  # noqa: E731
                                           d["kd"], **kw)
    trace = []
    q, v, a, f, tau = run(trace=trace)
    q32, v32, a32, f32, tau32 = run(fd=fr.aba, dtype=np.float32)
    assert q32.dtype == np.float32 and f32.dtype == np.float32
    out = dict(q0=d["q"], v0=d["v"], tau_ff=d["tau_ff"], q_des=d["q_des"], kp=d["kp"], kd=d["kd"], dt=d["dt"], n_sub=d["n_sub"],
               q50=trace[49][0], v50=trace[49][1], q=q, v=v, a=a, f=f, tau=tau, q32=q32, v32=v32, a32=a32, f32=f32, tau32=tau32)
    np.savez(os.path.join(HERE, "contact_settle.npz"), **out)
    weight = d["m"].mass.sum() * fr.G
    print(f"sum f_z {f[:, 2].sum():.4f} N, weight {weight:.4f} N, max|v| {np.abs(v).max():.2e}, penetration mm "
          f"{np.round(-1e3 * cr.feet(d['m'], q, v)[0][:, 2], 2)}, pitch {q[4]:.4f}")
    print(f"float32 loop: |q - q64| {np.abs(q32 - q).max():.2e} |v - v64| {np.abs(v32 - v).max():.2e} |f - f64| {np.abs(f32 - f).max():.2e}")


if __name__ == "__main__":
    main()
