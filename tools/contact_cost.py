#!/usr/bin/env python3
"""What the contact plant of the torque layer costs: torch-event time of `BatchedTorqueLayer.contact_step` next to `step`
(given forces), both with n_sub = 20, and of `contact_forces` / `foot_kinematics` next to `forward_dynamics`, on the quadruped
tree at B = 1024 and B = 8192 on the same box.
    python tools/contact_cost.py [--runs 5] [--reps 20] [--out FILE.json]
Per figure: one warm-up, then `runs` timed windows of `reps` back-to-back calls each; microseconds per call, median and range,
as one JSON line.  The states are standing poses a few millimetres in the ground, so the law is at work in every substep; the
calls go through the Python layer (argument checks, output allocation from torch's cache); nothing here asserts a time."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"

    def timed(call):
        call()                                              # warm-up: code object, allocator
        torch.cuda.synchronize()
        us = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                call()
            t1.record()
            torch.cuda.synchronize()
            us.append(t0.elapsed_time(t1) * 1e3 / a.reps)
        return dict(median_us=round(statistics.median(us), 1), min_us=round(min(us), 1), max_us=round(max(us), 1))

    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, reps=a.reps, n_sub=20)
    L = BatchedTorqueLayer(**quadruped_tree())
    ground = GroundContact()
    stand = np.tile([0.0, 0.7, -1.4], 4)
    for B in (1024, 8192):
        rng = np.random.default_rng(B)
        dev = lambda x: torch.as_tensor(x, dtype=torch.float32, device="cuda:0")   # noqa: E731
        q = np.zeros((B, 18)); q[:, 6:] = stand + rng.uniform(-0.05, 0.05, (B, 12))
        q = dev(q)
        q[:, 2] -= L.foot_kinematics(q)[0][:, :, 2].amin(dim=1) + 0.003     # the lowest foot 3 mm in the ground
        v, tau = dev(rng.uniform(-0.2, 0.2, (B, 18))), dev(rng.uniform(-5, 5, (B, 12)))
        q_des = q[:, 6:].contiguous()
        f = L.contact_forces(q, v, ground)
        res[f"B{B}"] = dict(
            feet_in_contact=float((f[:, :, 2] > 0).float().mean()),
            foot_kinematics=timed(lambda: L.foot_kinematics(q, v)),
            contact_forces=timed(lambda: L.contact_forces(q, v, ground)),
            forward_dynamics=timed(lambda: L.forward_dynamics(q, v, tau, f)),
            step20=timed(lambda: L.step(q, v, 5e-4, 20, tau_ff=tau, q_des=q_des, f=f)),
            contact_step20=timed(lambda: L.contact_step(q, v, 5e-4, 20, tau_ff=tau, q_des=q_des, ground=ground)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
