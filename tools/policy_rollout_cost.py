#!/usr/bin/env python3
"""What a policy in the loop on the contact plant costs: torch-event time per control step of `BatchedTorqueLayer.policy_rollout`
(one library call for all steps) next to the same chain made of three Python calls per step (`observe`, `DevicePolicy.forward`,
`contact_step`) in the same process, and of each of the three calls alone, at B = 1024 and B = 8192 with n_sub = 2 and 20 at
dt = 0.5 ms, on the quadruped tree with the policy of the reference's configuration (47 -> 3 x 512 with BatchNorm -> 12,
batch_max = B).
    python tools/policy_rollout_cost.py [--runs 5] [--steps 20] [--out FILE.json]
Per figure: one warm-up, then `runs` timed windows of `steps` control steps each; microseconds per control step, median and
range, as one JSON line.  The robots start in standing poses a few millimetres in the ground and the policy's last bias is the
standing pose (its last weights scaled down), so the plant stays near standing and the law is at work; the calls go through the
Python layer (argument checks, output allocation from torch's cache); nothing here asserts a time."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    from iterative_learning_nmpc_amd.torque import NOMINAL_PERIOD, BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    K, dt = a.steps, 5e-4

    def timed(call, per):
        call()                                              # warm-up: code object, allocator, the handle's action buffer
        torch.cuda.synchronize()
        us = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            us.append(t0.elapsed_time(t1) * 1e3 / per)
        return dict(median_us=round(statistics.median(us), 1), min_us=round(min(us), 1), max_us=round(max(us), 1))

    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, steps=K, dt=dt)
    L = BatchedTorqueLayer(**quadruped_tree())
    ground = GroundContact()
    stand = np.tile([0.0, 0.7, -1.4], 4)
    for B in (1024, 8192):
        rng = np.random.default_rng(B)
        dev = lambda x, t=torch.float32: torch.as_tensor(x, dtype=t, device="cuda:0")   # noqa: E731
        q = np.zeros((B, 18)); q[:, 6:] = stand + rng.uniform(-0.05, 0.05, (B, 12))
        q = dev(q)
        q[:, 2] -= L.foot_kinematics(q)[0][:, :, 2].amin(dim=1) + 0.003     # the lowest foot 3 mm in the ground
        v, goal = dev(rng.uniform(-0.2, 0.2, (B, 18))), dev(rng.uniform(-0.5, 0.5, (B, 3)))
        mean, std = dev(rng.uniform(-0.5, 0.5, 44), torch.float64), dev(rng.uniform(0.5, 2.0, 44), torch.float64)
        policy = DevicePolicy(47, 12, 3, 512, True, batch_max=B, seed=B)
        theta, rm, rv = policy.get_parameters()
        name, shape, off = policy.items[-2]
        theta[off:off + 12 * 512] *= 0.01                                    # actions near the last bias ...
        theta[policy.items[-1][2]:] = dev(stand)                             # ... which is the standing pose
        policy.set_parameters(theta, rm, rv)
        x = L.observe(q, v, 0.0, NOMINAL_PERIOD, goal, s_mean=mean, s_std=std)[1]
        act = policy.forward(x)
        out = {}
        for n_sub in (2, 20):
            def chain():
                qc, vc = q, v
                failed = torch.zeros(B, dtype=torch.int32, device="cuda:0")
                S, A = torch.empty(B, K, 44, device="cuda:0"), torch.empty(B, K, 12, device="cuda:0")
                for k in range(K):
                    s, xk = L.observe(qc, vc, k * n_sub * dt, NOMINAL_PERIOD, goal, s_mean=mean, s_std=std, failed=failed, step_index=k, term_mask=33)
                    ak = policy.forward(xk)
                    qc, vc = L.contact_step(qc, vc, dt, n_sub, q_des=ak, ground=ground)[:2]
                    S[:, k], A[:, k] = s, ak
                L.observe(qc, vc, K * n_sub * dt, NOMINAL_PERIOD, goal, s_mean=mean, s_std=std, failed=failed, step_index=K, term_mask=33)
            out[f"n_sub{n_sub}"] = dict(
                rollout=timed(lambda: L.policy_rollout(policy, q, v, K, dt, n_sub, goal, s_mean=mean, s_std=std, ground=ground), K),
                rollout_no_record=timed(lambda: L.policy_rollout(policy, q, v, K, dt, n_sub, goal, s_mean=mean, s_std=std, ground=ground, record=False), K),
                chain=timed(chain, K),
                contact_step=timed(lambda: [L.contact_step(q, v, dt, n_sub, q_des=act, ground=ground) for _ in range(K)], K))
        out["observe"] = timed(lambda: [L.observe(q, v, 0.0, NOMINAL_PERIOD, goal, s_mean=mean, s_std=std) for _ in range(K)], K)
        out["forward"] = timed(lambda: [policy.forward(x) for _ in range(K)], K)
        qf, vf, _, A, failed = L.policy_rollout(policy, q, v, K, dt, 20, goal, s_mean=mean, s_std=std, ground=ground)
        out["finite"] = bool(torch.isfinite(qf).all() and torch.isfinite(vf).all())
        out["terminated"] = int((failed >> 8 != 0).sum())
        out["action_spread"] = float((A - dev(stand)).abs().max())
        res[f"B{B}"] = out
        del policy
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
