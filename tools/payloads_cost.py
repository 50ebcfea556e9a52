#!/usr/bin/env python3
"""What a payload per robot costs, torch-event times on one device at B = 1024 / 8192:
  1. `contact_track` (20 control steps of 2 substeps) under both integrators: with nothing attached -- the launches the parent
     commit makes too: run this file there for the baseline, in turns with this tree, and compare inside the spread of the
     repeats --, with a table of grounds alone, and with a table of payloads (`torque.sample_payloads`) beside it, one launch of
     the chain with a law and a payload per lane;
  2. `policy_rollout` (20 control steps of 2 substeps, a 3 x 512 policy), the same three ways.
    python tools/payloads_cost.py [--runs 5] [--batches 1024 8192] [--out FILE.json]
One warm-up, then `runs` timed windows; median and range as one JSON line.  Nothing here asserts a time."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import torque as torque_mod
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = "cuda:0"
    tables = hasattr(torque_mod, "sample_payloads")       # the parent commit has no payloads: the other two ways only

    def timed(call, reset=lambda: None):
        reset(); call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            reset()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))

    L = BatchedTorqueLayer(**quadruped_tree(), device=dev)
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, tables=tables)
    ground, steps, n_sub, dt = GroundContact(tau_max=30.0), 20, 2, 5e-4
    stand = np.tile([0.0, 0.7, -1.4], 4)
    for B in a.batches:
        rng = np.random.default_rng(B)
        t32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev)      # noqa: E731
        q0 = np.zeros((B, 18)); q0[:, 6:] = stand + rng.uniform(-0.05, 0.05, (B, 12))
        q0 = t32(q0)
        q0[:, 2] -= L.foot_kinematics(q0)[0][:, :, 2].amin(dim=1) + 0.003      # the lowest foot 3 mm in the ground
        v0 = t32(rng.uniform(-0.2, 0.2, (B, 18)))
        A = t32(stand + rng.uniform(-0.05, 0.05, (B, steps, 12)))
        goal = t32(rng.uniform(-0.5, 0.5, (B, 3)))
        policy = DevicePolicy(47, 12, 3, 512, True, batch_max=B, seed=B)
        rows = t32(torque_mod.sample_grounds(B, rng, base=ground, mu=(0.2, 1.2), stiffness=(5e3, 2e4), damping=(1.0, 5.0),
                                             ground_z=(-0.002, 0.002), tau_max=(10.0, 40.0)))
        loads = t32(torque_mod.sample_payloads(B, B)) if tables else None
        q, v = q0.clone(), v0.clone()

        def reset():
            q.copy_(q0); v.copy_(v0)

        out = {}
        track = lambda: L.contact_track(q, v, A, dt, n_sub, ground=ground, record=False)                         # noqa: E731
        rollout = lambda: L.policy_rollout(policy, q0, v0, steps, dt, n_sub, goal, ground=ground, record=False)   # noqa: E731
        calls = [(f"track_{integrator}", integrator, track) for integrator in ("explicit", "implicit")] + [("policy_rollout", "explicit", rollout)]
        for name, integrator, call in calls:
            L.set_integrator(integrator)
            out[f"{name}_uniform_ms"] = timed(call, reset)
            L.set_grounds(rows)
            out[f"{name}_grounds_ms"] = timed(call, reset)
            if tables:
                L.set_payloads(loads)
                out[f"{name}_payloads_ms"] = timed(call, reset)
                L.set_payloads(None)
                out[f"{name}_payloads_over_grounds"] = round(out[f"{name}_payloads_ms"]["median"] / out[f"{name}_grounds_ms"]["median"], 3)
            L.set_grounds(None)
        L.set_integrator("explicit")
        res[f"B{B}"] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
