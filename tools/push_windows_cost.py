#!/usr/bin/env python3
"""What a push window per rollout costs, torch-event times on one device at B = 1024 / 8192:
  1. a pushed `contact_track` (20 control steps of 2 substeps) under both integrators, with one window for the batch -- the cut
     into un-pushed and pushed launches, which the parent commit has too: run this file there for the baseline -- and with every
     robot on a window of its own (`mpc.sample_push_windows` over the length of the track), one launch of the windowed kernel;
  2. a plant-mode whole-body rollout of `--seconds` (2 s) pushed as a force, with one window and with a window per rollout.
    python tools/push_windows_cost.py [--runs 5] [--seconds 2.0] [--batches 1024 8192] [--no-rollout] [--out FILE.json]
One warm-up, then `runs` timed windows; median and range as one JSON line.  Nothing here asserts a time."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import mpc as mpc_mod
    from iterative_learning_nmpc_amd import wholebody as wbk
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = "cuda:0"
    windows = hasattr(mpc_mod, "sample_push_windows")      # the parent commit has the uniform path only

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
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, windows=windows)
    ground, steps, n_sub, dt = GroundContact(), 20, 2, 5e-4
    stand = np.tile([0.0, 0.7, -1.4], 4)
    for B in a.batches:
        rng = np.random.default_rng(B)
        t32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev)      # noqa: E731
        q0 = np.zeros((B, 18)); q0[:, 6:] = stand + rng.uniform(-0.05, 0.05, (B, 12))
        q0 = t32(q0)
        q0[:, 2] -= L.foot_kinematics(q0)[0][:, :, 2].amin(dim=1) + 0.003      # the lowest foot 3 mm in the ground
        v0 = t32(rng.uniform(-0.2, 0.2, (B, 18)))
        A = t32(stand + rng.uniform(-0.05, 0.05, (B, steps, 12)))
        F = t32(rng.uniform(-80, 80, (B, 3)))
        q, v = q0.clone(), v0.clone()

        def reset():
            q.copy_(q0); v.copy_(v0)

        out = {}
        track = lambda: L.contact_track(q, v, A, dt, n_sub, ground=ground, record=False)      # noqa: E731
        total = steps * n_sub
        for integrator in ("explicit", "implicit"):
            L.set_integrator(integrator)
            L.set_push(F, 5 * n_sub + n_sub // 2, 10 * n_sub)                   # from the middle of step 5 to the middle of step 15
            out[f"track_{integrator}_uniform_ms"] = timed(track, reset)
            if windows:
                # ten start points over the track, 0.2 - 0.4 of its length
                w = mpc_mod.sample_push_windows(B, B, total * dt, duration=(0.2 * total * dt, 0.4 * total * dt))
                first = np.round(w["start"] / dt).astype(np.int64)
                count = np.round(w["duration"] / dt).astype(np.int64)
                L.set_push(F, first, count)
                out[f"track_{integrator}_per_robot_ms"] = timed(track, reset)
                out[f"track_{integrator}_per_robot_over_uniform"] = round(
                    out[f"track_{integrator}_per_robot_ms"]["median"] / out[f"track_{integrator}_uniform_ms"]["median"], 3)
            L.set_push(None)
        L.set_integrator("explicit")
        if not a.no_rollout:
            q_start = np.zeros((B, 18)); q_start[:, 2] = 0.30; q_start[:, 6:] = wbk.Q_HOME
            v_start = np.zeros((B, 18))
            force = rng.uniform(-60, 60, (B, 3))

            def rollout(push):
                def call():
                    mpc = LocomotionMPC(print_info=False, device=dev, batch=B, force_reference="gravity_share")
                    mpc.open_loop_device(q_start, v_start, a.seconds, torque_layer=L, plant=ground, plant_substeps=n_sub, push=push,
                                         push_as_force=True)
                return call

            out["rollout_uniform_ms"] = timed(rollout(dict(start=0.5, duration=0.3, force=force)))
            if windows:
                w = mpc_mod.sample_push_windows(B, B, 0.5)
                out["rollout_per_rollout_ms"] = timed(rollout(dict(w, force=force)))
                out["rollout_per_rollout_over_uniform"] = round(out["rollout_per_rollout_ms"]["median"] / out["rollout_uniform_ms"]["median"], 3)
        res[f"B{B}"] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
