#!/usr/bin/env python3
"""What the push on the contact plant costs, torch-event times on one device: `contact_step` (one control step) and
`contact_track` (20 control steps) at B = 1024 / 8192 and n_sub = 2 / 20,
  1. detached -- the un-pushed kernels, which a build without the push (the parent commit: run this file there) has too;
  2. with a push that covers every substep -- one launch of the pushed kernel;
  3. with a window inside the call, from the middle of one control step to the middle of a later one (for the step: the middle
     half of its substeps) -- the call is then cut into un-pushed and pushed launches, three for the step, seven for the track.
    python tools/push_cost.py [--runs 5] [--out FILE.json]
One warm-up, then `runs` timed windows; median and range as one JSON line.  Nothing here asserts a time."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = "cuda:0"

    def timed(call, reset):
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
    can_push = hasattr(L, "set_push")
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, pushes=can_push)
    ground, steps, dt = GroundContact(), 20, 5e-4
    stand = np.tile([0.0, 0.7, -1.4], 4)
    for B in (1024, 8192):
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

        for n_sub in (2, 20):
            step = lambda: L.contact_step(q0, v0, dt, n_sub, q_des=A[:, 0], ground=ground)      # noqa: E731
            track = lambda: L.contact_track(q, v, A, dt, n_sub, ground=ground, record=False)     # noqa: E731
            out = dict(step_detached_ms=timed(step, reset), track_detached_ms=timed(track, reset))
            if can_push:
                L.set_push(F, 0, steps * n_sub)
                out.update(step_pushed_ms=timed(step, reset), track_pushed_ms=timed(track, reset))
                if n_sub >= 4:                                              # a window strictly inside a step needs three substeps
                    L.set_push(F, n_sub // 4, n_sub // 2)                   # the step: its middle half, three launches
                    out["step_inside_ms"] = timed(step, reset)
                L.set_push(F, 5 * n_sub + n_sub // 2, 10 * n_sub)           # the track: from the middle of step 5 to the middle of step 15
                out["track_inside_ms"] = timed(track, reset)
                L.set_push(None)
                for k in ("step", "track"):
                    out[f"{k}_pushed_over_detached"] = round(out[f"{k}_pushed_ms"]["median"] / out[f"{k}_detached_ms"]["median"], 3)
                    if f"{k}_inside_ms" in out:
                        out[f"{k}_inside_over_detached"] = round(out[f"{k}_inside_ms"]["median"] / out[f"{k}_detached_ms"]["median"], 3)
            res[f"B{B}_n_sub{n_sub}"] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
