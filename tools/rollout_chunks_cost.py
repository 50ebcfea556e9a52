#!/usr/bin/env python3
"""What running a whole-body rollout in stretches costs, torch-event times on one device: 8192 rollouts of 2 s
(50 replans of 40 simulation steps, N = 30, labels attached) from a cold start, plan-following and on the ground-contact
plant, as ONE `open_loop_device(n_replans=50)` and as 5 stretches of 10 replans, the later ones `resume=True`.  A stretch adds
the host's bookkeeping and its copy of the solution views (`parse_sol`) and the allocation of its own S and labels; the
kernels launched are the same.
    python tools/rollout_chunks_cost.py [--runs 5] [--batch 8192] [--out FILE.json]
One warm-up, then `runs` timed windows; median and range as one JSON line.  Nothing here asserts a time."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import wholebody as wbk
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev, B, REPLANS, CHUNK = "cuda:0", a.batch, 50, 10

    def timed(call):
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        return dict(median=round(statistics.median(ms), 2), min=round(min(ms), 2), max=round(max(ms), 2))

    L = BatchedTorqueLayer(**quadruped_tree(), device=dev)
    mpc = LocomotionMPC(print_info=False, device=dev, batch=B, n_nodes=30, force_reference="gravity_share")
    rng = np.random.default_rng(0)
    q0 = np.zeros((B, 18)); q0[:, 2] = 0.30; q0[:, 6:] = wbk.Q_HOME + rng.normal(0, 0.03, (B, 12))
    v0 = np.zeros((B, 18))

    def rollout(stretches, **kw):
        mpc.reset()
        mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
        q, v = q0, v0
        for i, k in enumerate(stretches):
            S = mpc.open_loop_device(q, v, n_replans=k, resume=i > 0, torque_layer=L, **kw)
            q, v = mpc.q_final, mpc.v_final
            del S
        return int((mpc.failed >> 8 != 0).sum())

    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, batch=B, replans=REPLANS, chunk=CHUNK, ms={})
    for name, kw in (("plan", {}), ("plant", dict(plant=GroundContact(), plant_substeps=2))):
        for form, stretches in (("one_call", (REPLANS,)), ("stretches", (CHUNK,) * (REPLANS // CHUNK))):
            res["ms"][f"{name}_{form}"] = timed(lambda: rollout(stretches, **kw))
            res.setdefault("terminated", {})[f"{name}_{form}"] = rollout(stretches, **kw)
            print(name, form, res["ms"][f"{name}_{form}"], flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
