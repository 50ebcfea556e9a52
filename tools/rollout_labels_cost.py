#!/usr/bin/env python3
"""What the action labels cost a whole-body device rollout: torch-event time of `LocomotionMPC.open_loop_device` without and
with a label buffer, alternating, at the size of tests/test_gpu_wholebody.py::test_wholebody_device_rollouts_full_size
(B = 8192, N = 30, T = 2.0 s, gravity_share force reference, pushes of 50-70 N).
    python tools/rollout_labels_cost.py [--B 8192] [--T 2.0] [--runs 3] [--no-labels] [--out FILE.json]
One warm-up per variant, then `runs` timed calls of each, alternating; prints the runs, medians and spread (max - min) as one
JSON line.  --no-labels times the plain rollout only and needs nothing this feature added (it runs on an older checkout when
the script is started from that tree: ROOT is the tree the script lies in, or NMPC_TREE).  Under rocprofv3 --kernel-trace
--stats use --runs 1: the label kernel is `plan_actions_kernel`."""
import argparse, json, os, statistics, sys

ROOT = os.environ.get("NMPC_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--T", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-labels", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import wholebody as wbk
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    B, T = a.B, a.T
    rng = np.random.default_rng(5)
    q0 = np.zeros((B, 18)); q0[:, 2] = 0.30; q0[:, 6:] = wbk.Q_HOME + rng.normal(0, 0.03, (B, 12))
    v0 = np.zeros((B, 18))
    force = rng.uniform(-1, 1, (B, 3)); force /= np.linalg.norm(force, axis=1, keepdims=True); force *= rng.uniform(50, 70, (B, 1))
    force[0] = 0.0
    push = dict(start=0.2, duration=0.3, force=force)
    layer = None if a.no_labels else BatchedTorqueLayer(**quadruped_tree())
    mpc = LocomotionMPC(print_info=False, device="cuda:0", batch=B, n_nodes=30, force_reference="gravity_share")

    def run(labels: bool) -> float:
        mpc.reset()
        mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
        kw = dict(torque_layer=layer) if labels else {}
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        mpc.open_loop_device(q0, v0, T, push=push, **kw)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / 1e3

    variants = [False] if a.no_labels else [False, True]
    for v in variants:
        run(v)                                              # warm-up: code objects, allocator
    times = {v: [] for v in variants}
    for _ in range(a.runs):
        for v in variants:
            times[v].append(run(v))
    res = dict(B=B, T=T, replans=int(round(T * mpc.replanning_freq)), terminated=int((mpc.failed >> 8 != 0).sum()))
    for v in variants:
        k = "with_labels" if v else "without_labels"
        res[k + "_s"] = [round(t, 4) for t in times[v]]
        res[k + "_median_s"] = round(statistics.median(times[v]), 4)
        res[k + "_spread_s"] = round(max(times[v]) - min(times[v]), 4)
    if len(variants) == 2:
        res["labels_cost_s"] = round(res["with_labels_median_s"] - res["without_labels_median_s"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
