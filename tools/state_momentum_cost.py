#!/usr/bin/env python3
"""What the tree's momentum in x0 costs a device rollout, torch-event times on one device: one first-solve replan
of `nmpc_wb_rollout_batch` at B = 8192, N = 30 on a handle in the articulated mode with x0's momentum from the tree
(`set_state_momentum("tree")`), against two figures of the same run: the same replan on a declared handle, and the kernel the
mode adds (`BatchedTorqueLayer.state_momentum`) alone at the same B.
    python tools/state_momentum_cost.py [--B 8192] [--N 30] [--windows 5] [--out FILE.json]
A window is one call between two events; every replan starts from the same plant states (the copy that restores q, v is inside
the window, the same for both modes); one warm-up window, then `windows` timed ones per figure, interleaved; median and range as
one JSON line.  The difference of the two replans is the articulated solve (tools/momentum_model_cost.py) plus the kernel; the
kernel's own time says how much of it the new launch is.  Nothing here asserts a time."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import wholebody as wbk
    from iterative_learning_nmpc_amd import workloads as wl
    from iterative_learning_nmpc_amd.config import COLLISION_HEIGHT, N_SQP_FIRST, TERMINATE_DEFAULT
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = torch.device("cuda:0")
    B, N = a.B, a.N
    layer = BatchedTorqueLayer(**wl.quadruped_tree(), device=dev)
    rng = np.random.default_rng(0)
    q0 = np.zeros((B, 18)); q0[:, 2] = 0.30; q0[:, 6:] = wbk.Q_HOME + rng.normal(0, 0.03, (B, 12))
    v0 = rng.normal(0, 0.05, (B, 18))

    def setup(mode):
        kw = dict(momentum_model="articulated", torque_layer=layer) if mode == "tree" else {}
        mpc = LocomotionMPC(print_info=False, device=dev, batch=B, n_nodes=N, force_reference="gravity_share", **kw)
        if mode == "tree":
            mpc.set_state_momentum("tree")
        s = mpc.solver._device_solver()
        c, g = mpc.config_opt, mpc.config_gait
        gait, peaks = (s.to_device(t, torch.int8) for t in (mpc.contact_planner.gait_sequence, mpc.contact_planner.peak_swing))
        joint_ref = s.to_device(mpc.joint_ref)
        qs, vs = s.to_device(q0), s.to_device(v0)
        q, v = qs.clone(), vs.clone()
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)      # noqa: E731
        X, U, status = z(B, N + 1, 42), z(B, N, 30), z(B, dtype=torch.int32)
        v_des, w_des, ref = s.to_device(np.tile([0.2, 0.0, 0.0], (B, 1)), torch.float64), z(B, 3, dtype=torch.float64), z(B, 12, dtype=torch.float64)
        cfg = dict(n_replans=1, replanning_steps=mpc.replanning_steps, nodes_per_cycle=mpc.contact_planner.nodes_per_cycle, first_solve=1,
                   last_node=0, max_sqp_first=N_SQP_FIRST, nlp_tol_first=c.nlp_tol / 10.0, nlp_tol=c.nlp_tol, sim_dt=mpc.sim_dt,
                   time_horizon=c.time_horizon, nom_height=g.nom_height, height_offset=mpc.height_offset, step_height=float(g.step_height),
                   push_start=0.0, push_duration=0.0, record_sim_steps=0, force_reference_gravity=1,
                   nominal_period=float(g.nominal_period), terminate_mask=int(TERMINATE_DEFAULT), collision_height=float(COLLISION_HEIGHT))
        keep = {}

        def call():
            q.copy_(qs); v.copy_(vs); ref.zero_()
            keep["failed"] = s.wb_rollout(gait, peaks, [0], q, v, v_des, w_des, ref, joint_ref, None, X, U, status, **cfg)[1]
        return call, status, keep, mpc

    figures = {m: setup(m) for m in ("declared", "tree")}
    qd, vd = torch.as_tensor(q0, dtype=torch.float32, device=dev), torch.as_tensor(v0, dtype=torch.float32, device=dev)
    h = torch.empty(B, 6, dtype=torch.float32, device=dev)
    calls = {"declared": figures["declared"][0], "tree": figures["tree"][0], "kernel": lambda: layer.state_momentum(qd, vd, out=h)}

    def window(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    ms = {k: [] for k in calls}
    for i in range(a.windows + 1):          # window 0 warms up; the figures alternate within every round
        for k, call in calls.items():
            t = window(call)
            if i:
                ms[k].append(t)
    res = dict(device=torch.cuda.get_device_name(0), B=B, N=N, windows=a.windows, max_sqp_first=N_SQP_FIRST)
    for k, x in ms.items():
        res[k] = dict(median_ms=round(statistics.median(x), 4), min_ms=round(min(x), 4), max_ms=round(max(x), 4))
        if k in figures:
            st = figures[k][1]
            res[k]["solver_failures"] = int(((st == 1) | (st == 4)).sum().item())
    res["tree_over_declared"] = round(res["tree"]["median_ms"] / res["declared"]["median_ms"], 3)
    res["kernel_share_of_tree"] = round(res["kernel"]["median_ms"] / res["tree"]["median_ms"], 5)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
