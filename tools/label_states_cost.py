#!/usr/bin/env python3
"""What DAgger relabelling costs and what one iteration of it does, torch-event times on one device:
  1. `BatchedNmpcSolver.label_states` on 8192 visited states (B = 64 robots x K = 128 rows, batch_max = 8192: one chunk) next to a
     one-replan first-solve `wb_rollout` of 8192 rollouts from the same states on the same build -- the same solves behind the
     existing prepare kernel --, without and with labels attached;
  2. `BatchedTorqueLayer.policy_rollout` per control step with and without `set_rollout_states`, B = 1024 / 8192, n_sub = 2 / 20;
  3. one `learning.dagger_iteration` at B = 64, T = 1 s from an untrained policy: visited states labelled, solves per status, mean
     |A - A*| over the appended rows before and after the iteration's training.
    python tools/label_states_cost.py [--runs 5] [--out FILE.json]
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
    from iterative_learning_nmpc_amd import learning, wholebody as wbk
    from iterative_learning_nmpc_amd.config import COLLISION_HEIGHT, N_SQP_FIRST, TERMINATE_DEFAULT
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = "cuda:0"

    def timed(call, per=1.0):
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1) / per)
        return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))

    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs)
    L = BatchedTorqueLayer(**quadruped_tree(), device=dev)

    # ---- 1. 8192 states against 8192 one-replan rollouts
    B, K, M = 64, 128, 8192
    mpc = LocomotionMPC(print_info=False, device=dev, batch=M, n_nodes=30, force_reference="gravity_share")
    mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
    s = mpc.solver._device_solver()
    rng = np.random.default_rng(0)
    q = np.zeros((M, 18)); q[:, 2] = 0.30; q[:, 6:] = wbk.Q_HOME + rng.normal(0, 0.03, (M, 12))
    Q, V = s.to_device(q.reshape(B, K, 18)), torch.zeros(B, K, 18, dtype=torch.float32, device=dev)
    nodes, ref_steps = mpc.label_clock(K, 0.0, 20 * 5e-4)
    gait, peaks = (s.to_device(t, torch.int8) for t in (mpc.contact_planner.gait_sequence, mpc.contact_planner.peak_swing))
    c, g = mpc.config_opt, mpc.config_gait
    common = dict(nodes_per_cycle=mpc.contact_planner.nodes_per_cycle, sim_dt=mpc.sim_dt, time_horizon=c.time_horizon, nom_height=g.nom_height,
                  height_offset=mpc.height_offset, step_height=float(g.step_height), force_reference_gravity=1)
    f64 = lambda x, n: s.to_device(np.tile(x, (n, 1)), torch.float64)      # noqa: E731
    cmd = {n: (f64([0.2, 0, 0], n), f64([0, 0, 0], n), f64(np.zeros(12), n)) for n in (B, M)}      # v_des, w_des, ref_state per robot / rollout
    X, U = torch.zeros(M, 31, 42, dtype=torch.float32, device=dev), torch.zeros(M, 30, 30, dtype=torch.float32, device=dev)
    A, st = torch.zeros(B, K, 12, dtype=torch.float32, device=dev), torch.zeros(B, K, dtype=torch.int32, device=dev)
    dn, ds, zoh1, jref = s.to_device(nodes, torch.int32), s.to_device(ref_steps, torch.int32), s.to_device([0], torch.int32), s.to_device(mpc.joint_ref)

    def label(steps):
        s.label_states(L, gait, peaks, dn, steps, Q, V, *cmd[B], jref, zoh1, A=A, status=st,
                       X=X, U=U, max_sqp=N_SQP_FIRST, nlp_tol=c.nlp_tol / 10.0, kp=mpc.Kp, kd=mpc.Kd, terminate_mask=TERMINATE_DEFAULT, **common)

    qm, vm = Q.reshape(M, 18).contiguous(), V.reshape(M, 18).contiguous()
    status = torch.zeros(M, dtype=torch.int32, device=dev)

    def harness():
        s.wb_rollout(gait, peaks, [0], qm.clone(), vm.clone(), cmd[M][0], cmd[M][1], cmd[M][2].clone(), jref, None, X, U, status,
                     n_replans=1, replanning_steps=mpc.replanning_steps, first_solve=1, last_node=0, max_sqp_first=N_SQP_FIRST,
                     nlp_tol_first=c.nlp_tol / 10.0, nlp_tol=c.nlp_tol, push_start=0.0, push_duration=0.0, record_sim_steps=1,
                     nominal_period=float(g.nominal_period), terminate_mask=0, collision_height=float(COLLISION_HEIGHT), **common)

    one = dict(label_states_ms=timed(lambda: label(ds)), label_states_no_reference_steps_ms=timed(lambda: label(torch.zeros_like(ds))),
               rollout_one_replan_ms=timed(harness))
    Al = torch.zeros(M, mpc.replanning_steps, 12, dtype=torch.float32, device=dev)
    s.set_rollout_actions(L, s.to_device(mpc.id_repeat[:mpc.replanning_steps], torch.int32), Al, mpc.Kp, mpc.Kd)
    one["rollout_one_replan_with_labels_ms"] = timed(harness)
    s.set_rollout_actions(None)
    one["ratio_label_over_rollout"] = round(one["label_states_ms"]["median"] / one["rollout_one_replan_ms"]["median"], 3)
    label(ds); torch.cuda.synchronize()
    one["statuses"] = {int(k): int(v) for k, v in zip(*np.unique(st.cpu().numpy(), return_counts=True))}
    res["states_8192"] = one
    del mpc, s, X, U, Al

    # ---- 2. the policy rollout with and without states attached
    ground, steps, dt = GroundContact(), 20, 5e-4
    stand = np.tile([0.0, 0.7, -1.4], 4)
    for Bp in (1024, 8192):
        rng = np.random.default_rng(Bp)
        t32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev)      # noqa: E731
        qp = np.zeros((Bp, 18)); qp[:, 6:] = stand + rng.uniform(-0.05, 0.05, (Bp, 12))
        qp = t32(qp)
        qp[:, 2] -= L.foot_kinematics(qp)[0][:, :, 2].amin(dim=1) + 0.003
        vp, goal = t32(rng.uniform(-0.2, 0.2, (Bp, 18))), t32(rng.uniform(-0.5, 0.5, (Bp, 3)))
        policy = DevicePolicy(47, 12, 3, 512, True, batch_max=Bp, seed=Bp)
        theta, rm, rv = policy.get_parameters()
        theta[policy.items[-2][2]:policy.items[-2][2] + 12 * 512] *= 0.01
        theta[policy.items[-1][2]:] = t32(stand)
        policy.set_parameters(theta, rm, rv)
        Qs, Vs = (torch.empty(Bp, steps, 18, dtype=torch.float32, device=dev) for _ in range(2))
        out = {}
        for n_sub in (2, 20):
            roll = lambda: L.policy_rollout(policy, qp, vp, steps, dt, n_sub, goal, ground=ground)      # noqa: E731
            plain = timed(roll, steps / 1e3)
            L.set_rollout_states(Qs, Vs)
            attached = timed(roll, steps / 1e3)
            L.set_rollout_states(None)
            out[f"n_sub{n_sub}"] = dict(plain_us_per_step=plain, with_states_us_per_step=attached)
        res[f"policy_rollout_B{Bp}"] = out
        del policy

    # ---- 3. one iteration
    Bd, T = 64, 1.0
    mpc = LocomotionMPC(print_info=False, device=dev, batch=Bd, n_nodes=30, force_reference="gravity_share")
    mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
    rng = np.random.default_rng(1)
    q0 = np.zeros((Bd, 18)); q0[:, 2] = 0.30; q0[:, 6:] = wbk.Q_HOME + rng.normal(0, 0.03, (Bd, 12))
    goal = np.tile(np.float32([0.2, 0.0, 0.0]), (Bd, 1))
    policy = DevicePolicy(47, 12, 3, 512, True, batch_max=8192, seed=0)
    db = DeviceDatabase(limit=32768, norm_input=False, device=dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = learning.dagger_iteration(mpc, L, db, policy, q0, np.zeros((Bd, 18)), goal, T, n_epoch=1, batch_size=256, lr=1e-3, seed=0)
    t1.record()
    torch.cuda.synchronize()
    Kd = out["S"].shape[1]
    alive = torch.arange(Kd, device=dev)[None, :] < out["steps_survived"][:, None]
    stv = out["status"][alive].cpu().numpy()
    n = len(db)
    Sx, Ax = db.tables["states"][:n], db.tables["actions"][:n]
    xin = torch.cat([Sx, torch.as_tensor(goal[:1], device=dev).expand(n, 3)], dim=1).contiguous()
    kept = (alive & (out["status"] != 1) & (out["status"] != 4))
    res["dagger_iteration"] = dict(
        B=Bd, T=T, control_steps=Kd, ms=round(t0.elapsed_time(t1), 1), survived=int(out["survived"].sum()), states_labelled=int(alive.sum()),
        statuses={int(k): int(v) for k, v in zip(*np.unique(stv, return_counts=True))}, rows_appended=out["n_rows"],
        mean_abs_A_minus_Astar_before=float((out["A"][kept] - out["A_star"][kept]).abs().mean()),
        mean_abs_A_minus_Astar_after=float((policy.forward(xin) - Ax).abs().mean()),
        train_loss_first_last=[float(out["train_loss"][0, 0]), float(out["train_loss"][0, -1])])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
