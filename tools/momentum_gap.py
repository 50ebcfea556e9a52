#!/usr/bin/env python3
"""How far the declared centroidal momentum of model 2 is from the articulated tree's, and what the composite-inertia pass costs
("Composite inertia: mass matrix and centroidal map").
    python tools/momentum_gap.py [--runs 5] [--rollouts 8] [--every 10] [--out FILE.json]
Gap: `wholebody.centroidal_momentum_batch(q, v, 15.0, (0.11, 0.27, 0.33))` -- [m rdot; R I_b E(theta) thetadot], centre of mass at the
base origin -- against h and com - q[:3] of `workloads.quadruped_tree()`, over three state sets:
  standing            Q_HOME at z = 0.30, at rest (both momenta are zero: only the centre-of-mass offset says something);
  standing_perturbed  that pose + N(0, 0.03) on all 18 coordinates, base velocity N(0, 0.3), joint rates N(0, 2.0); 256 states;
  trot_on_plant       the plant states of one second of the whole-body expert trotting at 0.3 m/s on the contact plant
                      (`plant_rollout_study.py`'s run), every `every`-th recorded row of the rollouts that survive, turned
                      back from the 44-slot row into the Euler layout (x = y = 0: neither quantity depends on them).  Needs a
                      HIP device; without one the set is left out.
Per set: relative L2 of the linear part, relative L2 of the angular part (|declared - tree| / |tree| over the set), and the mean
and largest norm of com - q[:3]; from the fp64 reference of tests/crba_reference.py, and beside it from the device.
Cost (HIP device only), torch-event times, one warm-up and the median, min, max of `runs` windows at B = 1024 and 8192 on the
perturbed standing states: `mass_matrix`, `centroidal` with and without Ag, and `forward_dynamics` as the yardstick of the family.
One JSON line; nothing here asserts a number."""
import argparse, json, os, statistics, sys, warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASS, INERTIA = 15.0, (0.11, 0.27, 0.33)      # the declared model's (mpc.LocomotionMPC defaults)


def rows_to_euler(S):
    """44-slot rows [.., 44] -> (q, v) [.., 18] in the solver's Euler layout with x = y = 0: the inverse of
    trajectory_io.convert_to_mujoco on [phase, v(18), z, quaternion wxyz, joints(12), base_wrt_feet(8)]"""
    import numpy as np
    S = np.asarray(S, float)
    w, x, y, z = (S[..., 20 + k] for k in range(4))
    r00, r10, r20 = 1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)
    r21, r22 = 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    yaw, pitch, roll = np.arctan2(r10, r00), -np.arcsin(np.clip(r20, -1, 1)), np.arctan2(r21, r22)
    q = np.zeros(S.shape[:-1] + (18,)); v = np.zeros_like(q)
    q[..., 2] = S[..., 19]; q[..., 3], q[..., 4], q[..., 5] = yaw, pitch, roll; q[..., 6:] = S[..., 24:36]
    sp, cp, sr, cr = np.sin(pitch), np.cos(pitch), np.sin(roll), np.cos(roll)
    zero, one = np.zeros_like(sp), np.ones_like(sp)
    E = np.stack([np.stack([-sp, zero, one], -1), np.stack([cp * sr, cr, zero], -1), np.stack([cr * cp, -sr, zero], -1)], -2)
    v[..., :3] = S[..., 1:4]
    v[..., 3:6] = np.linalg.solve(E, S[..., 4:7][..., None])[..., 0]      # body rates = E (yaw, pitch, roll rates)
    v[..., 6:] = S[..., 7:19]
    return q, v


def gap(q, v, com, h):
    """the figures of one set from the tree's com [B, 3] and h [B, 6]"""
    import numpy as np
    from iterative_learning_nmpc_amd import wholebody as wbk
    d = wbk.centroidal_momentum_batch(q, v, MASS, INERTIA)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b)) if np.linalg.norm(b) > 0 else None      # noqa: E731
    off = np.linalg.norm(com - q[:, :3], axis=1)
    return dict(states=len(q), linear_rel_l2=rel(d[:, :3], h[:, :3]), angular_rel_l2=rel(d[:, 3:], h[:, 3:]),
                com_offset_mean_m=float(off.mean()), com_offset_max_m=float(off.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=8)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import wholebody as wbk
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    from oracle import torque_oracle as to
    from tests import crba_reference as cr
    tree = quadruped_tree()
    m = to.TreeModel.from_arrays(tree)
    gpu = torch.cuda.is_available()
    res = dict(device=torch.cuda.get_device_name(0) if gpu else None, declared=dict(mass=MASS, inertia=INERTIA), tree_mass=float(m.mass.sum()))

    stand = np.zeros(18); stand[2] = 0.30; stand[6:] = wbk.Q_HOME
    rng = np.random.default_rng(7)
    sets = dict(standing=(stand[None].copy(), np.zeros((1, 18))))
    v = np.concatenate([rng.normal(0, 0.3, (256, 6)), rng.normal(0, 2.0, (256, 12))], axis=1)
    sets["standing_perturbed"] = (stand + rng.normal(0, 0.03, (256, 18)), v)
    # the inverse above against the forward conversion, on the perturbed set
    from iterative_learning_nmpc_amd.trajectory_io import convert_to_mujoco, state_row
    q_p, v_p = sets["standing_perturbed"]
    rows = np.stack([state_row(0.0, *convert_to_mujoco(q_p[b], v_p[b])[::-1], np.zeros(8)) for b in range(8)])
    q_b, v_b = rows_to_euler(rows)
    assert np.abs(q_b[:, 2:] - q_p[:8, 2:]).max() < 1e-12 and np.abs(v_b - v_p[:8]).max() < 1e-12, "rows_to_euler does not invert convert_to_mujoco"

    L = None
    if gpu:
        from iterative_learning_nmpc_amd.config import TERMINATE_DEFAULT
        from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
        from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
        L = BatchedTorqueLayer(**tree)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mpc = LocomotionMPC(print_info=False, batch=a.rollouts, force_reference="gravity_share")
        mpc.set_command(np.array([0.3, 0.0, 0.0]), 0.0)
        q0 = np.tile(stand, (a.rollouts, 1))
        mask = TERMINATE_DEFAULT | 8 | 2 | 4      # height, roll, pitch: plant_rollout_study.py's predicates
        S = mpc.open_loop_device(q0, np.zeros_like(q0), 1.0 - 0.5e-3, torque_layer=L, plant=GroundContact(), plant_substeps=2, terminate_mask=mask)
        alive = (mpc.failed.cpu().numpy() >> 8) == 0
        S = S.cpu().numpy().astype(np.float64)[alive][:, ::a.every]
        res["trot_rollouts"] = dict(rollouts=a.rollouts, survived=int(alive.sum()), rows_each=int(S.shape[1]) if alive.any() else 0)
        if alive.any() and np.isfinite(S).all():
            sets["trot_on_plant"] = rows_to_euler(S.reshape(-1, 44))

    res["gap"] = {}
    for name, (q, v) in sets.items():
        q32, v32 = q.astype(np.float32), v.astype(np.float32)      # what the device is handed
        com, h, _ = cr.centroidal_ref_batch(m, q32, v32)
        entry = dict(fp64_reference=gap(q32.astype(float), v32.astype(float), com, h))
        if L is not None:
            com_d, h_d = L.centroidal(q32, v32)
            entry["device"] = gap(q32.astype(float), v32.astype(float), com_d.cpu().numpy().astype(float), h_d.cpu().numpy().astype(float))
        res["gap"][name] = entry
        print(name, json.dumps(entry), file=sys.stderr, flush=True)

    if L is not None:
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
            return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))

        res["cost_ms"] = {}
        for B in (1024, 8192):
            r = np.random.default_rng(B)
            t32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=L.device)      # noqa: E731
            q = t32(stand + r.normal(0, 0.03, (B, 18)))
            v = t32(np.concatenate([r.normal(0, 0.3, (B, 6)), r.normal(0, 2.0, (B, 12))], axis=1))
            tau = t32(r.uniform(-5, 5, (B, 12)))
            res["cost_ms"][f"B{B}"] = dict(mass_matrix=timed(lambda: L.mass_matrix(q)), centroidal=timed(lambda: L.centroidal(q, v)),
                                           centroidal_with_Ag=timed(lambda: L.centroidal(q, v, jacobian=True)),
                                           com_only=timed(lambda: L.centroidal(q)),
                                           forward_dynamics=timed(lambda: L.forward_dynamics(q, v, tau)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
