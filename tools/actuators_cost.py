#!/usr/bin/env python3
"""What an actuator per robot costs, and what rotor inertia does to the explicit step, on one device:
  1. torch-event times of `contact_track` (20 control steps of 2 substeps, B = 8192) under both integrators: with nothing attached
     and with a table of payloads alone -- the launches the parent commit makes too: run this file there for the baseline, in
     turns with this tree, and compare inside the spread of the repeats --, and with a table of actuators
     (`torque.sample_actuators`) alone and beside the payloads, one launch of the chain with a law, a payload and an actuator per
     lane;
  2. the settle experiment: the quadruped of tests/contact_reference.drop() dropped from 2 cm under the explicit step at
     dt = 0.5 ms and 1 ms for 1 s, one robot per armature 0, 0.005, 0.01, 0.02 kg m^2 (rows (KP, KD, 0, armature) of one table),
     and the largest |v| over the last 20 % of the run, read after every substep of that stretch.
    python tools/actuators_cost.py [--runs 5] [--batches 8192] [--out FILE.json] [--no-settle]
One warm-up, then `runs` timed windows; median and range as one JSON line.  Nothing here asserts a time or a speed."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMATURES = (0.0, 0.005, 0.01, 0.02)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[8192])
    ap.add_argument("--out", default="")
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import torque as torque_mod
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = "cuda:0"
    tables = hasattr(torque_mod, "sample_actuators")      # the parent commit has no actuators: the other two ways only

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
    t32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev)      # noqa: E731
    for B in a.batches:
        rng = np.random.default_rng(B)
        q0 = np.zeros((B, 18)); q0[:, 6:] = stand + rng.uniform(-0.05, 0.05, (B, 12))
        q0 = t32(q0)
        q0[:, 2] -= L.foot_kinematics(q0)[0][:, :, 2].amin(dim=1) + 0.003      # the lowest foot 3 mm in the ground
        v0 = t32(rng.uniform(-0.2, 0.2, (B, 18)))
        A = t32(stand + rng.uniform(-0.05, 0.05, (B, steps, 12)))
        loads = t32(torque_mod.sample_payloads(B, B))
        drives = t32(torque_mod.sample_actuators(B, B)) if tables else None
        q, v = q0.clone(), v0.clone()

        def reset():
            q.copy_(q0); v.copy_(v0)

        out = {}
        track = lambda: L.contact_track(q, v, A, dt, n_sub, ground=ground, record=False)      # noqa: E731
        for integrator in ("explicit", "implicit"):
            name = f"track_{integrator}"
            L.set_integrator(integrator)
            out[f"{name}_uniform_ms"] = timed(track, reset)
            L.set_payloads(loads)
            out[f"{name}_payloads_ms"] = timed(track, reset)
            if tables:
                L.set_actuators(drives)
                out[f"{name}_payloads_actuators_ms"] = timed(track, reset)
                L.set_payloads(None)
                out[f"{name}_actuators_ms"] = timed(track, reset)
                L.set_actuators(None)
                out[f"{name}_actuators_over_payloads"] = round(out[f"{name}_actuators_ms"]["median"] / out[f"{name}_payloads_ms"]["median"], 3)
            L.set_payloads(None)
            out[f"{name}_uniform_again_ms"] = timed(track, reset)
        L.set_integrator("explicit")
        res[f"B{B}"] = out
    if tables and not a.no_settle:
        from iterative_learning_nmpc_amd.trajectory_io import KD, KP
        from tests import contact_reference as cr
        d = cr.drop()
        n = len(ARMATURES)
        rows = t32([[KP, KD, 0.0, arm] for arm in ARMATURES])
        tau_ff, q_des = t32(np.tile(d["tau_ff"], (n, 1))), t32(np.tile(d["q_des"], (n, 1)))
        settle = {}
        for step in (5e-4, 1e-3):
            total = int(round(1.0 / step))
            head = int(round(0.8 * total))
            for attached in (True, False):
                L.set_actuators(rows if attached else None)
                qs, vs = t32(np.tile(d["q"], (n, 1))), t32(np.tile(d["v"], (n, 1)))
                qs, vs = L.contact_step(qs, vs, step, head, tau_ff=tau_ff, q_des=q_des, kp=KP, kd=KD)[:2]
                worst = torch.zeros(n, device=dev)
                for _ in range(total - head):
                    qs, vs = L.contact_step(qs, vs, step, 1, tau_ff=tau_ff, q_des=q_des, kp=KP, kd=KD)[:2]
                    worst = torch.maximum(worst, torch.nan_to_num(vs.abs(), nan=float("inf")).amax(dim=1))
                key = f"dt_{step * 1e3:g}ms" + ("" if attached else "_no_table")
                settle[key] = {f"armature_{arm:g}": float(w) for arm, w in zip(ARMATURES, worst.cpu())} if attached else float(worst[0])
        L.set_actuators(None)
        res["settle_tail_speed"] = settle
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
