#!/usr/bin/env python3
"""What a delay per robot costs, and what it does to the expert on the plant, on one device:
  1. torch-event times at B = 8192, the un-delayed call of the same build as the baseline: `contact_track` (20 control steps of 2
     substeps) and a 1 s `policy_rollout` (100 control steps of 20 substeps of 0.5 ms, an untrained policy), each with nothing
     attached, with a table of delays (`torque.sample_delays`, 0 .. 2 control steps), and with nothing attached again.  The pass in
     front of a track moves 2 * B * n_steps * nu * 4 bytes plus the register;
  2. the effect: `--effect-batch` robots (64) trotting at 0.3 m/s for 1 s under the whole-body expert on the plant
     (`open_loop_device(..., plant=GroundContact(), plant_substeps=2)`, joints started within 0.02 rad of Q_HOME), every robot late
     by the same 0, 5, 10 and 20 simulation steps of 1 ms; the count that is never stamped as terminated.
    python tools/delays_cost.py [--runs 5] [--batches 8192] [--out FILE.json] [--no-effect]
One warm-up, then `runs` timed windows; median and range as one JSON line.  Nothing here asserts a time or a count."""
import argparse, json, os, statistics, sys, warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DELAYS_MS = (0, 5, 10, 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[8192])
    ap.add_argument("--effect-batch", type=int, default=64)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-effect", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import torque as torque_mod
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = "cuda:0"

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
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs)
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
        goal = t32(np.tile([0.3, 0.0, 0.0], (B, 1)))
        late = torque_mod.sample_delays(B, B)
        policy = DevicePolicy(47, 12, 3, 512, True, batch_max=B, seed=B)
        q, v = q0.clone(), v0.clone()

        def reset():
            q.copy_(q0); v.copy_(v0)
            if L._delays is not None:
                L.reset_delay_history(q0)

        calls = dict(track=lambda: L.contact_track(q, v, A, dt, n_sub, ground=ground, record=False),
                     rollout_1s=lambda: L.policy_rollout(policy, q0, v0, 100, dt, 20, goal, ground=ground, record=False))
        out = dict(pass_bytes_per_track=2 * B * steps * 12 * 4)
        for name, call in calls.items():
            out[f"{name}_ms"] = timed(call, reset)
            L.set_delays(late, work_rows=steps)
            out[f"{name}_delays_ms"] = timed(call, reset)
            L.set_delays(None)
            out[f"{name}_again_ms"] = timed(call, reset)
            out[f"{name}_delays_over_none"] = round(out[f"{name}_delays_ms"]["median"] / out[f"{name}_ms"]["median"], 4)
        res[f"B{B}"] = out
    if not a.no_effect:
        from iterative_learning_nmpc_amd import wholebody as wbk
        from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
        B = a.effect_batch
        q0 = np.zeros((B, 18)); q0[:, 2] = 0.30; q0[:, 6:] = wbk.Q_HOME + np.random.default_rng(0).uniform(-0.02, 0.02, (B, 12))
        effect = {}
        for ms in DELAYS_MS:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                mpc = LocomotionMPC(print_info=False, batch=B, force_reference="gravity_share")
            mpc.set_command(np.array([0.3, 0.0, 0.0]), 0.0)
            assert mpc.sim_dt == 1.0e-3
            L.set_delays(np.full(B, ms, np.int32))
            S = mpc.open_loop_device(q0, np.zeros((B, 18)), 1.0 - 0.5e-3, torque_layer=L, plant=GroundContact(), plant_substeps=2)
            L.set_delays(None)
            stamp = (mpc.failed >> 8).cpu().numpy()
            effect[f"{ms}_ms"] = dict(standing=int((stamp == 0).sum()), of=B, replans=S.shape[1] // mpc.replanning_steps,
                                      first_termination_replan=int(stamp[stamp > 0].min()) if (stamp > 0).any() else None)
        res["expert_trot_0.3_1s"] = effect
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
