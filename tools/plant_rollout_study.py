#!/usr/bin/env python3
"""The whole-body expert on the ground-contact plant, measured: does it stand, does it trot, what does it cost.
    python tools/plant_rollout_study.py [--batch 64] [--seconds 1.0] [--timing-batch 8192] [--timing-seconds 2.0] [--out FILE.json]
Behaviour, per command v_des = 0 and (0.3, 0, 0), B rollouts of `LocomotionMPC.open_loop_device(..., plant=GroundContact(),
plant_substeps=2)` with force_reference="gravity_share" from the standing start at Q_HOME: the surviving fraction under the
reference's predicates (solver, collision, height band, roll, pitch), the flag histogram, min / max base height over the
recorded rows, and -- a second run with the reference's push (50-70 N for 0.3 s from 0.2 s, rollout 0 unpushed) -- the
out-of-distribution fraction of the valid rollouts' rows on the 44-slot row at threshold 4.0.
Cost, torch-event time: `timing-batch` rollouts of `timing-seconds` with and without the plant on the same build, and
`contact_track` of 40 steps x 2 substeps against its chain of 40 `contact_step` launches at the same batch.
One JSON line; nothing here asserts a number."""
import argparse, json, os, sys, warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLAGS = dict(solver=1, roll=2, pitch=4, height=8, velocity_tracking=16, collision=32, joint_limit=64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--timing-batch", type=int, default=8192)
    ap.add_argument("--timing-seconds", type=float, default=2.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import wholebody as wbk
    from iterative_learning_nmpc_amd.config import TERMINATE_DEFAULT
    from iterative_learning_nmpc_amd.mpc import sample_pushes
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.parallel import learning_update, ood_threshold
    from iterative_learning_nmpc_amd.solver import tracking_error
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device"
    L = BatchedTorqueLayer(**quadruped_tree())
    mask = TERMINATE_DEFAULT | FLAGS["height"] | FLAGS["roll"] | FLAGS["pitch"]

    def controller(B, v_des):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mpc = LocomotionMPC(print_info=False, batch=B, force_reference="gravity_share")
        mpc.set_command(np.asarray(v_des, float), 0.0)
        return mpc

    def start(B):
        q0 = np.zeros((B, 18)); q0[:, 2] = 0.30; q0[:, 6:] = wbk.Q_HOME
        return q0, np.zeros((B, 18))

    def event_ms(call):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); call(); t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    res = dict(device=torch.cuda.get_device_name(0), batch=a.batch, seconds=a.seconds, plant_substeps=2, terminate_mask=mask)
    T = a.seconds - 0.5e-3                                   # the float clock then runs whole replanning intervals
    for name, v_des in (("stand", (0.0, 0.0, 0.0)), ("trot_0.3", (0.3, 0.0, 0.0))):
        B = a.batch
        q0, v0 = start(B)
        mpc = controller(B, v_des)
        S = mpc.open_loop_device(q0, v0, T, torque_layer=L, plant=GroundContact(), plant_substeps=2, terminate_mask=mask)
        f = mpc.failed.cpu().numpy()
        stamp = f >> 8
        alive = stamp == 0
        rows = S.shape[1]
        # rows before the termination of each rollout (all of them for a survivor): 40 per replan
        upto = np.where(alive, rows, np.minimum(stamp * mpc.replanning_steps, rows))
        z = S[:, :, 19].cpu().numpy()
        live = np.arange(rows)[None, :] < upto[:, None]
        entry = dict(replans=rows // mpc.replanning_steps, survived=float(alive.mean()), finite=bool(torch.isfinite(S).all()),
                     flags={k: int(((f & bit) != 0).sum()) for k, bit in FLAGS.items()},
                     first_termination_replan=int(stamp[~alive].min()) if (~alive).any() else None,
                     z_min=float(np.nanmin(np.where(live, z, np.nan))), z_max=float(np.nanmax(np.where(live, z, np.nan))),
                     z_end_of_survivors=[float(z[alive, -1].min()), float(z[alive, -1].max())] if alive.any() else None)
        push = sample_pushes(B, seed=(1000, 0), start=0.2, duration=0.3)
        push["force"][0] = 0.0
        mp = controller(B, v_des)
        Sp = mp.open_loop_device(q0, v0, T, push=push, torque_layer=L, plant=GroundContact(), plant_substeps=2, terminate_mask=mask).contiguous()
        valid = (mp.failed & mask) == 0
        err, _ = tracking_error(Sp, Sp[0].contiguous(), threshold=ood_threshold(44), ood_weight=5.0)
        ood, _ = learning_update(err, ood_threshold(44), 5.0, valid)
        entry["pushed"] = dict(valid=float(valid.float().mean()), nominal_valid=bool(valid[0]),
                               ood_fraction=float(ood[valid].float().mean()) if bool(valid.any()) else None)
        res[name] = entry
        print(name, json.dumps(entry), file=sys.stderr, flush=True)
    # cost
    B = a.timing_batch
    q0, v0 = start(B)
    Tt = a.timing_seconds - 0.5e-3
    times = {}
    for name, kw in (("plan_following", dict()), ("labels", dict(torque_layer=L)), ("plant", dict(torque_layer=L, plant=GroundContact(), plant_substeps=2))):
        ms = []
        for _ in range(2):                                   # the second run is the figure (code objects, allocator)
            mpc = controller(B, (0.3, 0.0, 0.0))
            mpc.solver._device_solver()
            ms.append(event_ms(lambda: mpc.open_loop_device(q0, v0, Tt, **kw)))
            del mpc
        times[name] = ms[-1]
    print("rollouts", json.dumps(times), file=sys.stderr, flush=True)
    res["rollouts"] = dict(batch=B, seconds=a.timing_seconds, ms=times, plant_over_plan_following=times["plant"] / times["plan_following"],
                           plant_over_labels=times["plant"] / times["labels"])
    dev = lambda x: torch.as_tensor(x, dtype=torch.float32, device="cuda:0")   # noqa: E731
    q, v = dev(q0), dev(v0)
    A = dev(np.tile(wbk.Q_HOME, (B, 40, 1)))
    g = GroundContact()

    def chain():
        qq, vv = q, v
        for k in range(40):
            qq, vv = L.contact_step(qq, vv, 5e-4, 2, q_des=A[:, k].contiguous(), ground=g)[:2]

    def track(record):
        L.contact_track(q.clone(), v.clone(), A, 5e-4, 2, ground=g, record=record)
    for fn in (chain, lambda: track(True), lambda: track(False)):
        fn()
    c, t, t0 = (min(event_ms(fn) for _ in range(5)) for fn in (chain, lambda: track(True), lambda: track(False)))
    res["track"] = dict(batch=B, steps=40, n_sub=2, chain_ms=c, track_ms=t, track_without_rows_ms=t0, chain_over_track=c / t)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
