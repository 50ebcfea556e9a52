#!/usr/bin/env python3
"""What observation and action history on the policy input costs, and what it does for a learner under randomisation it cannot
see in one row, on one device:
  1. torch-event times of `BatchedTorqueLayer.policy_rollout` (100 control steps of 20 substeps of 0.5 ms, an untrained policy of
     3 x 512 with BatchNorm) at B = 1024 and 8192 in three settings that alternate inside every run, so that drift of the device
     hits all of them alike: detached -- the launches of the parent commit's rollout --; a history of (1, 0) attached with the same
     47-input policy, the pure cost of the added launches; a history of (4, 3) with the correspondingly wider policy (215 inputs).
     Reported per control step;
  2. the effect: `--effect-batch` robots under `sample_delays` and `sample_payloads`, a memoryless and a (4, 3) policy that start
     from the same near-standing parameters (random hidden layers, the last layer scaled by 0.01, its bias the standing pose: NOT
     trained), each taken through the same `--iterations` of `learning.dagger_iteration` with the whole-body expert and then
     driven for 1 s under fresh draws of the two tables; the count that is never stamped as terminated.
    python tools/history_cost.py [--runs 5] [--batches 1024 8192] [--out FILE.json] [--no-effect] [--effect-batch 32] [--iterations 3]
One warm-up, then `runs` timed windows per variant; median and range as one JSON line.  Nothing here asserts a time or a count."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS, N_SUB, DT = 100, 20, 5e-4
DEEP = (4, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 8192])      # none given: the effect run alone
    ap.add_argument("--effect-batch", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-effect", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import learning
    from iterative_learning_nmpc_amd import torque as torque_mod
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact, history_width
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = "cuda:0"

    def timed_alternating(calls):
        for call in calls.values():
            call()
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(a.runs):
            for name, call in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                t1.record()
                torch.cuda.synchronize()
                ms[name].append(t0.elapsed_time(t1) / STEPS)
        return {name: dict(median=round(statistics.median(x), 5), min=round(min(x), 5), max=round(max(x), 5)) for name, x in ms.items()}

    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, unit="ms per control step", steps=STEPS)
    ground = GroundContact(tau_max=30.0)
    stand = np.tile([0.0, 0.7, -1.4], 4)
    t32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev)      # noqa: E731
    L = BatchedTorqueLayer(**quadruped_tree(), device=dev)

    def start(B, rng, spread):
        q0 = np.zeros((B, 18)); q0[:, 6:] = stand + rng.uniform(-spread, spread, (B, 12))
        q0 = t32(q0)
        q0[:, 2] -= L.foot_kinematics(q0)[0][:, :, 2].amin(dim=1) + 0.003      # the lowest foot 3 mm in the ground
        return q0

    for B in a.batches:
        rng = np.random.default_rng(B)
        q0, v0 = start(B, rng, 0.05), t32(rng.uniform(-0.2, 0.2, (B, 18)))
        goal = t32(np.tile([0.3, 0.0, 0.0], (B, 1)))
        narrow = DevicePolicy(47, 12, 3, 512, True, batch_max=B, seed=B)
        deep = DevicePolicy(history_width(*DEEP) + 3, 12, 3, 512, True, batch_max=B, seed=B)
        S0 = L.observe_rows(q0[:, None], v0[:, None], 0.0, N_SUB * DT)[:, 0]

        def run(policy, depths):
            L.set_history(None)
            if depths is not None:
                L.set_history(*depths, batch=B)
                L.reset_history(S0, q0)
            L.policy_rollout(policy, q0, v0, STEPS, DT, N_SUB, goal, ground=ground)

        out = timed_alternating({"detached_ms": lambda: run(narrow, None), "attached_1_0_ms": lambda: run(narrow, (1, 0)),
                                 "attached_4_3_ms": lambda: run(deep, DEEP)})
        L.set_history(None)
        out["attached_1_0_over_detached"] = round(out["attached_1_0_ms"]["median"] / out["detached_ms"]["median"], 4)
        out["attached_4_3_over_detached"] = round(out["attached_4_3_ms"]["median"] / out["detached_ms"]["median"], 4)
        res[f"B{B}"] = out
        del narrow, deep
    if not a.no_effect:
        from iterative_learning_nmpc_amd import wholebody as wbk
        from iterative_learning_nmpc_amd.database import DeviceDatabase
        from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
        B = a.effect_batch
        mpc = LocomotionMPC(print_info=False, device=dev, batch=B, force_reference="gravity_share", n_nodes=30)
        mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
        q0 = np.zeros((B, 18)); q0[:, 2] = 0.30; q0[:, 6:] = wbk.Q_HOME
        v0, goal = np.zeros((B, 18)), np.tile(np.float32([0.2, 0.0, 0.0]), (B, 1))
        effect = {}
        for name, depths in (("memoryless", None), ("history_4_3", DEEP)):
            n_state = 44 if depths is None else history_width(*depths)
            policy = DevicePolicy(n_state + 3, 12, 3, 256, True, batch_max=max(B, 256), seed=0)      # rollouts of B, training batches of 256
            theta, rm, rv = policy.get_parameters()
            theta[policy.items[-2][2]:policy.items[-2][2] + 12 * 256] *= 0.01
            theta[policy.items[-1][2]:] = t32(wbk.Q_HOME)
            policy.set_parameters(theta, rm, rv)
            db = DeviceDatabase(limit=1 << 16, n_state=n_state, norm_input=False, device=dev)
            rows = []
            for it in range(a.iterations):
                out = learning.dagger_iteration(mpc, L, db, policy, q0, v0, goal, 0.3, n_epoch=a.epochs, batch_size=256, lr=1e-3, seed=it,
                                                delays=torque_mod.sample_delays(B, 10 + it), payloads=torque_mod.sample_payloads(B, 20 + it),
                                                history=depths)
                rows.append(dict(n_rows=out["n_rows"], survived=int(out["survived"].sum()), last_loss=round(float(out["train_loss"][-1].mean()), 5)))
            test = learning.evaluate_policy(L, policy, None, q0, v0, goal, 1.0, delays=torque_mod.sample_delays(B, 99),
                                            payloads=torque_mod.sample_payloads(B, 98), history=depths)
            effect[name] = dict(iterations=rows, standing_1s=int(test["survived"].sum()), of=B,
                                mean_steps_survived=round(float(test["steps_survived"].float().mean()), 2))
        res["effect"] = dict(policy="near-standing start, not pre-trained", dagger_T=0.3, **effect)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
