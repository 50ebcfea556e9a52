#!/usr/bin/env python3
"""What sensor noise per robot costs, and what it does to a policy on the plant, on one device:
  1. torch-event times of `learning.evaluate_policy` at its defaults (1 s = 100 control steps of 20 substeps of 0.5 ms) at B = 8192
     with an untrained policy: with nothing attached, with a table of noise (`torque.sample_noise`), and -- with `--parent-lib` --
     the same un-noised call on a library built from the parent commit, loaded beside this tree's.  The variants alternate inside
     every run, so that drift of the device hits all of them alike;
  2. the effect: `--effect-batch` robots (1024) standing for 1 s under a policy, every robot with the same standard deviation
     `m x NOISE_SIGMA_MAX` on every group and no bias, for the multipliers `--sweep`; the count that is never stamped as
     terminated.  The policy is `--policy FILE.npz` (theta, running_mean, running_var of a 47 -> 3 x 512 with BatchNorm -> 12
     `DevicePolicy`: a trained one) or, without it, the near-standing policy of tools/label_states_cost.py -- random hidden layers, the
     last layer scaled by 0.01, its bias the standing pose -- which is NOT a trained policy and is reported as such.
    python tools/noise_cost.py [--runs 5] [--batches 8192] [--parent-lib PATH/libnmpc_hip.so] [--policy FILE.npz] [--out FILE.json] [--no-effect]
One warm-up, then `runs` timed windows per variant; median and range as one JSON line.  Nothing here asserts a time or a count."""
import argparse, ctypes, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWEEP = (0.0, 0.5, 1.0, 2.0, 4.0, 8.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[8192])
    ap.add_argument("--effect-batch", type=int, default=1024)
    ap.add_argument("--sweep", type=float, nargs="+", default=list(SWEEP))
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--policy", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-effect", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import _lib, learning
    from iterative_learning_nmpc_amd import torque as torque_mod
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = "cuda:0"
    here = _lib.load()
    parent = None
    if a.parent_lib:                    # the parent's library, bound for every symbol it has
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name, (res, args) in _lib.SIGNATURES.items():
            if hasattr(parent, name):
                getattr(parent, name).restype, getattr(parent, name).argtypes = res, args

    def made_on(lib, make):
        """an object of the Python layer whose handle lives in `lib`: the layer and the policy of a rollout must share a library"""
        _lib._lib = lib
        try:
            return make()
        finally:
            _lib._lib = here

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
                ms[name].append(t0.elapsed_time(t1))
        return {name: dict(median=round(statistics.median(x), 4), min=round(min(x), 4), max=round(max(x), 4)) for name, x in ms.items()}

    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, parent=bool(parent))
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
        table = t32(torque_mod.sample_noise(B, B))
        layers = {"this": (L, DevicePolicy(47, 12, 3, 512, True, batch_max=B, seed=B))}
        if parent:
            layers["parent"] = (made_on(parent, lambda: BatchedTorqueLayer(**quadruped_tree(), device=dev)),
                                made_on(parent, lambda: DevicePolicy(47, 12, 3, 512, True, batch_max=B, seed=B)))
        run = lambda which, **kw: learning.evaluate_policy(*layers[which], None, q0, v0, goal, 1.0, ground=ground, **kw)      # noqa: E731
        calls = {}
        if parent:
            calls["parent_ms"] = lambda: run("parent")
        calls["none_ms"] = lambda: run("this")
        calls["noise_ms"] = lambda: run("this", noise=table, noise_seed=1)
        out = timed_alternating(calls)
        out["noise_over_none"] = round(out["noise_ms"]["median"] / out["none_ms"]["median"], 4)
        if parent:
            out["none_over_parent"] = round(out["none_ms"]["median"] / out["parent_ms"]["median"], 4)
            out["noise_over_parent"] = round(out["noise_ms"]["median"] / out["parent_ms"]["median"], 4)
        res[f"B{B}"] = out
        del layers
    if not a.no_effect:
        B = a.effect_batch
        policy = DevicePolicy(47, 12, 3, 512, True, batch_max=B, seed=0)
        theta, rm, rv = policy.get_parameters()
        if a.policy:
            saved = np.load(a.policy)
            theta, rm, rv = (t32(saved[k]) for k in ("theta", "running_mean", "running_var"))
        else:
            theta[policy.items[-2][2]:policy.items[-2][2] + 12 * 512] *= 0.01
            theta[policy.items[-1][2]:] = t32(stand)
        policy.set_parameters(theta, rm, rv)
        rng = np.random.default_rng(0)
        q0, v0 = start(B, rng, 0.02), torch.zeros(B, 18, device=dev)
        goal = t32(np.zeros((B, 3)))
        sigma = np.zeros(44, np.float32)
        for g, slots in torque_mod.NOISE_GROUPS.items():
            sigma[slots] = torque_mod.NOISE_SIGMA_MAX[g]
        effect = {}
        for m in a.sweep:
            kw = dict(noise=torque_mod.noise_table(m * sigma, B=B), noise_seed=2) if m > 0 else {}
            out = learning.evaluate_policy(L, policy, None, q0, v0, goal, 1.0, ground=ground, **kw)
            steps = out["steps_survived"].cpu().numpy()
            effect[f"x{m:g}"] = dict(standing=int(out["survived"].sum()), of=B, mean_steps_survived=round(float(steps.mean()), 2))
        res["standing_1s"] = dict(policy="trained: " + os.path.basename(a.policy) if a.policy else "near-standing, not trained", sweep=effect)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
