#!/usr/bin/env python3
"""What input noise in training and the observed rows beside a rollout cost, on one device:
  1. torch-event times of one `DevicePolicy.train_epoch` at batch 1024 over a database of 1 M rows (`--rows`, `--epoch-batches`
     batches per call; the reference's network, 47 -> 3 x 512 with BatchNorm -> 12; normalised inputs): with nothing attached, with
     a vector of input noise (`torque.training_sigma` of a `torque.sample_noise` table), and -- with `--parent-lib` -- the detached
     call on a library built from the parent commit, loaded beside this tree's;
  2. torch-event times of `learning.evaluate_policy` at its defaults (1 s = 100 control steps of 20 substeps of 0.5 ms) at B = 8192
     with an untrained policy and a table of sensor noise: without and with `record_observed=True`, and the same call without O on
     the parent's library.
The variants alternate inside every run, so that drift of the device hits all of them alike.
    python tools/input_noise_cost.py [--runs 7] [--rows 1000000] [--epoch-batches 64] [--batch 8192] [--parent-lib PATH/libnmpc_hip.so] [--out FILE.json]
One warm-up, then `runs` timed windows per variant; median and range as one JSON line.  Nothing here asserts a time."""
import argparse, ctypes, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--epoch-batches", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import _lib, learning
    from iterative_learning_nmpc_amd import torque as torque_mod
    from iterative_learning_nmpc_amd.database import DeviceDatabase
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

    def ratios(out, base, names):
        for name in names:
            out[f"{name[:-3]}_over_{base[:-3]}"] = round(out[name]["median"] / out[base]["median"], 4)

    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, parent=bool(parent))
    t32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev)      # noqa: E731
    sigma = torque_mod.training_sigma(torque_mod.sample_noise(4096, 1))

    # 1. the training epoch
    n, batch, nb = a.rows, 1024, a.epoch_batches
    g = torch.Generator(device=dev).manual_seed(0)
    db = DeviceDatabase(n, norm_input=True, device=dev)
    db.append(torch.randn(n, 44, generator=g, device=dev), torch.randn(n, 12, generator=g, device=dev),
              vc_goals=torch.rand(n, 3, generator=g, device=dev) - 0.5)
    net = lambda: DevicePolicy(47, 12, 3, 512, True, batch_max=batch, seed=1)      # noqa: E731
    detached, attached = net(), net()
    attached.set_input_noise(sigma, seed=1)
    calls = {}
    if parent:
        old = made_on(parent, net)
        calls["parent_ms"] = lambda: old.train_epoch(db, batch, nb, 1e-3, 3)
    calls["detached_ms"] = lambda: detached.train_epoch(db, batch, nb, 1e-3, 3)
    calls["attached_ms"] = lambda: attached.train_epoch(db, batch, nb, 1e-3, 3)
    out = timed_alternating(calls)
    ratios(out, "detached_ms", ["attached_ms"])
    out["us_per_batch_added"] = round(1e3 * (out["attached_ms"]["median"] - out["detached_ms"]["median"]) / nb, 3)
    if parent:
        ratios(out, "parent_ms", ["detached_ms", "attached_ms"])
    res[f"train_epoch_rows{n}_batch{batch}_x{nb}"] = out
    del db, calls

    # 2. the rollout
    B = a.batch
    L = BatchedTorqueLayer(**quadruped_tree(), device=dev)
    ground = GroundContact(tau_max=30.0)
    rng = np.random.default_rng(B)
    q0 = np.zeros((B, 18)); q0[:, 6:] = np.tile([0.0, 0.7, -1.4], 4) + rng.uniform(-0.05, 0.05, (B, 12))
    q0 = t32(q0)
    q0[:, 2] -= L.foot_kinematics(q0)[0][:, :, 2].amin(dim=1) + 0.003      # the lowest foot 3 mm in the ground
    v0, goal = t32(rng.uniform(-0.2, 0.2, (B, 18))), t32(np.tile([0.3, 0.0, 0.0], (B, 1)))
    table = t32(torque_mod.sample_noise(B, B))
    layers = {"this": (L, DevicePolicy(47, 12, 3, 512, True, batch_max=B, seed=B))}
    if parent:
        layers["parent"] = (made_on(parent, lambda: BatchedTorqueLayer(**quadruped_tree(), device=dev)),
                            made_on(parent, lambda: DevicePolicy(47, 12, 3, 512, True, batch_max=B, seed=B)))
    run = lambda which, **kw: learning.evaluate_policy(*layers[which], None, q0, v0, goal, 1.0, ground=ground, noise=table, noise_seed=1, **kw)      # noqa: E731
    calls = {}
    if parent:
        calls["parent_ms"] = lambda: run("parent")
    calls["without_ms"] = lambda: run("this")
    calls["observed_ms"] = lambda: run("this", record_observed=True)
    out = timed_alternating(calls)
    ratios(out, "without_ms", ["observed_ms"])
    out["us_per_step_added"] = round(1e3 * (out["observed_ms"]["median"] - out["without_ms"]["median"]) / 100, 3)
    if parent:
        ratios(out, "parent_ms", ["without_ms", "observed_ms"])
    res[f"evaluate_policy_1s_B{B}"] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
