#!/usr/bin/env python3
"""What the linearly implicit integrator of the contact plant costs, torch-event times on one device: one 10 ms
control step of `contact_step` at B = 1024 / 8192,
  1. explicit, dt = 0.5 ms x 20, on a library built from the parent commit (--parent-lib) and on this tree's library, in
     alternating windows -- existing behaviour requires the second to stay within the first one's own spread;
  2. implicit, dt = 1 ms x 10 and dt = 2 ms x 5, on this tree's library.
    python tools/implicit_cost.py [--parent-lib PATH/libnmpc_hip.so] [--windows 5] [--calls 20] [--out FILE.json]
A window is `calls` back-to-back calls between two events, divided by `calls`; one warm-up window, then `windows` timed ones per
variant, interleaved; median and range as one JSON line.  The parent's library is loaded beside this tree's and called through
its own C-ABI (the calls measured have the signatures they had).  Nothing here asserts a time."""
import argparse, ctypes, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd._lib import ptr, stream
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = torch.device("cuda:0")
    tree = quadruped_tree()
    L = BatchedTorqueLayer(**tree, device=dev)

    parent = None
    if a.parent_lib:                    # the parent's library, bound for the three calls used here
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in ("nmpc_torque_create", "nmpc_torque_destroy", "nmpc_contact_step_batch"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        f32 = lambda x, shape: np.ascontiguousarray(np.asarray(x, np.float32).reshape(shape))      # noqa: E731
        i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int32))                              # noqa: E731
        n, nf = len(tree["parent"]), len(tree["foot_joint"])
        arrays = dict(parent=i32(tree["parent"]), type=i32(tree["joint_type"]), axis=f32(tree["axis"], (n, 3)),
                      placement=np.ascontiguousarray(np.concatenate([f32(tree["placement_R"], (n, 9)), f32(tree["placement_p"], (n, 3))], axis=1)),
                      mass=f32(tree["mass"], (n,)), com=f32(tree["com"], (n, 3)), inertia=f32(tree["inertia"], (n, 6)),
                      foot_joint=i32(tree["foot_joint"]), foot_offset=f32(tree["foot_offset"], (nf, 3)))
        m = _lib.NmpcTreeModel()
        m.n_joints, m.n_actuated, m.n_feet = n, int(tree["n_actuated"]), nf
        for k, x in arrays.items():
            setattr(m, k, x.ctypes.data_as(ctypes.POINTER(ctypes.c_int if x.dtype == np.int32 else ctypes.c_float)))
        m.gravity = (ctypes.c_float * 3)(0.0, 0.0, -9.81)
        parent_h = ctypes.c_void_p()
        assert parent.nmpc_torque_create(ctypes.byref(m), 0, ctypes.byref(parent_h)) == 0

    res = dict(device=torch.cuda.get_device_name(0), windows=a.windows, calls=a.calls, parent=bool(parent))
    ground, cfg = GroundContact(), GroundContact().cfg()
    stand = np.tile([0.0, 0.7, -1.4], 4)
    for B in (1024, 8192):
        rng = np.random.default_rng(B)
        t32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev)      # noqa: E731
        q0 = np.zeros((B, 18)); q0[:, 6:] = stand + rng.uniform(-0.05, 0.05, (B, 12))
        q0 = t32(q0)
        q0[:, 2] -= L.foot_kinematics(q0)[0][:, :, 2].amin(dim=1) + 0.003      # the lowest foot 3 mm in the ground
        v0 = t32(rng.uniform(-0.2, 0.2, (B, 18)))
        A = t32(stand + rng.uniform(-0.05, 0.05, (B, 12)))
        out = [torch.empty(B, 18, device=dev) for _ in range(3)] + [torch.empty(B, 4, 3, device=dev), torch.empty(B, 12, device=dev)]

        def raw(lib, h, dt, n_sub):
            return lambda: lib.nmpc_contact_step_batch(h, B, n_sub, dt, ctypes.byref(cfg), ptr(q0), ptr(v0), None, ptr(A), 20.0, 1.5,
                                                       *[ptr(x) for x in out], stream(dev))

        def own(mode, dt, n_sub):
            def call():
                L.set_integrator(mode)
                return L.contact_step(q0, v0, dt, n_sub, q_des=A, ground=ground)
            return call

        variants = {"explicit_0.5ms_x20": own("explicit", 5e-4, 20), "implicit_1ms_x10": own("implicit", 1e-3, 10),
                    "implicit_2ms_x5": own("implicit", 2e-3, 5)}
        if parent:
            variants = {"parent_explicit_0.5ms_x20": raw(parent, parent_h, 5e-4, 20), **variants}

        def window(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                call()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / a.calls

        ms = {k: [] for k in variants}
        for w in range(a.windows + 1):      # window 0 warms up; the variants alternate within every round
            for k, call in variants.items():
                t = window(call)
                if w:
                    ms[k].append(t)
        row = {k: dict(median=round(statistics.median(x), 4), min=round(min(x), 4), max=round(max(x), 4)) for k, x in ms.items()}
        row["implicit_2ms_x5_over_explicit"] = round(row["implicit_2ms_x5"]["median"] / row["explicit_0.5ms_x20"]["median"], 3)
        row["implicit_1ms_x10_over_explicit"] = round(row["implicit_1ms_x10"]["median"] / row["explicit_0.5ms_x20"]["median"], 3)
        if parent:
            p, e = row["parent_explicit_0.5ms_x20"], row["explicit_0.5ms_x20"]
            row["explicit_within_parent_spread"] = bool(p["min"] <= e["median"] <= p["max"])
        res[f"B{B}"] = row
    L.set_integrator("explicit")
    if parent:
        parent.nmpc_torque_destroy(parent_h)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
