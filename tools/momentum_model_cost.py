#!/usr/bin/env python3
"""What the articulated momentum model of the whole-body solve costs, torch-event times on one device: one
`nmpc_shift_solve_batch` at B = 8192, N = 30 under the benchmark's policy (1 SQP x 6 IPM iterations, precision 0, full steps),
declared against articulated, on the same inputs, two handles side by side.
    python tools/momentum_model_cost.py [--B 8192] [--N 30] [--windows 5] [--calls 5] [--out FILE.json]
A window is `calls` back-to-back solves between two events, divided by `calls`; every solve starts from the same initial guess, so
the copy that restores X, U (2 x 17 MB at the default size) is inside the window, the same for both modes; one warm-up window, then `windows` timed ones per mode, interleaved; median and range as one JSON
line.  The yardstick is the parent commit's declared time: the declared kernels of this tree are the parent's instruction for
instruction (tools/asm_identity.py), so `declared` here is that time.  Nothing here asserts a time."""
import argparse, json, os, statistics, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from iterative_learning_nmpc_amd import workloads as wl
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = torch.device("cuda:0")
    w = wl.wholebody_trot(B=a.B, N=a.N, seed=0)
    layer = BatchedTorqueLayer(**wl.quadruped_tree(), device=dev)

    def setup(model):
        s = BatchedNmpcSolver(w.model_id, a.N, a.B, dev)
        s.set_model_params(w.mp)
        s.set_cost_weights(w.W, w.W_e, w.meta["reg"], w.meta["reg_e"])
        s.set_max_iter(1); s.set_max_qp_iter(6)
        if model == "articulated":
            s.set_momentum_model("articulated", torque_layer=layer)
        t = {k: s.to_device(getattr(w, k)) for k in ("x0", "yref", "yref_e", "params", "X", "U")}
        X0, U0 = t["X"].clone(), t["U"].clone()
        status = torch.empty(a.B, dtype=torch.int32, device=dev)
        stats = torch.empty(a.B, 4, dtype=torch.float32, device=dev)

        def call():
            t["X"].copy_(X0); t["U"].copy_(U0)
            s.solve(t["x0"], t["yref"], t["yref_e"], t["params"], t["X"], t["U"], status, stats)
        return call, status

    modes = {m: setup(m) for m in ("declared", "articulated")}

    def window(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.calls):
            call()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.calls

    ms = {k: [] for k in modes}
    for i in range(a.windows + 1):          # window 0 warms up; the modes alternate within every round
        for k, (call, _) in modes.items():
            t = window(call)
            if i:
                ms[k].append(t)
    res = dict(device=torch.cuda.get_device_name(0), B=a.B, N=a.N, windows=a.windows, calls=a.calls)
    for k, x in ms.items():
        st = modes[k][1]
        res[k] = dict(median_ms=round(statistics.median(x), 4), min_ms=round(min(x), 4), max_ms=round(max(x), 4),
                      failed=int(((st == 1) | (st == 4)).sum().item()))
    res["articulated_over_declared"] = round(res["articulated"]["median_ms"] / res["declared"]["median_ms"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
