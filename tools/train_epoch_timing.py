#!/usr/bin/env python3
"""What the epoch call saves over the chain it fuses: samples/s of policy training from a device-resident database,
    chain:  per batch  policy.weighted_sample -> DeviceDatabase.batch -> DevicePolicy.train_step   (driven from Python)
    epoch:  DevicePolicy.train_epoch                                                               (one library call)
on the reference's network (47 -> 3 x 512 -> 12, BatchNorm) at batch 256 and 1024 and databases of 1e5 and 1e7 rows.
    python tools/train_epoch_timing.py [--rows 100000 10000000] [--batch 256 1024] [--n-batches 64] [--min-s 0.5] [--out FILE.json]
Both variants run in the same process on the same library, on one stream, timed with device events around `n-batches`
steps; after one warm-up each they alternate until each has at least `min-s` seconds and three windows of timed work.
Before timing, the epoch is compared with the chain run on the index sequence of one sampler call, from identical
parameters: the losses must be the same bits (the timed chain draws with a seed per batch, as its caller would).  Prints one
JSON line per (rows, batch) with the windows, median samples/s and spread of both variants and the ratio of the medians."""
import argparse, json, os, statistics, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 10000000])
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--n-batches", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    from iterative_learning_nmpc_amd.policy import DevicePolicy, weighted_sample
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run says nothing about time"
    dev = torch.device("cuda:0")
    lr, nb = 1e-3, a.n_batches
    lines = []
    for rows in a.rows:
        g = torch.Generator(device=dev).manual_seed(rows)
        db = DeviceDatabase(rows, device=dev)
        db.append(torch.randn(rows, 44, generator=g, device=dev), torch.randn(rows, 12, generator=g, device=dev),
                  vc_goals=torch.randn(rows, 3, generator=g, device=dev),
                  weights=torch.where(torch.rand(rows, generator=g, device=dev) < 0.15, 5.0, 1.0))
        w = db.weights[:rows]
        for batch in a.batch:
            pols = {k: DevicePolicy(47, 12, 3, 512, True, batch_max=batch, device=dev, seed=1) for k in ("chain", "epoch")}

            def chain(seed):
                # the loop a caller has to write without the epoch call: a sampler call per batch (it rebuilds the prefix sums
                # of the whole table: nothing can be kept between calls), a seed per batch
                out = []
                for t in range(nb):
                    idx = weighted_sample(w, batch, seed * nb + t)
                    out.append(pols["chain"].train_step(*db.batch(idx), lr))
                return torch.cat(out)

            def epoch(seed):
                return pols["epoch"].train_epoch(db, batch, nb, lr, seed)

            # warm-up, and the same bits: the epoch against the chain on the index sequence of ONE sampler call
            idx = weighted_sample(w, nb * batch, 0).reshape(nb, batch)
            ref = torch.cat([pols["chain"].train_step(*db.batch(idx[t].contiguous()), lr) for t in range(nb)])
            assert torch.equal(ref, epoch(0)), "chain and epoch disagree"
            run = {"chain": chain, "epoch": epoch}

            def window(k, seed):
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run[k](seed)
                t1.record()
                torch.cuda.synchronize()
                return t0.elapsed_time(t1) / 1e3

            times = {k: [] for k in run}
            seed = 1
            while any(sum(times[k]) < a.min_s or len(times[k]) < 3 for k in run):
                for k in run:
                    times[k].append(window(k, seed))
                seed += 1
            res = dict(rows=rows, batch=batch, n_batches=nb)
            for k in run:
                rate = [nb * batch / t for t in times[k]]
                res[k + "_windows_s"] = [round(t, 5) for t in times[k]]
                res[k + "_samples_per_s"] = round(statistics.median(rate))
                res[k + "_spread_samples_per_s"] = round(max(rate) - min(rate))
            res["epoch_over_chain"] = round(res["epoch_samples_per_s"] / res["chain_samples_per_s"], 3)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
        del db, w
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
