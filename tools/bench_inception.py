"""Throughput of the Inception evaluation network (utils/inception_net.py, csrc/inception.hip) on one GPU.

    python tools/bench_inception.py [--graph classify_image_graph_def.pb | .tgz | dir] [--batch 500] [--moments] [--kid] [--pr]

Without --graph it synthesizes the full 2015 topology with random weights (tests/inception_graphs.py: same layers,
same FLOP count).  Input: generator-like 32 x 32 images in [-1, 1] through probs_from_generator (the training hook's
path: resize to 299 x 299 and the affines in one kernel).  Prints img/s and TFLOP/s at the batch size, from the plan's
FLOP count and HIP-event timing after warm-up, and the projected time of one evaluation of the reference
(2 x 50 000 samples, train.py:245-272), as one JSON line.  --moments: also the time of one fp64 moment update of the
batch's pool_3 (utils/fid.py, csrc/moments.hip; HIP events, same run) beside the forward pass, and the wall time of the
host finalisation of one Frechet distance at that width (two eigh).  --kid: also the time of ONE `kid_sums` call of the
Kernel Inception Distance (utils/kid.py, csrc/kid.hip; HIP events, same run) at its usual setting -- 100 subsets of 1000
rows -- on two banks of max(batch, 1000) rows at the graph's pool_3 width (the network's pool_3 of random images when the
batch has 1000, pool_3-like synthetic rows otherwise), its fp64 rate counting 2 m^2 C 2 per subset, and its share of the
forward passes of the 50 000 samples it follows.  --pr: also the time of the four k-NN passes behind precision, recall,
density and coverage of one model (utils/pr.py, csrc/knn.hip; HIP events, same run) at --pr_rows generated and as many
real rows, K = 3 -- the radii of the real rows, those of the generated rows, generated against real, real against
generated -- its fp64 rate counting 2 nq ny C per pass, and its share of the same forward passes.  The yardstick of that
rate is kid_fp64_tflops of the same run (--kid): the same block product with a cheaper epilogue.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="")
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--image_size", type=int, default=32)
    ap.add_argument("--moments", action="store_true", help="time the FID moment update of the batch's pool_3 as well")
    ap.add_argument("--kid", action="store_true", help="time one KID kernel-sum call (100 subsets x 1000 rows) as well")
    ap.add_argument("--pr", action="store_true", help="time the four k-NN passes of precision / recall / density / coverage as well")
    ap.add_argument("--pr_rows", type=int, default=50000, help="rows per side for --pr")
    a = ap.parse_args()
    import torch
    from otgan_amd.utils import inception_net, tfgraph
    t0 = time.time()
    if a.graph:
        plan = inception_net.lower(tfgraph.load_graph(a.graph))
    else:
        import inception_graphs as G
        plan = inception_net.lower(tfgraph.parse_graph(G.full_graph()[1]))
    t_load = time.time() - t0
    dev = torch.device("cuda:0")
    net = inception_net.InceptionNet(plan, dev, batch_size=a.batch)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((a.batch, a.image_size, a.image_size, 3), generator=g, device=dev) * 2 - 1
    for _ in range(a.warmup):
        net.probs_from_generator(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        p = net.probs_from_generator(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    img_s = a.batch / (ms * 1e-3)
    out = {"metric": "inception_img_per_s", "value": round(img_s, 1), "batch": a.batch, "ms_per_batch": round(ms, 3),
           "tflops": round(plan.flops_per_image() * img_s / 1e12, 2), "gflop_per_image": round(plan.flops_per_image() / 1e9, 3),
           "eval_2x50000_s": round(100000 / img_s, 2), "convs": len(plan.convs()),
           "arena_gb": round(plan.arena_floats_per_image * 4 * a.batch / 1e9, 2), "lower_s": round(t_load, 2),
           "graph": a.graph or "synthesized full 2015 topology", "probs_finite": bool(torch.isfinite(p).all())}
    if a.moments:
        from otgan_amd.utils import fid
        C = plan.pool3_channels
        pool3 = net.run(x, 127.5, 127.5)[0]
        acc = fid.MomentAccumulator(C, dev)
        for _ in range(a.warmup):
            acc.update(pool3)
        torch.cuda.synchronize()
        reps = 20 * a.iters                                     # a short kernel: a longer window than the forward pass's
        e0.record()
        for _ in range(reps):
            acc.update(pool3)
        e1.record()
        torch.cuda.synchronize()
        mms = e0.elapsed_time(e1) / reps
        other = fid.MomentAccumulator(C, dev).update(net.run(x.flip(0).neg(), 127.5, 127.5)[0])
        ma, mb = acc.moments(), other.moments()
        t0 = time.time()
        d = fid.frechet_distance(*fid.stats_from_moments(*ma), *fid.stats_from_moments(*mb))
        out.update({"moments_ms_per_batch": round(mms, 4), "moments_share_of_forward": round(mms / ms, 5),
                    "moments_fp64_tflops": round(2.0 * a.batch * C * C / (mms * 1e-3) / 1e12, 2), "pool3_channels": C,
                    "allreduce_mb": round(8 * (C * C + C + 1) / 1e6, 1), "feature_gather_mb_50000": round(4 * 50000 * C / 1e6, 1),
                    "fid_finalise_s": round(time.time() - t0, 2), "fid_finite": bool(d == d and abs(d) != float("inf"))})
    if a.kid:
        from otgan_amd.utils import kid
        C, nsub, m = plan.pool3_channels, 100, 1000
        rows = max(a.batch, m)
        if a.batch >= m:
            banks = [net.run(x, 127.5, 127.5)[0], net.run(x.flip(0).neg(), 127.5, 127.5)[0]]
        else:       # non-negative, a scale per channel: the statistics of pool_3, not its values
            banks = [torch.rand((rows, C), generator=g, device=dev) * torch.rand((1, C), generator=g, device=dev) for _ in range(2)]
        xi, yi = kid.subset_indices(rows, m, nsub, 0, 0), kid.subset_indices(rows, m, nsub, 0, 1)
        xi, yi = torch.as_tensor(xi, device=dev), torch.as_tensor(yi, device=dev)
        for _ in range(a.warmup):
            sums = kid.kid_sums(banks[0], xi, banks[1], yi)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            sums = kid.kid_sums(banks[0], xi, banks[1], yi)
        e1.record()
        torch.cuda.synchronize()
        kms = e0.elapsed_time(e1) / a.iters
        v = kid.mmd2_from_sums(sums, m).cpu().numpy()
        forward_ms_50000 = ms * (50000 / a.batch)
        out.update({"kid_ms": round(kms, 3), "kid_fp64_tflops": round(nsub * 2.0 * m * m * C * 2 / (kms * 1e-3) / 1e12, 2),
                    "kid_share_of_eval": round(kms / forward_ms_50000, 5), "kid_subsets": nsub, "kid_subset_size": m,
                    "kid_bank_rows": rows, "kid_features": "pool_3 of the graph" if a.batch >= m else "synthetic",
                    "pool3_channels": C, "kid_mean": float(v.mean()), "kid_std": float(v.std())})
    if a.pr:
        from otgan_amd.utils import kid, pr
        C, n, K = plan.pool3_channels, a.pr_rows, 3
        if a.batch >= n:
            rows = [net.run(x, 127.5, 127.5)[0][:n], net.run(x.flip(0).neg(), 127.5, 127.5)[0][:n]]
        else:       # non-negative, one scale per channel for both sides: the statistics of pool_3, not its values
            scale = torch.rand((1, C), generator=g, device=dev)
            rows = [torch.rand((n, C), generator=g, device=dev) * scale for _ in range(2)]
        gen, real = (kid.FeatureBank(n, C, dev).append(r) for r in rows)
        del rows

        def passes():
            return pr.precision_recall(gen, real, K, real_radii=pr.radii(real.rows, K))

        for _ in range(min(a.warmup, 1)):
            passes()
        torch.cuda.synchronize()
        reps = max(a.iters // 2, 1)                             # about a second per repetition at 50 000 rows
        e0.record()
        for _ in range(reps):
            v = passes()
        e1.record()
        torch.cuda.synchronize()
        pms = e0.elapsed_time(e1) / reps
        out.update({"pr_ms": round(pms, 2), "pr_fp64_tflops": round(4 * 2.0 * n * n * C / (pms * 1e-3) / 1e12, 2),
                    "pr_share_of_eval": round(pms / (ms * (50000 / a.batch)), 5), "pr_rows": n, "pr_neighbours": K, "pr_passes": 4,
                    "pr_features": "pool_3 of the graph" if a.batch >= n else "synthetic", "pool3_channels": C,
                    "pr_values": [round(f, 4) for f in v]})
        if "kid_fp64_tflops" in out:
            out["pr_rate_over_kid_rate"] = round(out["pr_fp64_tflops"] / out["kid_fp64_tflops"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
