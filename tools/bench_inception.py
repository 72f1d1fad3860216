"""Throughput of the Inception evaluation network (utils/inception_net.py, csrc/inception.hip) on one GPU.

    python tools/bench_inception.py [--graph classify_image_graph_def.pb | .tgz | dir] [--batch 500] [--moments]

Without --graph it synthesizes the full 2015 topology with random weights (tests/inception_graphs.py: same layers,
same FLOP count).  Input: generator-like 32 x 32 images in [-1, 1] through probs_from_generator (the training hook's
path: resize to 299 x 299 and the affines in one kernel).  Prints img/s and TFLOP/s at the batch size, from the plan's
FLOP count and HIP-event timing after warm-up, and the projected time of one evaluation of the reference
(2 x 50 000 samples, train.py:245-272), as one JSON line.  --moments: also the time of one fp64 moment update of the
batch's pool_3 (utils/fid.py, csrc/moments.hip; HIP events, same run) beside the forward pass, and the wall time of the
host finalisation of one Frechet distance at that width (two eigh).
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
