#!/usr/bin/env python3
"""DenseNet at 64 x 64 (dev tool, GPU box; beside tools/bench_layers.py).

    python tools/bench_densenet64.py ab   [--out DIR] [--runs 7]    -> DIR/densenet64_growth_ab.txt
    python tools/bench_densenet64.py step [--out DIR] [--steps 24]  -> DIR/densenet64_step.json

ab:   one whole dense block, forward + backward through ops.dense_block_op -- the critic's first block at the configs[3]
      batch: 128 images of 64 x 64, C0 = 32, L = 16, F = 16, CReLU -- with the growth chains on the two-scaled-fp16-piece
      kernels (ops.DENSE_H2_AT_64 = True) and on the fp32 / three-piece kernels (False), the two routes alternating inside one
      process.  A run = `--iters` block passes between two device events after a warm-up of the route; reported: every run, the
      median per route and the max - min spread of the old route's runs.
step: the training step of configs[3] at the new size (256 images as 2 x 128, L = 200 Sinkhorn iterations, 5 : 1 mix,
      step graphs as the trainer's default) and the 32 x 32 step of the same box beside it; then one eager period under the
      library's per-launch profiler (class times), and the largest layers of the 64 x 64 nets one by one.
Neither changes bench.py's flagship measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from otgan_amd import _lib, ops  # noqa: E402
from oracle import nets_torch as NT  # noqa: E402  (variable shapes of the nets only)


def _block(dev, N, H, C0, L, F, seed=1):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randn(N, H, H, C0, generator=gen).to(dev).requires_grad_(True)
    params = []
    for k in range(L):
        params.append([(torch.randn(3, 3, 2 * (C0 + k * F), F, generator=gen) * 0.05).to(dev).requires_grad_(True),
                       (torch.rand(F, generator=gen) + 0.5).to(dev).requires_grad_(True),
                       (torch.randn(F, generator=gen) * 0.1).to(dev).requires_grad_(True)])
    dy = torch.randn(N, H, H, C0 + L * F, generator=gen).to(dev)
    return x0, params, dy


def _block_pass(x0, params, dy, C0):
    y = ops.dense_block_op(x0, (C0,), params, 3, ops.ACT["crelu"])
    grads = torch.autograd.grad(y, [x0] + [t for p in params for t in p], dy)
    ops.join_side_stream(grads)
    return y, grads


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def growth_ab(dev, out_dir, runs, iters):
    N, H, C0, L, F = 128, 64, 32, 16, 16
    x0, params, dy = _block(dev, N, H, C0, L, F)
    times = {True: [], False: []}
    outs = {}
    for route in (True, False):                 # warm both routes: code objects, prepared filters, allocator
        ops.DENSE_H2_AT_64 = route
        plan = ops._split_block_plan(N, H, H, C0, L, F, (C0,), ops.ACT["crelu"], dev)
        assert plan is not None and plan["h2"] == route, (route, plan and plan["h2"])
        for _ in range(3):
            y, grads = _block_pass(x0, params, dy, C0)
        torch.cuda.synchronize()
        outs[route] = [y.detach().clone()] + [g.detach().clone() for g in grads]
    for _ in range(runs):
        for route in (True, False):             # alternating: both routes see the same neighbours on the machine
            ops.DENSE_H2_AT_64 = route
            _block_pass(x0, params, dy, C0)
            times[route].append(_timed(lambda: _block_pass(x0, params, dy, C0), iters))
    rel = max(float((a.double() - b.double()).norm() / b.double().norm()) for a, b in zip(outs[True], outs[False]))
    med_new, med_old = statistics.median(times[True]), statistics.median(times[False])
    spread_old = max(times[False]) - min(times[False])
    keep = med_old - med_new > spread_old
    lines = [
        "Growth chains of a dense block at 64 x 64: two-scaled-fp16-piece kernels (h2, W = 64 instantiations) against the fp32 /",
        "three-piece kernels (old route).  One whole block, forward + backward through ops.dense_block_op:",
        f"N = {N}, H = W = {H}, C0 = {C0}, L = {L}, F = {F}, CReLU.  {runs} runs per route, alternating, {iters} passes per run,",
        "device events, ms per pass.",
        "",
        "h2 route  runs: " + " ".join(f"{t:.3f}" for t in times[True]),
        "old route runs: " + " ".join(f"{t:.3f}" for t in times[False]),
        f"median h2  {med_new:.3f} ms",
        f"median old {med_old:.3f} ms",
        f"spread of the old route's runs (max - min) {spread_old:.3f} ms",
        f"largest relative L2 difference between the routes' outputs / gradients {rel:.2e}",
        f"decision: median old - median h2 = {med_old - med_new:.3f} ms {'>' if keep else '<='} spread -> "
        + ("h2 route is the default at W = 64" if keep else "the plan stays on the old kernels at W = 64"),
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(out_dir, "densenet64_growth_ab.txt"), "w") as f:
        f.write(text)


def _step_ms(dev, size, steps, graph=None, h2_at_64=None):
    from otgan_amd.trainer import OTGAN, default_args
    if h2_at_64 is not None:                    # (None: the plan's committed choice)
        ops.DENSE_H2_AT_64 = bool(h2_at_64)
        ops.bump_weights_epoch()
    m = OTGAN(default_args(model="densenet", image_size=size, batch_size=128, nr_gpu=2, nr_sinkhorn_iter=200,
                           nr_gen_per_disc=5, step_graph=graph), dev)
    x = torch.rand(m.nb, size, size, 3, device=dev) * 2 - 1
    for _ in range(12):                         # two periods: the eager one that captures, one replayed
        m.step(x)
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(steps):                  # a multiple of the period: the 5 : 1 mix
            m.step(x)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / steps * 1e3)
    res = {"ms_per_step_runs": [round(t, 3) for t in runs], "ms_per_step": round(statistics.median(runs), 3),
           "images_per_s": round(m.nb / statistics.median(runs) * 1e3, 1), "num_features": int(m.num_features),
           "step_graphs": m.graphs is not None}
    # class times of one eager period (the profiler brackets every library launch: slower than the step above)
    _lib.prof_reset()
    _lib.prof_enable(True)
    for _ in range(6):
        m.step(x)
    torch.cuda.synchronize()
    pc = _lib.prof_collect()
    _lib.prof_enable(False)
    res["profiled_period_ms_per_step"] = {k: round(v["ms"] / 6, 3) for k, v in pc.items() if v["launches"]}
    res["profiled_period_launches_per_step"] = {k: round(v["launches"] / 6, 1) for k, v in pc.items() if v["launches"]}
    m.close()
    return res


def _layer_ms(dev, N, H, Cin, Cout, pre, stride, up):
    x = torch.randn(N, H, H, Cin, device=dev).requires_grad_(True)
    V = (torch.randn(3, 3, Cin * (2 if pre else 1), Cout, device=dev) * 0.05).requires_grad_(True)
    g = torch.ones(Cout, device=dev, requires_grad=True)
    b = torch.zeros(Cout, device=dev, requires_grad=True)
    y = ops.conv2d_op(x, V, g, b, stride=stride, upsample=up, preact=ops.ACT[pre])
    dy = torch.randn_like(y)

    def run():
        y = ops.conv2d_op(x, V, g, b, stride=stride, upsample=up, preact=ops.ACT[pre])
        ops.join_side_stream(torch.autograd.grad(y, [x, V, g, b], dy))

    for _ in range(3):
        run()
    return round(statistics.median(_timed(run, 5) for _ in range(5)), 3)


def step_numbers(dev, out_dir, steps):
    res = {"workload": "densenet, 256 images per step as 2 x 128, 200 Sinkhorn iterations, nr_gen_per_disc 5, synthetic data",
           "method": f"per size: 12 warm-up steps, then 5 runs of {steps} steps (host clock around a device synchronise), median; "
                     "the configurations one after the other in one process (64x64, 64x64 on the other growth route, 32x32), not alternated",
           "growth_route_at_64": "h2" if ops.DENSE_H2_AT_64 else "fp32 / three-piece"}
    default = bool(ops.DENSE_H2_AT_64)
    res["64x64"] = _step_ms(dev, 64, steps)
    res["64x64_other_growth_route"] = dict(_step_ms(dev, 64, steps, h2_at_64=not default),
                                           growth_route_at_64="fp32 / three-piece" if default else "h2")
    ops.DENSE_H2_AT_64 = default
    ops.bump_weights_epoch()
    res["32x32"] = _step_ms(dev, 32, steps)
    N = 128
    x0, params, dy = _block(dev, N, 64, 32, 16, 16)
    for _ in range(3):
        _block_pass(x0, params, dy, 32)
    # the layers' shapes from the nets' own variable inventory (V: 3 x 3 x Cin_eff x Cout; CReLU doubles Cin)
    L = 16
    dV = dict(NT.densenet_disc_shapes("crelu", L))
    gV = dict(NT.densenet_gen_shapes("crelu", L))
    rgb_in, trans = dV["conv2d_0"], dV[f"conv2d_{L + 1}"]             # critic: RGB-in, block 1, transition 64 -> 32
    up, rgb_out = gV[f"conv2d_{2 * L + 1}"], gV[f"conv2d_{3 * L + 2}"]  # generator: ..., upsample 32 -> 64, block 3, RGB-out
    res["largest_layers_64x64_fwd_bwd_ms"] = {
        "batch": N,
        "critic block 1 (64x64, 32 -> 288 channels, 16 growth layers)":
            round(statistics.median(_timed(lambda: _block_pass(x0, params, dy, 32), 5) for _ in range(5)), 3),
        f"critic transition 64 -> 32 ({trans[2] // 2} -> {trans[3]})": _layer_ms(dev, N, 64, trans[2] // 2, trans[3], "crelu", 2, False),
        f"generator upsample 32 -> 64 ({up[2] // 2} -> {up[3]})": _layer_ms(dev, N, 32, up[2] // 2, up[3], "crelu", 1, True),
        f"critic RGB-in 64x64 ({rgb_in[2]} -> {rgb_in[3]})": _layer_ms(dev, N, 64, rgb_in[2], rgb_in[3], None, 1, False),
        f"generator RGB-out 64x64 ({rgb_out[2] // 2} -> {rgb_out[3]})": _layer_ms(dev, N, 64, rgb_out[2] // 2, rgb_out[3], "crelu", 1, False),
    }
    print(json.dumps(res, indent=1))
    with open(os.path.join(out_dir, "densenet64_step.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ab", "step"])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=24)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    if a.steps < 6 or a.steps % 6:
        ap.error("--steps must be a multiple of 6: one period of the 5 : 1 mix")
    os.makedirs(a.out, exist_ok=True)
    _lib.lib()
    dev = torch.device("cuda:0")
    if a.what == "ab":
        growth_ab(dev, a.out, max(5, a.runs), a.iters)
    else:
        step_numbers(dev, a.out, a.steps)


if __name__ == "__main__":
    main()
