#!/usr/bin/env python3
"""--health_every (csrc/health.hip, ops.tensor_health / ops.plan_marginals, utils/health.py): the two kernels alone and a
reported training step against a plain one (dev tool, GPU box; beside tools/bench_augment.py).

    python tools/bench_health.py [--out DIR]    -> DIR/health.json

kernels: device-event time of ops.tensor_health over the REAL variable lists of the DCGAN and the DenseNet generator and critic
      (one segment per variable, as the trainer calls it): the gradient pass (no ref) and the parameter pass (ref = a copy of the
      flat parameter buffer), the wrapper's host work included, as a reported step pays it.  After 10 warm-up calls, 7 runs of
      50 calls each between two events; the median run, per call, and the spread of the runs.  Achieved GB/s against 4 bytes per
      element (8 with ref).  The tensors of one network are 1 - 50 MB: they stay in the 256 MiB Infinity Cache between calls, as
      gradients a step has just produced do.  ops.plan_marginals the same way on six N x N plans at N = 128 (the benchmarked
      2 x 128 step) and N = 2500 (the reference's 8 x 625).
step: whole-step wall time of DCGAN 2 x 128, 100 Sinkhorn iterations, on a resident batch, with every step reported
      (health_every 1) and with none (0), in the same process, alternating, 3 runs each: 18 warm-up steps, then 60 steps between
      two device synchronisations.  A reported step synchronises and reads its results back; the difference is the cost of ONE
      report, to be divided by --health_every for a run.
bench.py's flagship measurement is not involved."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from otgan_amd import ops  # noqa: E402
from otgan_amd.trainer import OTGAN, default_args  # noqa: E402

WARMUP, RUNS, CALLS = 10, 7, 50
STEP_WARMUP, STEP_STEPS, STEP_RUNS = 18, 60, 3


def _event_us(fn):
    for _ in range(WARMUP):
        fn()
    runs = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return statistics.median(runs), runs


def _row(name, fn, nbytes, **extra):
    us, runs = _event_us(fn)
    row = dict(extra, what=name, us_per_call=round(us, 2), us_runs=[round(r, 2) for r in runs],
               spread_us=round(max(runs) - min(runs), 2), mbytes_read=round(nbytes / 1e6, 3),
               gbytes_per_s=round(nbytes / (us * 1e-6) / 1e9, 1))
    print(json.dumps(row), flush=True)
    return row


def kernel_numbers(dev):
    out = []
    for model in ("dcgan", "densenet"):
        m = OTGAN(default_args(model=model, batch_size=4, nr_gpu=2, nr_sinkhorn_iter=10, step_graph=False), dev)
        for net, params in (("generator", m.gen_params), ("critic", m.disc_params)):
            n = sum(p.numel() for p in params)
            grads = [torch.randn_like(p) * 1e-3 for p in params]
            before = [p.detach().clone() for p in params]
            info = dict(model=model, net=net, variables=len(params), elements=n)
            out.append(_row("tensor_health(gradients)", lambda: ops.tensor_health(grads), 4 * n, **info))
            out.append(_row("tensor_health(parameters, refs)", lambda: ops.tensor_health(params, refs=before), 8 * n, **info))
        m.close()
    for N in (128, 2500):
        plans = torch.softmax(torch.randn(6, N, N, device=dev), 2)
        out.append(_row("plan_marginals", lambda: ops.plan_marginals(plans), 4 * plans.numel(), problems=6, rows=N))
    return out


def _step_ms(dev, every):
    torch.manual_seed(1)
    m = OTGAN(default_args(model="dcgan", batch_size=128, nr_gpu=2, nr_sinkhorn_iter=100, step_graph=False, health_every=every), dev)
    x = torch.rand(m.nb, 32, 32, 3, device=dev) * 2 - 1
    for _ in range(STEP_WARMUP):
        m.step(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEP_STEPS):
        m.step(x)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / STEP_STEPS * 1e3
    m.check_finite()
    m.close()
    return ms


def step_numbers(dev):
    runs = {"plain": [], "reported": []}
    for _ in range(STEP_RUNS):
        for name, every in (("plain", 0), ("reported", 1)):          # alternating: the same neighbours on the machine
            runs[name].append(_step_ms(dev, every))
    res = {"workload": "OTGAN.step, dcgan, 256 images per step as 2 x 128, 100 Sinkhorn iterations, nr_gen_per_disc 5, a resident "
                       "32 x 32 batch, eager steps; reported: health_every 1 (every step), plain: 0",
           "method": "%d runs per setting, alternating, in one process; per run %d warm-up steps, then the wall clock over %d steps "
                     "between two device synchronisations" % (STEP_RUNS, STEP_WARMUP, STEP_STEPS)}
    for name, r in runs.items():
        res[name] = {"ms_per_step_runs": [round(v, 4) for v in r], "ms_per_step": round(statistics.median(r), 4),
                     "spread_ms": round(max(r) - min(r), 4)}
    res["one_report_costs_ms"] = round(res["reported"]["ms_per_step"] - res["plain"]["ms_per_step"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    os.makedirs(a.out, exist_ok=True)
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "method": "%d warm-up calls, then %d runs of %d calls between two device events; median run per call" % (WARMUP, RUNS, CALLS),
           "kernels": kernel_numbers(dev), "step": step_numbers(dev)}
    print(json.dumps(res["step"]), flush=True)
    with open(os.path.join(a.out, "health.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
