#!/usr/bin/env python3
"""--augment (csrc/augment.hip, ops.augment): the two kernels alone and the training step with and without them (dev tool, GPU
box; beside tools/bench_input.py).

    python tools/bench_augment.py [--out DIR]    -> DIR/augment.json

kernels: device-event time of the forward and the backward launch, policy color,translation,cutout, at 512 images of 32 x 32 and
      of 64 x 64 (and at 256 of 32 x 32, the launches of a generator step).  After 10 warm-up launches, 7 runs of 50 launches
      each between two events; the median run, per launch.  Achieved GB/s against 8 bytes per element (one read, one write).
      Twice: on ONE pair of buffers (6 - 50 MB: they stay in the 256 MiB Infinity Cache, as a batch a step has just produced
      does) and rotating over enough pairs to exceed 320 MB (every launch reads HBM).
step: whole-step wall time of DCGAN 2 x 128, 100 Sinkhorn iterations, on a resident batch, with `augment` on and off in the
      same process, alternating, 3 runs each: 18 warm-up steps, then 60 steps between two device synchronisations.  Against it:
      what the step's augmentation launches cost alone -- a period of 6 steps holds one 512-row forward launch (critic step)
      and five times two 256-row forward launches and one 256-row backward launch (generator steps).
bench.py's flagship measurement is not involved."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from otgan_amd import _lib, ops  # noqa: E402
from otgan_amd.trainer import OTGAN, default_args  # noqa: E402

POLICY = "color,translation,cutout"
KERNEL_SHAPES = ((512, 32), (512, 64), (256, 32))
WARMUP, RUNS, LAUNCHES = 10, 7, 50
STEP_WARMUP, STEP_STEPS, STEP_RUNS = 18, 60, 3
ROTATE_BYTES = 320 << 20


def _event_ms(fn, pairs):
    """Median over RUNS of (time of LAUNCHES launches between two events) / LAUNCHES; launch i uses pair i % len(pairs)."""
    for i in range(WARMUP):
        fn(*pairs[i % len(pairs)])
    runs = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(LAUNCHES):
            fn(*pairs[i % len(pairs)])
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) / LAUNCHES)
    return statistics.median(runs), runs


def kernel_numbers(dev):
    L, out = _lib.lib(), []
    for rows, S in KERNEL_SHAPES:
        nbytes = rows * S * S * 3 * 8
        u = torch.rand(rows, 8, device=dev)
        row = {"rows": rows, "image_size": S, "mbytes_moved_per_launch": round(nbytes / 1e6, 2)}
        for where, npairs in (("cache_resident", 1), ("from_hbm", -(-ROTATE_BYTES // nbytes))):
            pairs = [(torch.rand(rows, S, S, 3, device=dev) * 2 - 1, torch.empty(rows, S, S, 3, device=dev)) for _ in range(npairs)]
            for name, entry in (("fwd", L.otgan_augment_fwd_f32), ("bwd", L.otgan_augment_bwd_f32)):
                def launch(a, b, entry=entry):
                    _lib.check(entry(a.data_ptr(), rows, S, u.data_ptr(), 7, b.data_ptr(), _lib.stream_ptr()), name)
                ms, runs = _event_ms(launch, pairs)
                row["%s_%s_us" % (name, where)] = round(ms * 1e3, 2)
                row["%s_%s_us_runs" % (name, where)] = [round(r * 1e3, 2) for r in runs]
                row["%s_%s_gbytes_per_s" % (name, where)] = round(nbytes / (ms * 1e-3) / 1e9, 1)
            row["buffer_pairs_" + where] = npairs
            del pairs
        print(json.dumps(row))
        out.append(row)
    return out


def _step_ms(dev, augment):
    torch.manual_seed(1)
    m = OTGAN(default_args(model="dcgan", batch_size=128, nr_gpu=2, nr_sinkhorn_iter=100, augment=augment), dev)
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


def step_numbers(dev, kernels):
    runs = {"off": [], "on": []}
    for _ in range(STEP_RUNS):
        for name, augment in (("off", ""), ("on", POLICY)):          # alternating: the same neighbours on the machine
            runs[name].append(_step_ms(dev, augment))
    res = {"workload": "OTGAN.step, dcgan, 256 images per step as 2 x 128, 100 Sinkhorn iterations, nr_gen_per_disc 5, a resident "
                       "32 x 32 batch, eager steps",
           "method": "%d runs per setting, alternating, in one process; per run %d warm-up steps, then the wall clock over %d steps "
                     "between two device synchronisations" % (STEP_RUNS, STEP_WARMUP, STEP_STEPS)}
    for name, r in runs.items():
        res[name] = {"ms_per_step_runs": [round(v, 4) for v in r], "ms_per_step": round(statistics.median(r), 4),
                     "spread_ms": round(max(r) - min(r), 4)}
    k = {(r["rows"], r["image_size"]): r for r in kernels}
    f512, f256, b256 = (k[(512, 32)]["fwd_cache_resident_us"], k[(256, 32)]["fwd_cache_resident_us"],
                        k[(256, 32)]["bwd_cache_resident_us"])
    alone = (f512 + 5 * (2 * f256 + b256)) / 6 / 1e3
    added = res["on"]["ms_per_step"] - res["off"]["ms_per_step"]
    res["added_ms_per_step"] = round(added, 4)
    res["augmentation_launches_alone_ms_per_step"] = round(alone, 4)
    res["added_within_launches_alone_plus_off_spread"] = added <= alone + res["off"]["spread_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    os.makedirs(a.out, exist_ok=True)
    dev = torch.device("cuda:0")
    assert ops.AUG_COLOR | ops.AUG_TRANSLATION | ops.AUG_CUTOUT == 7
    res = {"method_kernels": "device events around %d launches, median of %d runs after %d warm-up launches, per launch; policy %s; "
                             "GB/s = 8 bytes per element / time; cache_resident = one pair of buffers, from_hbm = rotating over "
                             "pairs that total more than %d MB" % (LAUNCHES, RUNS, WARMUP, POLICY, ROTATE_BYTES >> 20)}
    res["kernels"] = kernel_numbers(dev)
    res["step"] = step_numbers(dev, res["kernels"])
    print(json.dumps(res, indent=1))
    with open(os.path.join(a.out, "augment.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
