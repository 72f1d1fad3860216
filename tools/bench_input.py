#!/usr/bin/env python3
"""The input path of a training step: host gather + copy + flip against the device-resident uint8 store (dev tool, GPU box;
beside tools/bench_densenet64.py).

    python tools/bench_input.py [--out DIR]    -> DIR/input_path.json

prep: input preparation ALONE, no model.  Per step the host path does what train.main's loop does by default -- fancy-index
      the float32 set by the epoch's permutation, copy the batch from pageable memory, torch.where over a flipped copy -- and
      the device path what it does with --data_on_device: draw the flip mask, one `otgan_batch_from_u8_f32` launch
      (utils/data.py).  --synthetic stores (floats / uint8).  Wall clock over 50 steps between two device synchronisations (the
      host path is host-bound: device events alone would hide it), median of 5 repeats, at 2 x 128 and 8 x 625 images of
      32 x 32 and 2 x 128 of 64 x 64.
box:  the device path's box-downsample (stored side / image size = 2, 4), which the host path has no counterpart of: the same
      clock, 2 x 128 images of 32 x 32 from 64 x 64 and from 128 x 128 stores.
loop: `train.main` itself, DCGAN 2 x 128, 100 Sinkhorn iterations, --synthetic, on both paths: the clock starts when step 12
      is entered and stops when step 72 is entered (a device synchronisation at both), so it covers 60 steps and 60 input
      preparations of the real loop; images per second; the paths alternate, 3 runs each.
Neither changes bench.py's flagship measurement, which times `model.step` on a resident batch."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from otgan_amd import _lib, train  # noqa: E402
from otgan_amd.utils import data as udata  # noqa: E402

PREP_SHAPES = ((2, 128, 32, 50000), (8, 625, 32, 50000), (2, 128, 64, 20000))     # shards, B, image size, images in the set
BOX_SHAPES = ((2, 128, 32, 64, 20000), (2, 128, 32, 128, 5000))                    # shards, B, image size, stored side, images in the set
PREP_STEPS, PREP_REPEATS = 50, 5
LOOP_WARMUP, LOOP_STEPS, LOOP_RUNS = 12, 60, 3


def _steps(n, shards, B):
    """(first step of an epoch?, t) for ever: the epoch / batch structure of train.main's loop."""
    nr_batches = n // (shards * B)
    while True:
        for t in range(nr_batches):
            yield t == 0, t, nr_batches


def _host_prep(dev, shards, B, S, n):
    trainx = np.random.rand(n, S, S, 3).astype(np.float32) * 2 - 1
    state = {"it": _steps(n, shards, B), "inds": None}

    def step():
        first, t, nr_batches = next(state["it"])
        if first:
            state["inds"] = np.random.permutation(n)
        inds = state["inds"]
        rows = [inds[(t + s * nr_batches) * B:(t + s * nr_batches + 1) * B] for s in range(shards)]
        xb = torch.from_numpy(trainx[np.concatenate(rows)]).to(dev, non_blocking=True)
        return train.maybe_flip(xb)

    return step


def _device_prep(dev, shards, B, S, n, side=None):
    side = side or S
    ds = udata.DeviceDataset(np.random.randint(0, 256, (n, side, side, 3), dtype=np.uint8), dev, S)
    state = {"it": _steps(n, shards, B)}

    def step():
        first, t, nr_batches = next(state["it"])
        if first:
            ds.set_permutation(np.random.permutation(n))
        flip = torch.rand(shards * B, device=dev) < 0.5
        return ds.batch([(t + s * nr_batches) * B for s in range(shards)], B, flip)

    return step


def _wall_ms(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def prep_numbers(dev):
    out = []
    for shards, B, S, n in PREP_SHAPES:
        row = {"shards": shards, "batch_size": B, "image_size": S, "images_in_set": n,
               "batch_mbytes_fp32": round(shards * B * S * S * 3 * 4 / 1e6, 2)}
        for name, make in (("host", _host_prep), ("device", _device_prep)):
            np.random.seed(1)
            torch.manual_seed(1)
            step = make(dev, shards, B, S, n)
            for _ in range(5):
                step()
            runs = [_wall_ms(step, PREP_STEPS) for _ in range(PREP_REPEATS)]
            row[name + "_ms_per_step_runs"] = [round(t, 4) for t in runs]
            row[name + "_ms_per_step"] = round(statistics.median(runs), 4)
            del step
        row["device_not_above_host"] = row["device_ms_per_step"] <= row["host_ms_per_step"]
        print(json.dumps(row))
        out.append(row)
    return out


def box_numbers(dev):
    out = []
    for shards, B, S, side, n in BOX_SHAPES:
        np.random.seed(1)
        torch.manual_seed(1)
        step = _device_prep(dev, shards, B, S, n, side)
        for _ in range(5):
            step()
        runs = [_wall_ms(step, PREP_STEPS) for _ in range(PREP_REPEATS)]
        row = {"shards": shards, "batch_size": B, "image_size": S, "stored_side": side, "images_in_set": n,
               "device_ms_per_step_runs": [round(t, 4) for t in runs], "device_ms_per_step": round(statistics.median(runs), 4)}
        print(json.dumps(row))
        out.append(row)
    return out


def _loop_images_per_s(extra, save_dir):
    """One train.main run; the window between the entries of steps LOOP_WARMUP and LOOP_WARMUP + LOOP_STEPS."""
    from otgan_amd.trainer import OTGAN
    orig, stamps, calls = OTGAN.step, {}, [0]

    def step(self, x, *a, **k):
        if calls[0] in (LOOP_WARMUP, LOOP_WARMUP + LOOP_STEPS):
            torch.cuda.synchronize()
            stamps[calls[0]] = time.perf_counter()
        calls[0] += 1
        return orig(self, x, *a, **k)

    OTGAN.step = step
    try:
        m = train.main(["--synthetic", "--model", "dcgan", "--nr_gpu", "2", "--batch_size", "128", "--nr_sinkhorn_iter", "100",
                        "--max_steps", str(LOOP_WARMUP + LOOP_STEPS + 1), "--save_dir", save_dir] + extra)
    finally:
        OTGAN.step = orig
    sec = stamps[LOOP_WARMUP + LOOP_STEPS] - stamps[LOOP_WARMUP]
    return LOOP_STEPS * m.nb / sec, sec / LOOP_STEPS * 1e3


def loop_numbers(save_dir):
    runs = {"host": [], "device": []}
    for _ in range(LOOP_RUNS):
        for name, extra in (("host", []), ("device", ["--data_on_device"])):     # alternating: the same neighbours on the machine
            runs[name].append(_loop_images_per_s(extra, save_dir))
    res = {"workload": "train.main, dcgan, 256 images per step as 2 x 128, 100 Sinkhorn iterations, nr_gen_per_disc 5, "
                       "--synthetic (50000 images of 32 x 32)",
           "method": "%d runs per path, alternating; per run the wall clock between the entries of steps %d and %d of the loop "
                     "(device synchronised at both): %d steps and %d input preparations" % (LOOP_RUNS, LOOP_WARMUP,
                                                                                           LOOP_WARMUP + LOOP_STEPS, LOOP_STEPS, LOOP_STEPS)}
    for name, r in runs.items():
        ips = [x[0] for x in r]
        res[name] = {"images_per_s_runs": [round(v, 1) for v in ips], "images_per_s": round(statistics.median(ips), 1),
                     "ms_per_step": round(statistics.median(x[1] for x in r), 3),
                     "spread_images_per_s": round(max(ips) - min(ips), 1)}
    gain = res["device"]["images_per_s"] - res["host"]["images_per_s"]
    spread = max(res["host"]["spread_images_per_s"], res["device"]["spread_images_per_s"])
    res["device_minus_host_images_per_s"] = round(gain, 1)
    res["difference_exceeds_run_to_run_spread"] = abs(gain) > spread
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--what", choices=["all", "prep", "loop"], default="all")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    os.makedirs(a.out, exist_ok=True)
    _lib.lib()
    dev = torch.device("cuda:0")
    res = {"method_prep": "input preparation alone, no model: wall clock over %d steps between two device synchronisations, median "
                          "of %d repeats after 5 warm-up steps; host = fancy-index the float32 set, copy from pageable memory, "
                          "torch.where flip; device = flip mask + one otgan_batch_from_u8_f32 launch on the uint8 store; the "
                          "epoch's permutation is drawn (and, on the device path, uploaded) inside the timed steps that start an epoch"
                          % (PREP_STEPS, PREP_REPEATS)}
    if a.what in ("all", "prep"):
        res["prep"] = prep_numbers(dev)
        res["box"] = box_numbers(dev)
    if a.what in ("all", "loop"):
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            res["loop"] = loop_numbers(td)
    print(json.dumps(res, indent=1))
    with open(os.path.join(a.out, "input_path.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
