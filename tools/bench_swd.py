"""Time of the sliced Wasserstein distance (utils/swd.py, csrc/swd.hip) at the paper's sizes.

    python tools/bench_swd.py [--out profiles/swd.json] [--samples 16384] [--patches 128] [--dirs 128] [--repeats 4]

For 32 x 32 and 64 x 64 random uint8 images: one build of the real side (utils.swd.SwdReal's loop) and one evaluation
(utils.swd.distances' loop) in one process, each split into its stages -- statistics (otgan_swd_channel_stats_u8), projection
(otgan_swd_project_u8), sort (torch.sort) and distance (otgan_swd_row_l1_f64; the real side's copy of the sorted rows is
counted there) -- with device events around every stage call, summed per stage.  `total_ms` is a host clock around the whole
loop, synchronised at both ends.  A first pass on 256 images loads the kernels.  The tool records; it sets no threshold."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from otgan_amd import ops  # noqa: E402
from otgan_amd.utils import swd  # noqa: E402


class Stages:
    def __init__(self):
        self.pairs = {}

    def run(self, name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.pairs.setdefault(name, []).append((a, b))
        return out

    def ms(self):
        torch.cuda.synchronize()
        return {k: round(sum(a.elapsed_time(b) for a, b in v), 3) for k, v in self.pairs.items()}


def one_side(images, pos, dirs, real_sorted=None):
    """The loop of SwdReal (real_sorted None: returns the kept rows) or of distances (returns the [L, nd] table), staged."""
    st = Stages()
    n, P, L = images.shape[0], pos.shape[2], pos.shape[0]
    chunk = swd.chunk_directions(n, P)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mean, inv_std = st.run("stats", lambda: ops.swd_channel_stats(images, pos))
    kept = []
    table = torch.empty(L, dirs.shape[0], dtype=torch.float64, device=images.device)
    for l in range(L):
        if real_sorted is None:
            kept.append(torch.empty(dirs.shape[0], n * P, dtype=torch.float32, device=images.device))
        for j0 in range(0, dirs.shape[0], chunk):
            d = dirs[j0:j0 + chunk]
            proj = st.run("projection", lambda: ops.swd_project(images, pos, l, mean, inv_std, d))
            rows = st.run("sort", lambda: torch.sort(proj, dim=1)[0])
            del proj
            if real_sorted is None:
                st.run("distance", lambda: kept[l][j0:j0 + rows.shape[0]].copy_(rows))
            else:
                table[l, j0:j0 + rows.shape[0]] = st.run("distance", lambda: ops.swd_row_l1(rows, real_sorted[l][j0:j0 + rows.shape[0]])) * 1e3
            del rows
    ms = st.ms()
    ms["total_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    return (kept if real_sorted is None else table), ms, chunk


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "swd.json"))
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--patches", type=int, default=128)
    ap.add_argument("--dirs", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=4)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "patches": args.patches,
           "directions": args.dirs * args.repeats,
           "timing": "device events around every stage call, summed per stage, one pass; total_ms: host clock around the loop",
           "cases": []}
    for S in (32, 64):
        g = torch.Generator().manual_seed(S)
        dirs = swd.directions(args.repeats, args.dirs, g).to(dev)
        for n in (256, args.samples):                       # the first pass loads the kernels and is not recorded
            pos_r, pos_g = swd.positions(n, S, args.patches, g).to(dev), swd.positions(n, S, args.patches, g).to(dev)
            gd = torch.Generator(device=dev).manual_seed(n)
            real = torch.randint(0, 256, (n, S, S, 3), generator=gd, device=dev, dtype=torch.uint8)
            fake = torch.randint(0, 256, (n, S, S, 3), generator=gd, device=dev, dtype=torch.uint8)
            kept, ms_real, chunk = one_side(real, pos_r, dirs)
            table, ms_eval, _ = one_side(fake, pos_g, dirs, kept)
            per = table.mean(dim=1).tolist()
            del kept, table
        case = {"S": S, "levels": swd.levels(S), "directions_per_chunk": chunk,
                "real_side_bytes": swd.levels(S) * dirs.shape[0] * args.samples * args.patches * 4,
                "real_side_build_ms": ms_real, "evaluation_ms": ms_eval, "swd_x1e3_of_two_random_sets": [round(v, 4) for v in per]}
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
