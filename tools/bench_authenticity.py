"""Rate of the pixel-space neighbour search (csrc/pixnn.hip, int8 MFMA) beside the only neighbour search the tree had before
it, `otgan_topk_dot_f64` (csrc/topk.hip, fp64 MFMA) on the same rows converted to fp32.

    python tools/bench_authenticity.py [--out profiles/authenticity.json] [--runs 3] [--nq 10000] [--ny 50000]

Times whole host calls with device events (every launch of a call and its workspace included), in one process, on seeded
random uint8 rows: 10 000 queries x 50 000 bank rows at D = 3072 (32 x 32 x 3) and D = 12288 (64 x 64 x 3), k = 3.  After one
small call of each that loads the kernels and one untimed full call that grows the workspace, the two calls ALTERNATE --runs
times; every pair is recorded, the new call must be the faster one in EVERY pair (the exit status says so), and the ratio
written down is that of the medians.  int8 rate = 2 nq ny D / time; the share of peak is against INT8_DENSE_PEAK, twice the
chip's bf16 dense figure (the i8 MFMAs run the cycles of the bf16 form at twice the K).  Also timed: the one-off
`authenticity.radii` pass, 50 000 x 50 000 leave-one-out at D = 3072.  The two searches rank by different scores (distance,
inner product), so their outputs are not compared here; the int8 results are tested bit for bit in tests/."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from otgan_amd.utils import authenticity, probe  # noqa: E402

INT8_DENSE_PEAK = 5.0e15       # ops / s: 2 x the 2.5 PF bf16 dense specification
K = 3


def rows(n, D, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(0, 256, (n, D), generator=g, device=dev, dtype=torch.uint8)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rate(nq, ny, D, ms):
    ops = 2.0 * nq * ny * D
    return {"ms": round(ms, 3), "tops": round(ops / (ms * 1e-3) / 1e12, 2), "of_int8_dense_peak": round(ops / (ms * 1e-3) / INT8_DENSE_PEAK, 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "authenticity.json"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--ny", type=int, default=50000)
    ap.add_argument("--dims", type=int, nargs="+", default=[3072, 12288])
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_authenticity.py measures on an MI355X: no device is visible")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "k": K, "int8_dense_peak_ops": INT8_DENSE_PEAK,
           "timing": "device events around whole host calls, alternating, every pair listed", "cases": []}
    ok = True
    for D in args.dims:
        q, y = rows(args.nq, D, 1, dev), rows(args.ny, D, 2, dev)
        qf, yf = q.float(), y.float()
        new = lambda: authenticity.nearest(q, y, K)
        old = lambda: probe.topk(qf, yf, K)
        authenticity.nearest(q[:64], y[:64], K)
        probe.topk(qf[:64], yf[:64], K)
        new(), old()
        torch.cuda.synchronize()
        pairs = []
        for _ in range(args.runs):
            pairs.append({"nn_u8_ms": round(timed(new), 3), "topk_dot_f64_ms": round(timed(old), 3)})
        t_new = statistics.median(p["nn_u8_ms"] for p in pairs)
        t_old = statistics.median(p["topk_dot_f64_ms"] for p in pairs)
        faster = all(p["nn_u8_ms"] < p["topk_dot_f64_ms"] for p in pairs)
        ok = ok and faster
        case = {"nq": args.nq, "ny": args.ny, "D": D, "pairs": pairs, "otgan_nn_u8": rate(args.nq, args.ny, D, t_new),
                "otgan_topk_dot_f64": {"ms": round(t_old, 3), "tflops": round(2.0 * args.nq * args.ny * D / (t_old * 1e-3) / 1e12, 2)},
                "speedup_over_topk_dot_f64": round(t_old / t_new, 2), "new_faster_in_every_pair": faster}
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        del qf, yf
    D = args.dims[0]
    bank = rows(args.ny, D, 2, dev)
    authenticity.radii(bank[:256])
    torch.cuda.synchronize()
    ms = [timed(lambda: authenticity.radii(bank)) for _ in range(args.runs)]
    out["radii"] = dict(n=args.ny, D=D, runs_ms=[round(v, 3) for v in ms], **rate(args.ny, args.ny, D, statistics.median(ms)))
    print(json.dumps(out["radii"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not ok:
        sys.exit("otgan_nn_u8 was not the faster call in every pair")


if __name__ == "__main__":
    main()
