"""Rate of the probe's top-k launch (csrc/topk.hip) beside the k-NN launch it shares its block product with.

    python tools/bench_probe.py [--out profiles/probe_topk.json] [--reps 2]

Times, with device events around whole calls (every launch of a call, its workspace allocation included) and in one
process: `otgan_topk_dot_f64` and `otgan_knn_f64` at k = 3 without a threshold on the same synthetic unit-norm rows at
1000 x 5000 x 32768 (the DCGAN critic's width at 32 x 32) and 1000 x 5000 x 7296 (the DenseNet's), then
`otgan_topk_dot_f64` at k = 5 and k = 8 on the same rows.  The rate is 2 nq ny C / time, the best of `--reps` calls
after one call on 64 rows that loads the kernels."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from otgan_amd.utils import pr, probe  # noqa: E402

SHAPES = ((1000, 5000, 32768), (1000, 5000, 7296))


def rows(n, C, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, C, generator=g, device=dev)
    return x / x.norm(dim=1, keepdim=True)


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "probe_topk.json"))
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "timing": "device events around whole calls, best of reps",
           "cases": []}
    for nq, ny, C in SHAPES:
        q, y = rows(nq, C, 1, dev), rows(ny, C, 2, dev)
        calls = [("otgan_knn_f64", 3, lambda q=q, y=y: pr.knn(q, y, 3))]
        calls += [("otgan_topk_dot_f64", k, lambda q=q, y=y, k=k: probe.topk(q, y, k)) for k in (3, 5, 8)]
        for name, k, fn in calls:
            (pr.knn if name == "otgan_knn_f64" else probe.topk)(q[:64], y[:64], k)      # loads the kernels
            torch.cuda.synchronize()
            ms = timed(fn, args.reps)
            case = {"kernel": name, "nq": nq, "ny": ny, "C": C, "k": k, "ms": round(ms, 3),
                    "tflops": round(2.0 * nq * ny * C / (ms * 1e-3) / 1e12, 2)}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
        base = out["cases"][-4]["tflops"]
        for case in out["cases"][-3:]:
            case["rate_over_knn_k3"] = round(case["tflops"] / base, 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
