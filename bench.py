#!/usr/bin/env python3
"""Headline benchmark: OT-GAN training images/sec (CIFAR-10-shaped synthetic 32x32x3 data,
256 images per GPU, DCGAN generator + critic, 100 Sinkhorn iterations, 5:1 generator:critic
step mix) on N MI355X GPUs of one node.

    python bench.py --gpus 1 --steps 30 --warmup 6
    python bench.py --gpus 1 --steps 30 --warmup 6 --full             # + every secondary measurement below
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (see the field notes in DESIGN.md section "Measurement").  A plain run sets up, warms
up, times the K steps and prints the line; `--full` adds what the headline does not need: the per-rank exchange times
(`config.rank_times`), the profiled passes (`roofline`, `kernel_classes`), the other configurations (`secondary`) and the
CPU baseline (`cpu_baseline`).  `--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # same guide: v_mfma_f32_32x32x16_bf16 dense peak (~2.5 PF)
PEAK_HBM_GBPS = 8000.0


# What the arithmetic of the timed step is (kept next to the numbers it describes; VERDICT r4 weak #10: the round-4 text was stale)
_CONV_NOTE = ("fp32 tensors and fp32 accumulation everywhere; the Winograd-domain GEMMs (F(4x4,3x3)) multiply operands stored "
              "as two fp16 pieces of the power-of-two-scaled value (hi + lo = 22 significand bits; one scale per frequency from "
              "the tensor's largest magnitude) with three fp16 MFMAs per product (hi*hi, hi*lo, lo*hi): 7.5e-8 rel. L2 from the "
              "split on dot products (fp32 accumulation itself: 3e-7; a plain fp32 MFMA chain: 1.3e-6), layer parity vs fp64 at "
              "2e-5; OTGAN_WINO_PIECES=3 = three bf16 pieces (24 bits, six MFMAs; `secondary.three_bf16_pieces_24bit`), "
              "OTGAN_WINO_FP32=1 = the same transforms on the fp32 MFMA engine.  ")
_MATCH_NOTE = ("Matching GEMMs (cost, plan application) on two scaled fp16 pieces / three MFMAs per product like the convolutions "
               "at every size since round 5: Sinkhorn rows N <= 128 (this configuration at one GPU) in cost128_h2_kernel / "
               "plan_apply128_h2_kernel, which split the fp32 operands while staging them (a-priori scale 2^13: unit-length "
               "feature rows, plan entries <= 1); N >= 256 (64x64 configuration, every multi-GPU problem) on the pre-split "
               "operand engine.  OTGAN_MATCH_FP32=1 keeps them on the exact-fp32 MFMA engine (v_mfma_f32_32x32x2_f32); "
               "injected gradients 3.7e-6 ... 6.0e-6 rel. L2 vs fp64 at lambda = 500 either way "
               "(tests/test_matching_engine_accuracy_gpu.py)")
PRECISION_NOTE = {
    "dcgan": _CONV_NOTE + _MATCH_NOTE,
    "densenet": ("fp32 tensors and accumulation; dense blocks are cut into wide 3x3 convolutions of finished channel groups "
                 "(Winograd F(4x4,3x3) GEMMs on two scaled fp16 pieces, as in the DCGAN configuration) + short 16-output growth "
                 "chains whose forward, input gradient (gathered per slice) AND weight gradient run on two scaled fp16 pieces "
                 "(v_mfma_f32_16x16x32_f16 / 16x16x16_f16, three MFMAs per product; round 4); the stride-2 / upsampling "
                 "transitions are implicit GEMMs on two scaled fp16 pieces; RGB layers on the exact-fp32 MFMA engine.  " + _MATCH_NOTE),
    "fp32": "OTGAN_WINO_FP32=1: Winograd-domain GEMMs on the exact-fp32 MFMA engine.  " + _MATCH_NOTE,
}


def _time_steps(model, x, warmup, steps):
    import torch
    for _ in range(warmup):
        model.step(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.step(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def roofline_of(prof, model, ms_per_step_prof, steps, default_cfg, cfg_tag=None):
    """`roofline` object of the dominant kernel class of a profiled pass (otgan_prof_* HIP-event totals)."""
    conv = {k: prof[k] for k in ("conv_fwd", "conv_dgrad", "conv_wgrad")}
    dom = max(conv, key=lambda k: conv[k]["ms"])
    # The Winograd-domain batched GEMM is ONE kernel family serving all three conv classes (its
    # launches are also counted inside them, together with the transform kernels): when it carries
    # the step, the roofline is reported for its dominant variant.
    nested = {k: prof[k]["ms"] for k in ("wino_gemm", "wino_gemm_bf16x3") if k in prof}
    if nested:
        # (round 4: always the GEMM kernel when it ran -- a whole conv CLASS mixes kernels of two matrix pipes and the
        # transform kernels, its FLOP over one pipe's peak is not a roofline; DenseNet's class figure of round 3 was that)
        top = max(nested, key=nested.get)
        if nested[top] > 0:
            dom = top
    d = prof[dom]
    ach = d["flop"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 else 0.0
    # HBM traffic per launch of that kernel class: from the committed rocprofv3 PMC passes
    # (tools/pmc_bench.sh -> profiles/rNN_pmc_summary_<model>.json), not measurable in-process.
    traffic, traffic_src = None, None
    try:
        tag = model if (default_cfg or model == "densenet") else cfg_tag
        if tag is None:
            raise LookupError("no PMC summary for this configuration")
        for rnd in ("r06", "r05b", "r05", "r04", "r03", "r02", "r02b", "r01"):          # newest committed PMC summary of this configuration
            fn = os.path.join(ROOT, "profiles", f"{rnd}_pmc_summary_{tag}.json")
            if os.path.exists(fn):
                with open(fn) as f:
                    traffic = round(json.load(f)[dom]["hbm_bytes_per_launch"])
                traffic_src = (f"profiles/{rnd}_pmc_summary_{tag}.json: rocprofv3 --pmc passes of this command, "
                               "committed (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE); looked up, not measured in this run")
                break
    except Exception:
        pass
    # the kernels behind the class in a default run (profiles/r06_kernel_stats_*.csv: wino_bgemm_x3n_kernel<false> = NT,
    # forward / input-gradient GEMMs, <true> = t-leading, weight-gradient GEMMs; the three-piece build
    # OTGAN_WINO_PIECES=3 runs wino_bgemm_x3_kernel, the 256 x 256 tile, instead)
    three = os.environ.get("OTGAN_WINO_PIECES") == "3"
    kname = {"wino_gemm": "wino_bgemm_kernel (Winograd-domain GEMMs on the exact-fp32 MFMA engine)",
             "wino_gemm_bf16x3": ("wino_bgemm_x3_kernel (256x256 tile; operands as three bf16 pieces, 6 bf16 MFMA per product)" if three else
                                  "wino_bgemm_x3n_kernel<false|true> (256x128 tile, two workgroups per CU; operands as two scaled "
                                  "fp16 pieces, 3 fp16 MFMA per product)")}
    peak = PEAK_BF16_MFMA_TFLOPS if dom == "wino_gemm_bf16x3" else PEAK_F32_MFMA_TFLOPS
    r = {"bound": "mfma", "kernel": kname.get(dom, dom), "achieved": round(ach, 2),
         "peak": peak, "unit": "TFLOP/s",
         "frac": round(ach / peak, 4),
         # not measured in this run (PMC counters need rocprofv3's own passes): null here, the committed profile's figure beside it
         "traffic": None, "traffic_from_committed_profile": traffic, "traffic_source": traffic_src,
         "launches": d["launches"], "avg_ms": round(d["ms"] / max(d["launches"], 1), 4),
         "time_share_of_step": round(d["ms"] / (ms_per_step_prof * steps), 4),
         "pass": f"second pass of {steps} steps with per-launch HIP events "
                 f"({ms_per_step_prof:.3f} ms/step; the headline pass ran unprofiled)"}
    if dom == "wino_gemm_bf16x3":
        # three fp16 MFMAs (hi*hi, hi*lo, lo*hi) evaluate one product of the 22-bit operands: `frac` counts executed
        # matrix FLOP against the fp16 peak; products per second are fp32_equivalent_tflops
        per = 6 if os.environ.get("OTGAN_WINO_PIECES") == "3" else 3
        r["fp32_equivalent_tflops"] = round(ach / per, 2)
        r["mfma_per_product"] = per
    return r


def secondary(dev, a):
    """Driver-timed numbers for the other BASELINE configurations, measured in this process after the headline
    (unprofiled wall clock around whole calls, inputs resident in HBM):
      * the matching block alone (microseconds and TFLOP/s on 36*N^2*D; two-batch, lambda 500) at
        N = 128 / 256 (the single-GPU problems of configs[1] / [4]) and N = 1024 (the 8-GPU problem of
        configs[2], whole and as the 256 rows one rank of eight computes);
      * one DenseNet step (configs[3] shape: 256 img/GPU, 200 Sinkhorn iterations);
      * one 64x64 step (configs[4] shape: 512 img/GPU = two halves of 256, D = 131072)."""
    import torch
    from otgan_amd.trainer import OTGAN, default_args
    from otgan_amd.utils import matching
    sec = {}
    g = torch.Generator(device=dev).manual_seed(5)

    def feats(n, D, shift):
        c = torch.rand(32, D, device=dev, generator=g) + shift
        f = (c[torch.randint(0, 32, (n,), device=dev, generator=g)] + 0.1 * torch.randn(n, D, device=dev, generator=g)).abs()
        return torch.nn.functional.normalize(f, dim=1)

    blocks = []
    for N, D, L, rows in ((128, 32768, 100, None), (256, 131072, 100, None), (1024, 32768, 100, None),
                          (1024, 32768, 100, 256), (1024, 7296, 200, 256)):
        fa_flat = feats(2 * N, D, 0.0)
        fb_flat = torch.nn.functional.normalize(feats(2 * N, D, 0.5) ** 2, dim=1)
        fa, fb = list(torch.chunk(fa_flat, 2, 0)), list(torch.chunk(fb_flat, 2, 0))
        rr = None if rows is None else (0, rows)
        # three entry points: the reference's operator (four matched arrays + calc_distance statistics) and the
        # training-mode one the step calls (the injected gradients directly; generator steps need no data-side gradient)
        calls = {"four_matched_arrays": ((lambda: matching.get_matched_features(fa, fb, 500.0, L)) if rows is None else
                                         (lambda: matching.get_matched_features_rows(fa, fb, 500.0, L, 0, rows))),
                 "grads_generator_step": lambda: matching.matched_feature_grads(fa_flat, fb_flat, 500.0, L, need_b=False, rows=rr),
                 "grads_critic_step": lambda: matching.matched_feature_grads(fa_flat, fb_flat, 500.0, L, need_b=True, rows=rr)}
        case = {"N": N, "D": D, "iters": L, "rows": "all" if rows is None else rows}
        if rows is not None:
            # What rank 0 of 2N / rows ranks runs per step in the global matching scope (trainer._match): its three
            # [rows, N] cost row slices (the reference's sharding of the cost GEMMs, utils/matching.py:29-39), then -- on the
            # all-gathered six log-kernels -- the Sinkhorn problems and the plans applied to its own rows.  The all-gather
            # of the slices (6 N^2 floats in total) is NOT in this time; the assembled log-kernels are precomputed here.
            # The calls above, without precomputed log-kernels, make the library compute all six N x N costs itself:
            # more cost work than a rank does (labelled below).
            from otgan_amd import trainer as T
            W = 2 * N // rows
            own = lambda t, r: t[r * rows:(r + 1) * rows]
            allk = torch.stack([T.rank_log_kernel_slices(r, W, own(fa_flat, r), own(fb_flat, r), fa_flat, fb_flat, 500.0)
                                for r in range(W)], 0)
            K6 = T.assemble_log_kernels(allk, W)
            stack_path = T.rank_stack_ok(rows, fa_flat)
            if not stack_path:
                del allk

            def rank_step(need_b):
                if stack_path:      # what trainer._match runs since round 5: ONE split of the gathered features for both calls
                    return T.rank_matching_stack(0, W, rows, fa_flat, fb_flat, 500.0, L, need_b, gather=allk)
                T.rank_log_kernel_slices(0, W, own(fa_flat, 0), own(fb_flat, 0), fa_flat, fb_flat, 500.0)
                return matching.matched_feature_grads(fa_flat, fb_flat, 500.0, L, need_b=need_b, rows=rr, log_kernels=K6)
            calls["rank_generator_step"] = lambda: rank_step(False)
            calls["rank_critic_step"] = lambda: rank_step(True)
            case["ranks"] = W
            case["rank_path"] = "feature stack split once per step (matching.FeatureStack)" if stack_path else "one split per library call"
            case["note"] = ("us_rank_*: what one rank of %d runs (cost row slices + Sinkhorn + plans on its rows; slice "
                            "all-gather excluded); us / us_grads_*: the same rows WITHOUT precomputed log-kernels -- the "
                            "library computes all six N x N costs, not a rank's workload" % W)
        for tag, call in calls.items():
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            reps = 5
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / reps * 1e6
            if tag == "four_matched_arrays":
                # algorithmic FLOP: 12 N^2 D cost + 24 N^2 D plan application (rows variant: the rank's share of the latter)
                flop = 12.0 * N * N * D + 24.0 * N * N * D * (1.0 if rows is None else rows / (2.0 * N))
                case["us"] = round(us, 1)
                case["tflops"] = round(flop / us / 1e6, 1)
            else:
                case["us_" + tag] = round(us, 1)
        if not a.no_prof:
            # per kernel class of the training-mode call (HIP events around the library's launches): the cost GEMMs against THEIR
            # roofline -- at N = 128 the six Gram blocks read 4 x N x D x 4 B = 67 MB for 6.4 GFLOP of products (8 us of fp16
            # matrix work at peak, 11 us of HBM at 6.3 TB/s): HBM-bound, so GB/s is the figure of merit and the north star's
            # "MFMA utilisation of the cost-matrix kernel" applies from N = 1024 (768 FLOP per byte) on
            from otgan_amd import _lib
            step_call = calls.get("rank_critic_step", calls["grads_critic_step"])
            _lib.prof_reset()
            _lib.prof_enable(True)
            for _ in range(5):
                step_call()
            torch.cuda.synchronize()
            pc = _lib.prof_collect()
            _lib.prof_enable(False)
            kc = {}
            for cls in ("cost_gemm", "sinkhorn", "plan_apply"):
                v = pc[cls]
                if not v["launches"]:
                    continue
                e = {"us_per_call": round(v["ms"] * 1e3 / 5, 1), "launches_per_call": round(v["launches"] / 5, 1)}
                if v["bytes"] > 0:
                    # the library counts a GEMM's operand bytes per problem (every block is an operand of three of the six
                    # problems: L2-level bytes); the HBM floor reads each of the four [N, D] blocks once
                    e["operand_GBps"] = round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 0)
                    if cls == "cost_gemm" and rows is None:
                        uniq = 16.0 * N * D * 5
                        e["hbm_unique_GBps"] = round(uniq / (v["ms"] * 1e-3) / 1e9, 0)
                        e["frac_of_8TBps"] = round(uniq / (v["ms"] * 1e-3) / 8e12, 3)
                if v["flop"] > 0:
                    e["product_tflops"] = round(v["flop"] / (v["ms"] * 1e-3) / 1e12, 1)
                kc[cls] = e
            if "cost_gemm" in kc:
                ai = (12.0 * N * N * D if rows is None else 6.0 * rows * N * D) / (16.0 * N * D if rows is None else 12.0 * (rows + N) * D)
                kc["cost_gemm"]["bound"] = "hbm" if ai < 2500e12 / 3 / 6.3e12 else "mfma"
                kc["cost_gemm"]["flop_per_byte"] = round(ai, 1)
            if "sinkhorn" in kc:
                kc["sinkhorn"]["bound"] = "on-chip latency (barriers / inter-workgroup exchanges; no HBM or MFMA roofline applies)"
            case["kernel_classes_critic_step"] = kc
        blocks.append(case)
        K6 = allk = None
        del fa, fb, fa_flat, fb_flat
    sec["matching_block"] = {"unit": "microseconds per call (wall, 5 calls); `us` / `tflops` (on 12*N^2*D + 24*N^2*D*(rows/2N)): the "
                                     "reference's operator = four matched arrays; us_grads_*: the training-mode entry the step calls "
                                     "(otgan_matching_two_batch_grad_f32: injected gradients directly, closed-form distance); "
                                     "us_rank_*: the per-step matching work of one data-parallel rank (see the case's note)",
                             "cases": blocks}
    torch.cuda.empty_cache()
    for tag, kw, size, bpg, (w, k) in (
            # (warm-up = one whole period of the 5:1 schedule: every step kind has run once, in the order it recurs, before
            # the timed six -- with three warm-up steps the timed window still met first-time allocations of the caching
            # allocator: DenseNet 26.3 ms there against 25.1 ms after a full period)
            ("densenet_cfg4_shape", dict(model="densenet", nr_sinkhorn_iter=200), 32, 256, (6, 6)),
            ("dcgan_64x64_cfg5_shape", dict(model="dcgan", nr_sinkhorn_iter=100, image_size=64), 64, 512, (6, 6))):
        args = default_args(batch_size=bpg // 2, nr_gpu=2, sinkhorn_lambda=500.0, nr_gen_per_disc=5, seed=1, **kw)
        m = OTGAN(args, dev)
        xs = torch.rand(m.nb, size, size, 3, device=dev) * 2 - 1
        m.prepare_step_graphs(xs)
        per = _time_steps(m, xs, w, k)
        sec[tag] = {"images_per_sec": round(m.nb / per, 1), "ms_per_step": round(per * 1e3, 2), "img_per_gpu": bpg,
                    "step_graph": sorted(m.graphs.graphs) if m.graphs is not None else "off",
                    "steps": k, "warmup": w, "sinkhorn_iters": args.nr_sinkhorn_iter,
                    "note": "6 timed steps = 1 critic + 5 generator steps (the 5:1 mix), unprofiled wall clock"}
        if not a.no_prof:
            # the same six steps once more with per-launch HIP events: the configuration's own roofline object
            # (one stream in this pass, as in the headline's roofline pass: every launch has the device to itself)
            from otgan_amd import _lib
            m.fork_real_pass = m.fork_wgrad = False
            _lib.prof_reset()
            _lib.prof_enable(True)
            per_prof = _time_steps(m, xs, 0, k)
            prof = _lib.prof_collect()
            _lib.prof_enable(False)
            sec[tag]["roofline"] = roofline_of(prof, kw["model"], per_prof * 1e3, k, False, "dcgan64" if size == 64 else None)
            sec[tag]["roofline"]["pass"] += "; ONE stream in this pass (each launch has the device to itself)"
            sec[tag]["launches_per_step"] = round(sum(v["launches"] for c, v in prof.items() if not c.startswith("wino_gemm")) / k, 1)
        m.close()
        del m, xs
        torch.cuda.empty_cache()
    return sec


def project_eight_ranks(gen_ms, disc_ms, sec, link_gbps=76.8):
    """What the FIRST real 8-GPU line should look like, from this run's single-GPU measurements (a projection, never a
    result; SURVEY 8e partitioning).  Per rank and step: the 1-GPU step with its N = 128 matching call replaced
    by the rank-of-eight call at N = 1024 (measured here, `secondary.matching_block`), plus the exchanges over xGMI as a direct
    exchange on the seven links (each 153.6 GB/s bidirectional = `link_gbps` per direction): a feature all-gather moves
    33.5 MB per link, the cost-slice gather 3.1 MB, the gradient SUM 2 x 151 / 8 MB (reduce-scatter + all-gather).
    `exposed`: milliseconds the compute stream waits; `hidden`: milliseconds that run under compute."""
    cases = {(c["N"], c["D"], c["rows"]): c for c in sec.get("matching_block", {}).get("cases", [])}
    one, rank8 = cases.get((128, 32768, "all")), cases.get((1024, 32768, 256))
    if not one or not rank8 or "us_rank_generator_step" not in rank8:
        return None
    feat = 256 * 32768 * 4 / 1e6 / link_gbps                  # ms per feature all-gather (one 33.5 MB block per link)
    slices = 3 * 256 * 1024 * 4 / 1e6 / link_gbps + 0.03      # + one small-message latency
    red = {"gen": 2 * 151.0 / 8 / link_gbps, "disc": 2 * 138.0 / 8 / link_gbps}
    out = {"link_GBps_per_direction": link_gbps, "steps": {}}
    tot = {"serial": 0.0, "overlapped": 0.0}
    for kind, ms1, w in (("gen", gen_ms, 5), ("disc", disc_ms, 1)):
        if ms1 is None:
            return None
        extra = (rank8["us_rank_generator_step" if kind == "gen" else "us_rank_critic_step"] -
                 one["us_grads_generator_step" if kind == "gen" else "us_grads_critic_step"]) / 1e3
        # serial: both feature gathers, the slice gather and the whole all-reduce are waited for where they are issued.
        # overlapped: a generator step hides the real features' gather under the generator + second critic pass, and both
        # kinds hide three of the four gradient buckets under the backward pass (the last bucket leaves after it)
        ser = 2 * feat + slices + red[kind]
        ovl = (feat if kind == "gen" else 2 * feat) + slices + red[kind] / 4
        out["steps"][kind] = {"ms_1gpu": round(ms1, 3), "matching_extra_ms": round(extra, 3),
                              "serial": {"exposed_ms": round(ser, 3), "hidden_ms": 0.0, "step_ms": round(ms1 + extra + ser, 3)},
                              "overlapped": {"exposed_ms": round(ovl, 3), "hidden_ms": round(ser - ovl, 3),
                                             "step_ms": round(ms1 + extra + ovl, 3)}}
        tot["serial"] += w * (ms1 + extra + ser) / 6
        tot["overlapped"] += w * (ms1 + extra + ovl) / 6
    base = (5 * gen_ms + disc_ms) / 6
    for mode in tot:
        out[mode] = {"ms_per_step": round(tot[mode], 3), "images_per_sec": round(8 * 256 / tot[mode] * 1e3, 0),
                     "weak_scaling_efficiency": round(base / tot[mode], 3)}
    out["note"] = ("PROJECTION from single-GPU measurements (no multi-GPU run exists): the replicated N = 1024 matching call is the "
                   "largest non-scaling term; link rate is the per-direction xGMI figure, RCCL efficiency not modelled")
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, model, last):
    """What the last timed step computed, as a caller of OTGAN.step holds it afterwards: the step's matching distance and
    entropy, and the weights it left behind (the generator's and the critic's trainable variables, in creation order, and
    the generator's EMA shadows), each flattened to one float32 array.  Arrays are read after the timed window has been
    synchronised, so nothing here is timed.  If the arrays together exceed DUMP_LIMIT_BYTES, each weight array is cut to the
    same fraction of its elements by a fixed sample of positions (NumPy seed 0, sorted), the same from run to run."""
    import numpy as np
    import torch

    def flat(ts):
        return torch.cat([t.detach().reshape(-1).float() for t in ts]).cpu().numpy()

    arrays = {"distance": flat([torch.as_tensor(last["distance"])]),
              "entropy": flat([torch.as_tensor(last["entropy"])]),
              "generator_weights": flat(model.gen_params),
              "critic_weights": flat(model.disc_params),
              "generator_ema_weights": flat([model.ema.average(p) for p in model.gen_params])}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        # the scalars stay whole; the weight arrays share what is left of the limit
        big = {k: v for k, v in arrays.items() if v.size > 1}
        frac = (DUMP_LIMIT_BYTES - (total - sum(v.nbytes for v in big.values()))) / sum(v.nbytes for v in big.values())
        for k, v in big.items():
            idx = np.sort(np.random.RandomState(0).choice(v.size, int(v.size * frac), replace=False))
            arrays[k] = v[idx]
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), np.ascontiguousarray(v, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--model", type=str, default="dcgan")
    ap.add_argument("--batch_per_gpu", type=int, default=256)
    ap.add_argument("--nr_sinkhorn_iter", type=int, default=100)
    ap.add_argument("--matching_scope", type=str, default="global")
    ap.add_argument("--image_size", type=int, default=32)
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beside the headline: per-rank exchange times, the profiled passes "
                         "(`roofline`), the secondary configurations and the CPU baseline (off by default)")
    ap.add_argument("--no_cpu_baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no_prof", action="store_true", help="with --full: skip the second (profiled) pass that feeds `roofline`")
    ap.add_argument("--no_secondary", action="store_true",
                    help="with --full: skip the secondary measurements (matching block alone, DenseNet cfg4 shape, 64x64 cfg5 shape)")
    ap.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (distance, entropy, the updated "
                         "generator / critic / EMA weights) as DIR/<name>.npy in float32")
    a = ap.parse_args()

    import torch
    from otgan_amd import _lib, parallel
    from otgan_amd.trainer import OTGAN, default_args

    if a.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if a.gpus > 1 and not parallel.launched():
        # started plainly (the way the reference starts all its towers from one command, train.py:72-85): become
        # the launcher of one process per GPU and hand back the ranks' exit code
        try:
            sys.exit(parallel.self_launch(os.path.abspath(__file__), sys.argv[1:], a.gpus))
        except parallel.LaunchError as e:
            sys.exit(f"bench.py --gpus {a.gpus}: {e}")
    try:
        parallel.check_devices(a.gpus)
    except parallel.LaunchError as e:
        sys.exit(f"bench.py --gpus {a.gpus}: {e}")
    rank, world, local = parallel.init_from_env()
    if world != a.gpus:
        sys.exit(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={world} ranks; start it as "
                 f"`python bench.py --gpus {a.gpus}` (self-launching) or `python -m torch.distributed.run "
                 f"--nproc-per-node {a.gpus} bench.py --gpus {a.gpus}`")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    _lib.lib()

    # 256 images per GPU = 2 logical shards x 128 (the reference needs an even shard count,
    # train.py:34); weak scaling: nr_gpu = 2 * world logical shards.
    shards_per_rank = 2
    args = default_args(model=a.model, batch_size=a.batch_per_gpu // shards_per_rank,
                        nr_gpu=shards_per_rank * world, nr_sinkhorn_iter=a.nr_sinkhorn_iter,
                        sinkhorn_lambda=500.0, nr_gen_per_disc=5, matching_scope=a.matching_scope, seed=1,
                        image_size=a.image_size)
    model = OTGAN(args, dev)
    torch.manual_seed(1 + rank)
    x = torch.rand(model.nb, a.image_size, a.image_size, 3, device=dev) * 2 - 1   # synthetic batch in [-1,1]

    # one-off setup: the trainer replays whole steps as hipGraphs (trainer.GraphedSteps); capturing them takes one eager
    # period plus one step per kind -- done here, before the W warm-up steps, so that neither warm-up nor the timed window
    # contains a capture (they are training steps like any other: untimed, and reported in config.step_graph_setup_steps)
    graph_setup_steps = model.prepare_step_graphs(x)
    for _ in range(a.warmup):
        model.step(x)
    torch.cuda.synchronize()
    # the timed window starts on a critic step whatever W was (the reference's schedule, train.py:214: a critic step
    # when step % 6 == 0): K steps then hold ceil(K/6) critic steps; the mix is reported in `config`
    period = args.nr_gen_per_disc + 1
    model.step_counter = 0
    n_disc = -(-a.steps // period)
    # ---- pass 1 (the headline `value`): exactly K steps, NO per-launch profiling (one event per step boundary on the
    # compute stream -- no synchronisation -- gives the per-kind step times reported next to the wall-clock value)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    parallel.barrier()
    torch.cuda.synchronize()
    ms0 = torch.cuda.memory_stats(dev)
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(a.steps):
        last = model.step(x)
        marks[i + 1].record()
    torch.cuda.synchronize()
    parallel.barrier()
    dt = time.perf_counter() - t0
    ms1 = torch.cuda.memory_stats(dev)
    # device-level allocations (hipMalloc / hipFree by torch's caching allocator) INSIDE the timed window: 0 when the warm-up
    # left the allocator in its steady state; anything else means some steps paid for a synchronising hipMalloc (diagnostic)
    alloc_diag = {k: int(ms1.get(k, 0) - ms0.get(k, 0)) for k in ("num_device_alloc", "num_device_free", "num_alloc_retries")}
    graph_kinds = sorted(model.graphs.graphs) if model.graphs is not None else []    # (before the profiled pass runs eagerly)
    per_kind = {"disc": [], "gen": []}
    for i in range(a.steps):
        per_kind["disc" if i % period == 0 else "gen"].append(marks[i].elapsed_time(marks[i + 1]))
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if torch.distributed.get_backend() == "gloo" else dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, model, last)
    # ---- pass 1b (--full, ranks > 1 only; never mixed into `value`): the same K steps with the exchange regions of the step
    # bracketed by events on every rank's compute stream (trainer.enable_timers): per-rank matching / all-gather / all-reduce
    # milliseconds per step, so that a first real scaling curve can be read (what grows with the rank count is there)
    rank_times = None
    if a.full and (world > 1 or model.collectives):
        model.enable_timers(True)
        model.step_counter = 0
        parallel.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(a.steps):
            model.step(x)
        mine = model.collect_timers(a.steps)
        mine["ms_per_step"] = round((time.perf_counter() - t1) / a.steps * 1e3, 3)
        mine["rank"] = rank
        model.enable_timers(False)
        if world > 1:
            allt = [None] * world
            torch.distributed.all_gather_object(allt, mine)
            rank_times = allt
        else:
            rank_times = [mine]
    # ---- pass 2 (--full; feeds `roofline` / `kernel_classes` only): the same K steps with every library launch
    # bracketed by HIP events on its launch stream (otgan_prof_*).  Never mixed into `value`.
    # Two sub-passes since the step runs on two streams (round 5): (2a) the schedule of the headline pass -- the GEMM's
    # launches overlap HBM-bound transform kernels of the other stream, so their event-bracketed durations are those of a
    # kernel SHARING the device (reported as `roofline.two_stream`); (2b) the same K steps with the second stream off: every
    # launch has the device to itself, which is what a kernel-vs-pipe roofline means (`roofline.achieved` / `frac`).
    prof, dt_prof, prof_ovl, dt_ovl = None, None, None, None
    if a.full and not a.no_prof:
        def _prof_pass():
            _lib.prof_reset()
            _lib.prof_enable(True)
            model.step_counter = 0
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(a.steps):
                model.step(x)
            torch.cuda.synchronize()
            d = time.perf_counter() - t1
            p = _lib.prof_collect()
            _lib.prof_enable(False)
            return p, d
        forks = (model.fork_real_pass, model.fork_wgrad)
        if any(forks):
            prof_ovl, dt_ovl = _prof_pass()
            model.fork_real_pass = model.fork_wgrad = False
        prof, dt_prof = _prof_pass()
        model.fork_real_pass, model.fork_wgrad = forks
    parallel.barrier()

    if rank != 0:
        return
    default_cfg = a.model == "dcgan" and a.image_size == 32 and a.batch_per_gpu == 256
    cfg_tag = ("configs[1]" if default_cfg else "configs[3]-shaped (DenseNet)" if a.model == "densenet"
               else "configs[4]-shaped (64x64)" if a.image_size == 64 else "custom")
    images = world * model.nb * a.steps
    value = images / dt
    out = {
        "metric": "OT-GAN train images/sec (CIFAR-10 32x32, bs=256/GPU)",
        "value": round(value, 2), "unit": "images/sec", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32 (Winograd-domain GEMMs on the fp16 matrix pipe with operands split into two scaled fp16 pieces = 22 significand bits, fp32 accumulate; errors at or below the fp32 MFMA chain's)" if a.model == "dcgan" else "f32", "data": "synthetic",
        "config": {"workload": f"{cfg_tag}: {a.model.upper()} generator+critic train step, synthetic "
                               f"CIFAR-10-shaped {a.image_size}x{a.image_size}x3, {a.batch_per_gpu} img/GPU as 2 logical shards x "
                               f"{a.batch_per_gpu // 2} (Sinkhorn rows N={world * a.batch_per_gpu // 2 if a.matching_scope == 'global' else a.batch_per_gpu // 2}), "
                               f"{a.nr_sinkhorn_iter} Sinkhorn iters, lambda 500, 5:1 generator:critic steps, Adam",
                   "global_batch": world * a.batch_per_gpu, "parallelism": f"dp{world}",
                   "ranks": parallel.world_size(),
                   "backend": (torch.distributed.get_backend() + (" (RCCL)" if torch.distributed.get_backend() == "nccl" else
                                                                  " (all ranks on cuda:0, logic test)" if parallel.single_device_mode() else "")
                               if torch.distributed.is_initialized() else "none (single process)"),
                   "sinkhorn_rows": model.sinkhorn_rows(),
                   "step_graph": (("hipGraph replay of whole steps, kinds captured: " + ", ".join(graph_kinds)) if graph_kinds else
                                  "off (eager launches)"),
                   "step_graph_setup_steps": graph_setup_steps,
                   "matching_scope": model.scope,
                   "step_mix": {"critic_steps": n_disc, "generator_steps": a.steps - n_disc,
                                "critic_ms_each": [round(v, 3) for v in per_kind["disc"]],
                                "device_allocations_in_window": alloc_diag,
                                "critic_ms": round(sum(per_kind["disc"]) / max(1, len(per_kind["disc"])), 3),
                                "generator_ms": (round(sum(per_kind["gen"]) / len(per_kind["gen"]), 3) if per_kind["gen"] else None),
                                "note": "timed window starts on a critic step; the reference's schedule is 1 critic : "
                                        f"{args.nr_gen_per_disc} generator steps (train.py:24,214)"},
                   **({"collectives": "forced (RCCL, world size 1)"} if (world == 1 and model.collectives) else {}),
                   "collectives_mode": (f"{model.collectives_mode}: {parallel.collectives_mode_reason()}"
                                        if model.collectives else "none (single process, no collectives)"),
                   **({"rank_times": {"per_rank": rank_times,
                                      "note": "separate pass of the same K steps with events around the exchange regions on each rank's "
                                              "compute stream (ms per step, mean over the step mix): matching_ms = the rank's cost row "
                                              "slices + the Sinkhorn problems + the plans applied to its rows; allgather_ms = feature and "
                                              "cost-slice all-gathers as the stream waits for them; allreduce_ms = the gradient SUM"}}
                      if rank_times else {}),
                   "last_distance": float(last["distance"]), "last_entropy": float(last["entropy"]),
                   "precision_note": PRECISION_NOTE[a.model if os.environ.get("OTGAN_WINO_FP32") != "1" else "fp32"]},
    }
    if prof:
        out["roofline"] = roofline_of(prof, a.model, dt_prof / a.steps * 1e3, a.steps, default_cfg,
                                      "dcgan64" if (a.model == "dcgan" and a.image_size == 64) else None)
        if prof_ovl:
            ro = roofline_of(prof_ovl, a.model, dt_ovl / a.steps * 1e3, a.steps, default_cfg, None)
            out["roofline"]["pass"] += ("; ONE stream in this pass (OTGAN_SIDE_STREAM=0 schedule): each launch has the device to "
                                        "itself -- the kernel against its pipe")
            out["roofline"]["two_stream"] = {
                "achieved": ro["achieved"], "frac": ro["frac"], "avg_ms": ro["avg_ms"], "launches": ro["launches"],
                "ms_per_step": round(dt_ovl / a.steps * 1e3, 3),
                "note": "the same kernel's launches bracketed by events in the DEFAULT two-stream schedule of the headline pass: "
                        "they share the device with the HBM-bound transform kernels of the other stream, so each launch takes "
                        "longer while the step gets shorter; not a kernel-vs-pipe figure"}
        out["kernel_classes"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3),
                                     "tflops": round(v["flop"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 and v["flop"] > 0 else None}
                                 for k, v in prof.items() if v["launches"]}
        # wino_gemm launches are nested inside the conv classes: not added again
        out["kernel_time_frac_of_wall"] = round(sum(v["ms"] for k, v in prof.items() if not k.startswith("wino_gemm")) / (dt_prof * 1e3), 4)
    if a.full and world == 1 and not a.no_secondary:
        model.close()
        del model, x
        torch.cuda.empty_cache()
        out["secondary"] = secondary(dev, a)
        if default_cfg:
            sm = out["config"]["step_mix"]
            proj = project_eight_ranks(sm["generator_ms"], sm["critic_ms"], out["secondary"])
            if proj is not None:
                out["config"]["projected_8_ranks"] = proj
            # the headline configuration with the convolution GEMMs on three bf16 pieces per operand element (24
            # significand bits, six MFMAs per product: the scheme before the two-piece fp16 operands) -- a fresh process
            # (OTGAN_WINO_PIECES=3), the same unprofiled timing; not the headline, a reference point for the trade
            import subprocess
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup),
                                    "--no_secondary", "--no_cpu_baseline", "--no_prof"], capture_output=True, text=True,
                                   timeout=300, env=dict(os.environ, OTGAN_WINO_PIECES="3"))
                line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
                d3 = json.loads(line)
                out["secondary"]["three_bf16_pieces_24bit"] = {
                    "images_per_sec": d3["value"], "ms_per_step": d3["ms_per_step"],
                    "note": "OTGAN_WINO_PIECES=3: conv GEMM operands as three bf16 pieces (hi+mid+lo = 24 significand bits), six "
                            "MFMAs per product; everything else identical; own process, unprofiled"}
            except Exception as e:      # never lose the headline line over the reference point
                out["secondary"]["three_bf16_pieces_24bit"] = {"error": repr(e)[:200]}
    if a.full and world == 1 and not a.no_cpu_baseline:
        from oracle import train_step_cpu
        # bounded sample: 2 shards x 16 images (~10 s of CPU work), at most 32 host threads (torch's CPU convs
        # degrade badly when oversubscribed: 256 threads took >4 min for this sample)
        torch.set_num_threads(min(32, os.cpu_count() or 1))
        bps = 16
        ips, best, nb = train_step_cpu.time_cpu_steps(batch_per_shard=bps, shards=2, iters=a.nr_sinkhorn_iter,
                                                      model=a.model)
        out["cpu_baseline"] = {"value": round(ips, 3), "unit": "images/sec", "cores": torch.get_num_threads(),
                               "kind": "port",
                               "sample": f"one generator step ({best['gen']:.2f} s) + one critic step "
                                         f"({best['disc']:.2f} s) of the oracle (PyTorch-CPU fp32 nets + C "
                                         f"Sinkhorn) at {nb} img/step (2 shards x {bps}), combined 5:1"}
    # the JSON line is the LAST thing on stdout: flush the C-level buffers first (RCCL prints a banner through
    # printf that would otherwise surface after Python's own output)
    sys.stdout.flush()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
