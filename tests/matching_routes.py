"""The calls that pin the training-mode matching entry points to every kernel route of csrc/sinkhorn.hip, and the route
predicates restated in Python (tests/test_matching_routes_cpu.py keeps the table on the routes it claims,
tests/test_matching_routes_gpu.py runs it).  No GPU and no library is needed to import this module.

The entry points (include/otgan.h) choose their kernels from the shape, the pitches, the alignment of the pointers and the
row range of the call; every Python caller passes packed torch allocations and full-tile row ranges, so the other routes are
only reachable through the C ABI -- and from the command line (`--batch_size 100` on 4 GPUs is N = 200 with 100-row ranges).

A case is one set of inputs: `mode` two / single (reference utils/matching.py:11-85 / :88-136), `entry` grad (the
training-mode entries) or infer (otgan_matching_two_batch_rows_f32), N rows per Sinkhorn problem, width D, `ldf_pad` / `ldo_pad`
floats added to D for the pitches, `in_off` / `out_off` floats by which fa, fb / the outputs are offset from a 16-byte
aligned base, the row ranges (None = the full call; two-batch ranges in rows of [0, 2N)) and for which of K_pre absent /
given every range runs.  lambda = 500, 8 cluster centres per side, 10 sweeps (3 at N > 1024), seed from the name.
"""

LAMBDA = 500.0
CENTRES = 8


def _case(name, mode, N, D, ranges, ldf_pad=0, ldo_pad=0, in_off=0, out_off=0, k_pre=(False,), iters=10, entry="grad"):
    return dict(name=name, mode=mode, entry=entry, N=N, D=D, iters=iters, ldf_pad=ldf_pad, ldo_pad=ldo_pad, in_off=in_off,
                out_off=out_off, ranges=list(ranges), k_pre=tuple(k_pre))


BOTH = (False, True)

CASES = [
    # ---- two-batch, one-tile kernels (N <= 128)
    _case("tile_h2_pitch", "two", 48, 100, [None, (0, 12), (48 + 36, 12)], ldf_pad=12, ldo_pad=8, k_pre=BOTH),
    _case("tile_scalar_pitch", "two", 32, 64, [None, (8, 5), (32 + 27, 5)], ldf_pad=3, ldo_pad=1, k_pre=BOTH),
    _case("tile_unaligned_in", "two", 32, 64, [None, (32, 16)], in_off=1),
    # D % 4 != 0 inside a 16-byte pitch: vector loaders with a ragged last float4, no fp16 kernels (they need D % 4 == 0)
    _case("tile_d70_vec", "two", 40, 70, [None, (0, 10), (40 + 30, 10)], ldf_pad=2, k_pre=BOTH),
    # two 128-column tiles of D in the fp16 plan application, the second one four columns wide
    _case("tile_h2_d132", "two", 32, 132, [None, (32 + 8, 8)]),
    _case("tile_n24_k24", "two", 24, 100, [None, (24 + 8, 8)]),                  # kdim % 16 != 0: no fp16 plan application
    # N % 4 != 0: the plans' pitch keeps the plan application on the scalar loaders whatever the cost kernel reads
    _case("tile_n33_ldp", "two", 33, 64, [None, (33 + 30, 3)]),
    _case("tile_n34_d70", "two", 34, 70, [None, (17, 17)], ldf_pad=2),
    # ---- two-batch, 128 < N < 256: panel Sinkhorn with two workgroups per problem, fp32 cost
    _case("panel2_k136", "two", 136, 72, [None, (0, 50), (136 + 86, 50), (40, 7)], k_pre=BOTH),
    _case("panel2_k144", "two", 144, 100, [None, (16, 128), (144 + 100, 44), (9, 3)], ldo_pad=4, k_pre=BOTH),
    _case("panel2_n200", "two", 200, 64, [None, (100, 100), (200, 100)]),
    _case("panel2_n130", "two", 130, 64, [None, (0, 65), (130 + 65, 65)]),       # second panel workgroup: two rows
    _case("panel2_scalar", "two", 136, 72, [None, (136 + 129, 7)], ldf_pad=1, k_pre=BOTH),
    # ---- two-batch, the split-precision engine (N >= 256, N % 32 == 0, D % 32 == 0, D >= 64) and the ways out of it
    _case("x3_smallest", "two", 256, 64, [None, (0, 16), (16, 40), (240, 16), (256 + 48, 200), (256 + 32, 100), (224, 32)],
          k_pre=BOTH),
    _case("x3_pitch", "two", 256, 64, [None, (64, 64)], ldf_pad=8, ldo_pad=4),
    _case("x3_m288", "two", 288, 96, [None, (272, 16), (288 + 128, 160), (256, 32), (288 + 224, 64)]),
    _case("x3_fallback_rowbegin", "two", 256, 64, [None, (8, 64), (256 + 40, 40), (250, 6), (8, 130)], k_pre=BOTH),
    _case("x3_fallback_ldo", "two", 256, 64, [None, (64, 64)], ldo_pad=2),
    _case("x3_fallback_out_align", "two", 256, 64, [None, (64, 64)], ldo_pad=4, out_off=1),
    _case("x3_fallback_ldf", "two", 256, 64, [None, (64, 64)], ldf_pad=1),
    _case("x3_fallback_in_align", "two", 256, 64, [None, (64, 64)], in_off=2),
    _case("n264_fp32", "two", 264, 64, [None, (0, 66), (264 + 198, 66)]),
    _case("n272_h2_long", "two", 272, 64, [None, (0, 128), (272 + 204, 68)], k_pre=BOTH),
    _case("d80_fp32", "two", 256, 80, [None, (0, 64)]),
    _case("d32_fp32", "two", 256, 32, [None, (128, 128)]),
    # ---- two-batch, N > 1024: the multi-launch Sinkhorn kernels
    _case("general_x3", "two", 1056, 64, [None, (1056 + 1040, 16), (0, 256)], iters=3, k_pre=BOTH),
    _case("general_fp32", "two", 1040, 64, [None, (0, 65), (1040 + 1000, 32), (200, 130)], iters=3, k_pre=BOTH),
    _case("general_scalar", "two", 1028, 32, [None, (1028 + 1000, 28)], iters=3, in_off=3, k_pre=BOTH),
    _case("general_n1026", "two", 1026, 32, [None, (0, 30)], iters=3),           # vector cost loaders, odd plan pitch
    # ---- single-batch
    _case("single_tile_pitch", "single", 48, 100, [None, (36, 12)], ldf_pad=12, ldo_pad=8),
    _case("single_panel2", "single", 136, 72, [None, (86, 50)]),
    _case("single_k144", "single", 144, 100, [None, (16, 128), (9, 3)], ldo_pad=4),
    _case("single_x3", "single", 256, 64, [None, (0, 16), (16, 40), (240, 16), (32, 100), (224, 32)], k_pre=BOTH),
    _case("single_x3_fallback", "single", 256, 64, [None, (8, 64), (250, 6)], k_pre=BOTH),
    _case("single_x3_fallback_ldo", "single", 256, 64, [None, (64, 64)], ldo_pad=2),
    _case("single_n264", "single", 264, 64, [None, (198, 66)]),
    # ---- the inference row variant (four matched arrays; its engine predicate has no output-alignment term)
    _case("infer_x3_smallest", "two", 256, 64, [(0, 16), (16, 40), (240, 16), (256 + 48, 200), (256 + 32, 100)], k_pre=BOTH,
          entry="infer"),
    _case("infer_x3_fallback_rowbegin", "two", 256, 64, [(8, 64), (256 + 40, 40), (250, 6)], k_pre=BOTH, entry="infer"),
    _case("infer_panel2_k144", "two", 144, 100, [(16, 128), (144 + 100, 44), (9, 3)], ldo_pad=4, k_pre=BOTH, entry="infer"),
]

# The shapes bench.py and the multi-rank runs ship on: (case, range, route).  No change to the kernels' predicates may move
# them (tests/test_matching_routes_cpu.py::test_shipped_routes_are_pinned).
SHIPPED = [
    (_case("ship_n128", "two", 128, 32768, [None]), None, ("h2", "small", "h2")),
    (_case("ship_n256", "two", 256, 7296, [None]), None, ("x3", "panel", "x3")),
    (_case("ship_n256_rows", "two", 256, 7296, [(256, 256)]), (256, 256), ("x3", "panel", "x3")),
    (_case("ship_n1024_rows", "two", 1024, 7296, [(256, 256)]), (256, 256), ("x3", "panel", "x3")),
    (_case("ship_n1024_rows_pre", "two", 1024, 7296, [(1024 + 768, 256)], k_pre=(True,)), (1024 + 768, 256), ("given", "panel", "x3")),
]


def seed_of(name):
    """the seed of a case's features: a function of its name alone"""
    s = 0
    for i, ch in enumerate(name):
        s = (s * 131 + ord(ch) + i) % 2147483629
    return s


def problem_rows(case):
    """rows of the feature arrays fa / fb: 2N (two mini-batches) or n"""
    return 2 * case["N"] if case["mode"] == "two" else case["N"]


# ------------------------------------------------------------------------------------------------------------------
# the predicates of csrc/sinkhorn.hip (file:line of what each one restates)
# ------------------------------------------------------------------------------------------------------------------
def x3_shape_ok(n, m, D):
    """sinkhorn.hip:1590-1592 (x3_shape_ok; OTGAN_MATCH_FP32 unset)"""
    return n >= 256 and m >= 256 and n % 32 == 0 and m % 32 == 0 and D % 32 == 0 and D >= 64


def aligned16_floats(off):
    """sinkhorn.hip:1720 (aligned16) for a pointer `off` floats behind a 16-byte aligned base"""
    return (4 * off) % 16 == 0


def engine_ok(case):
    """sinkhorn.hip:2079 (FeatSrc::engine_ok, arrays): ld % 4 == 0 && aligned16(fa) && aligned16(fb)"""
    return (case["D"] + case["ldf_pad"]) % 4 == 0 and aligned16_floats(case["in_off"])


def uses_engine(case, rng):
    """the x3 flag of the entry point: sinkhorn.hip:2337 (matching_grad_impl), :2557 (single_grad_impl), :2305
    (otgan_matching_two_batch_rows_f32: no output-alignment term); row_begin % 32: x3_row_begin_ok, :1594-1598"""
    N, D = case["N"], case["D"]
    ldo = D + case["ldo_pad"]
    row_begin = 0 if rng is None else rng[0]
    x3 = x3_shape_ok(N, N, D) and engine_ok(case) and ldo % 4 == 0 and row_begin % 32 == 0
    if case["entry"] == "grad":
        x3 = x3 and aligned16_floats(case["out_off"])        # grad_a and grad_b (NULL is aligned)
    return x3


def feature_blocks_vec(case):
    """sinkhorn.hip:1764-1769 (launch_cost) and :1863-1872 (launch_apply), the feature side: ldf % 4 == 0 and every block
    pointer 16-byte aligned.  A block starts b * N * ldf floats behind fa / fb (:2080), a multiple of 4 when ldf is one."""
    ldf = case["D"] + case["ldf_pad"]
    return ldf % 4 == 0 and aligned16_floats(case["in_off"]) and aligned16_floats(case["in_off"] + case["N"] * ldf)


def cost_h2_ok(case, vec):
    """sinkhorn.hip:1726-1728 (cost_h2_ok; cosine cost)"""
    N, D = case["N"], case["D"]
    return vec and N <= 128 and D % 4 == 0 and (D + case["ldf_pad"]) % 4 == 0


def cost_splits(case):
    """sinkhorn.hip:1729-1746 (plan_cost): K splits of the fp32 / fp16 one-tile cost kernels; 1 = the fused epilogue"""
    N, D = case["N"], case["D"]
    P = 6 if case["mode"] == "two" else 3
    tiles = ((N + 127) // 128) ** 2
    nkt = (D + 15) // 16
    target = 384 if cost_h2_ok(case, feature_blocks_vec(case)) else 768
    want = 1 if tiles * P >= 256 else -(-target // (tiles * P))
    want = max(1, min(want, nkt))
    per = -(-nkt // want)
    return -(-nkt // per)


def sinkhorn_route(n):
    """sinkhorn.hip:1817 (one workgroup), :1826-1839 (panel kernel: 128 / 64 / 32 rows per workgroup), :1846-1853 (one
    launch per half-sweep)"""
    if n <= 128:
        return "small"
    if n <= 1024:
        return "panel"
    return "multi"


def panel_workgroups(n):
    """sinkhorn.hip:1828,1831: (rows per workgroup, workgroups per problem) of the panel kernel"""
    rpw = 128 if n <= 256 else (64 if n <= 512 else 32)
    return rpw, -(-n // rpw)


def apply_route(case, rng):
    """sinkhorn.hip:1859-1923 (launch_apply) as the non-engine branches of matching_grad_impl (:2391-2414), single_grad_impl
    (:2583-2594) and apply_matched (:2216-2225) call it: every term is rows [r0, r0 + cnt) of an [N, N] plan in the
    workspace (256-byte aligned: Carver, :1748-1757), ldp = kdim = N, all blocks `cnt` rows."""
    N, D = case["N"], case["D"]
    if rng is None:
        r0, cnt = 0, N
    else:
        r0, cnt = (rng[0] % N if case["mode"] == "two" else rng[0]), rng[1]
    nprob = 6 if case["mode"] == "two" else 3
    plans_aligned = all(aligned16_floats(p * N * N + r0 * N) for p in range(nprob))            # :2223, :2405-2411, :2586-2591
    vec = feature_blocks_vec(case) and plans_aligned and N % 4 == 0                              # :1863-1872
    h2 = vec and cnt <= 128 and D % 4 == 0 and D >= 4                                            # :1875 (bounded plans)
    if h2 and N % 16 == 0 and N >= 16:                                                           # :1882
        return "h2"
    return "fp32_vec" if vec else "fp32_scalar"                                                  # :1918-1919


def expected_route(case, rng, k_pre=False):
    """(cost, sinkhorn, apply) of one call.  cost: given (K_pre) / x3 / h2 / fp32_vec / fp32_scalar (match_solve,
    sinkhorn.hip:2122-2142, and launch_cost :1786-1796); apply: x3 / h2 / fp32_vec / fp32_scalar."""
    x3 = uses_engine(case, rng)
    if k_pre:
        cost = "given"                                      # :2121-2122
    elif x3:
        cost = "x3"                                         # :2124-2130
    else:
        vec = feature_blocks_vec(case)
        cost = "h2" if cost_h2_ok(case, vec) else ("fp32_vec" if vec else "fp32_scalar")
    return cost, sinkhorn_route(case["N"]), ("x3" if x3 else apply_route(case, rng))


def failed_engine_terms(case, rng):
    """which terms of the engine predicate fail for a call (empty: the engine runs)"""
    N, D = case["N"], case["D"]
    failed = []
    if not x3_shape_ok(N, N, D):
        failed.append("shape")
    if (D + case["ldf_pad"]) % 4:
        failed.append("ldf % 4")
    if not aligned16_floats(case["in_off"]):
        failed.append("input alignment")
    if (D + case["ldo_pad"]) % 4:
        failed.append("ldo % 4")
    if case["entry"] == "grad" and not aligned16_floats(case["out_off"]):
        failed.append("output alignment")
    if rng is not None and rng[0] % 32:
        failed.append("row_begin % 32")
    return failed


def calls(case):
    """every (range, k_pre) the GPU test runs for a case: K_pre goes with the row-range entries only"""
    out = []
    for rng in case["ranges"]:
        out += [(None, False)] if rng is None else [(rng, kp) for kp in case["k_pre"]]
    return out


def packed_twin(case):
    """the same case without pitch padding when it runs the same kernels call for call, else None"""
    if not (case["ldf_pad"] or case["ldo_pad"]):
        return None
    twin = dict(case, ldf_pad=0, ldo_pad=0)
    same = all(expected_route(case, r, k) == expected_route(twin, r, k) for r, k in calls(case))
    return twin if same else None


# ------------------------------------------------------------------------------------------------------------------
# inputs and the fp64 reference, shared by the CPU and the GPU test (computed once per case)
# ------------------------------------------------------------------------------------------------------------------
_cache = {}


def features(case):
    """(fa, fb) float32 [rows, D]: clustered rows of unit length (oracle.matching_np.clustered_features), 8 centres per side"""
    import numpy as np
    from oracle import matching_np as M
    rows, D = problem_rows(case), case["D"]
    rng = np.random.RandomState(seed_of(case["name"].replace("infer_", "")))
    ca, cb = rng.randn(CENTRES, D), rng.randn(CENTRES, D)
    fa = M.clustered_features(rng, rows, D, ca).astype(np.float32)
    fb = M.clustered_features(rng, rows, D, cb).astype(np.float32)
    return fa, fb


def reference(case):
    """fp64 oracle on the fp32 inputs: dict(aa, bb, ab, ba [rows, D], entropy, dist).  Not to be modified by callers."""
    import numpy as np
    from oracle import matching_np as M
    key = (case["name"].replace("infer_", ""), case["mode"], case["N"], case["D"], case["iters"])
    if key in _cache:
        return _cache[key]
    fa, fb = (z.astype(np.float64) for z in features(case))
    N = case["N"]
    if case["mode"] == "two":
        fa1, fa2, fb1, fb2 = fa[:N], fa[N:], fb[:N], fb[N:]
        plans, costs, ent = M.two_batch_plans(fa1, fa2, fb1, fb2, LAMBDA, case["iters"])
        halves = [M.matched_rows(plans, fa1, fa2, fb1, fb2, h, 0, N) for h in (0, 1)]
        aa, bb, ab, ba = (np.concatenate([halves[0][i], halves[1][i]]) for i in range(4))
        dist = M.closed_form_from(plans, costs, N)
    else:
        ref = M.get_matched_features_single_batch([fa], [fb], LAMBDA, case["iters"])
        aa, bb, ab, ba = (ref[i][0] for i in range(4))
        ent = ref[4]
        dist = M.calc_distance([fa], [fb], ref)
    out = dict(aa=aa, bb=bb, ab=ab, ba=ba, entropy=float(ent), dist=float(dist))
    for v in out.values():
        if hasattr(v, "setflags"):
            v.setflags(write=False)
    _cache[key] = out
    return out
