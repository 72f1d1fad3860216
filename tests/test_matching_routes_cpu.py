"""CPU: the case table of tests/matching_routes.py stays on the kernel routes it claims.  The GPU test
(tests/test_matching_routes_gpu.py) runs the table; this file checks, from the predicates of csrc/sinkhorn.hip restated in
matching_routes.expected_route, that the table reaches every (cost, Sinkhorn, plan application) route an admissible call can
take, every way out of the split-precision engine on its own, the fp16 plan application at short and long contractions, and
that the fp64 reference it is compared with leaves the tolerance to the kernels."""
import itertools

import numpy as np
import pytest

import matching_routes as R
from conftest import REL_DIFF_INJECTED

ALL_CALLS = [(c, rng, kp) for c in R.CASES for rng, kp in R.calls(c)]


def test_case_names_are_unique_and_fields_complete():
    names = [c["name"] for c in R.CASES]
    assert len(set(names)) == len(names)
    for c in R.CASES:
        assert c["mode"] in ("two", "single") and c["entry"] in ("grad", "infer")
        assert c["iters"] == (3 if c["N"] > 1024 else 10)
        assert c["ldf_pad"] >= 0 and c["ldo_pad"] >= 0 and 0 <= c["in_off"] < 4 and 0 <= c["out_off"] < 4
        assert c["ranges"] and c["k_pre"] and set(c["k_pre"]) <= {False, True}
        assert c["entry"] == "grad" or None not in c["ranges"]      # the inference entry here is the row variant


def test_ranges_lie_inside_one_mini_batch():
    for c in R.CASES:
        N, total = c["N"], R.problem_rows(c)
        for rng in c["ranges"]:
            if rng is None:
                continue
            b, n = rng
            assert 0 <= b and n > 0 and b + n <= total, (c["name"], rng)
            if c["mode"] == "two":
                assert b // N == (b + n - 1) // N, (c["name"], rng)


def _admissible():
    """every route triple some admissible call takes: the predicates over a grid of shapes on both sides of each threshold
    (N 128 | 129, 255 | 256, 1024 | 1025, N % 4, % 16, % 32; D % 4, % 32, D < 64), pitches, offsets, ranges and K_pre"""
    got = set()
    Ns = (16, 24, 33, 34, 48, 128, 129, 130, 136, 144, 200, 255, 256, 264, 272, 288, 1024, 1025, 1028, 1040, 1056)
    Ds = (3, 32, 64, 70, 72, 80, 96, 100, 132)
    for (mode, entry), N, D, lf, lo, io, oo in itertools.product((("two", "grad"), ("single", "grad"), ("two", "infer")), Ns, Ds,
                                                                 (0, 1, 2, 4), (0, 1, 2, 4), (0, 1, 2), (0, 1)):
        c = R._case("grid", mode, N, D, [], ldf_pad=lf, ldo_pad=lo, in_off=io, out_off=oo, entry=entry)
        for rng in (None, (0, min(N, 16)), (8, min(N - 8, 5)), (1, 3), (16, min(N - 16, 128)), (0, N)):
            if rng is None and entry == "infer":
                continue
            for kp in ((False,) if rng is None else (False, True)):
                got.add(R.expected_route(c, rng, kp))
    return got


# Triples that no call can take, with the reason (asserted absent from the enumeration below).
IMPOSSIBLE = {
    ("x3", "*", "h2"): "one flag (x3) routes the cost stage and the plan application of a call: sinkhorn.hip:2337,2350,2370",
    ("x3", "*", "fp32_vec"): "the same flag",
    ("x3", "*", "fp32_scalar"): "the same flag",
    ("h2", "*", "x3"): "the same flag",
    ("fp32_vec", "*", "x3"): "the same flag",
    ("fp32_scalar", "*", "x3"): "the same flag",
    ("x3", "small", "*"): "the engine takes N >= 256 (x3_shape_ok), the one-workgroup Sinkhorn kernel N <= 128",
    ("*", "small", "x3"): "the same",
    ("h2", "panel", "*"): "cost128_h2_kernel takes N <= 128 (cost_h2_ok), the panel kernel N > 128",
    ("h2", "multi", "*"): "cost128_h2_kernel takes N <= 128, the multi-launch kernels N > 1024",
    ("fp32_scalar", "*", "h2"): "scalar cost loaders mean ldf % 4 != 0 or unaligned features, which launch_apply's vec refuses too",
    ("fp32_scalar", "*", "fp32_vec"): "the same",
    ("fp32_vec", "small", "h2"): "aligned features at N <= 128 with D % 4 == 0 go to cost128_h2_kernel; D % 4 != 0 keeps both "
                                 "stages off the fp16 kernels",
}


def _matches(pattern, triple):
    return all(p == "*" or p == t for p, t in zip(pattern, triple))


def test_every_admissible_route_is_in_the_table():
    admissible = _admissible()
    covered = {R.expected_route(c, rng, kp) for c, rng, kp in ALL_CALLS}
    assert covered <= admissible, sorted(covered - admissible)
    missing = sorted(admissible - covered)
    assert not missing, missing
    for pattern, why in IMPOSSIBLE.items():
        hit = [t for t in admissible | covered if _matches(pattern, t)]
        assert not hit, (pattern, why, hit)
    # and nothing else is left out: every triple of the three route sets is covered or listed as impossible
    costs, sinks, applies = ("given", "x3", "h2", "fp32_vec", "fp32_scalar"), ("small", "panel", "multi"), ("x3", "h2", "fp32_vec", "fp32_scalar")
    for t in itertools.product(costs, sinks, applies):
        assert t in covered or any(_matches(p, t) for p in IMPOSSIBLE), t


def test_every_way_out_of_the_engine_appears_alone():
    alone = {}
    for c, rng, kp in ALL_CALLS:
        failed = R.failed_engine_terms(c, rng)
        if len(failed) == 1:
            alone.setdefault(failed[0], []).append((c["name"], rng))
            assert R.expected_route(c, rng, False)[2] != "x3"
        if not failed:
            assert R.expected_route(c, rng, False)[2] == "x3"
    for trigger in ("row_begin % 32", "ldo % 4", "output alignment", "ldf % 4", "input alignment"):
        assert trigger in alone, (trigger, sorted(alone))
    # both ABIs leave the engine on a row range and on an output pitch
    for mode in ("two", "single"):
        names = {n for t in ("row_begin % 32", "ldo % 4") for n, _ in alone[t]}
        assert any(next(c for c in R.CASES if c["name"] == n)["mode"] == mode for n in names), mode


def test_fp16_plan_application_at_short_and_long_contractions():
    kdims = {c["N"] for c, rng, kp in ALL_CALLS if R.expected_route(c, rng, kp)[2] == "h2"}
    assert any(k <= 128 for k in kdims) and any(128 < k < 256 for k in kdims) and any(k >= 256 for k in kdims), sorted(kdims)
    # ... with a ragged row count, a row count of a full tile, and three- and two-term blocks
    h2 = [(c, rng) for c, rng, kp in ALL_CALLS if R.expected_route(c, rng, kp)[2] == "h2" and rng is not None]
    assert any(rng[1] == 128 for _, rng in h2) and any(rng[1] % 16 for _, rng in h2)
    assert {c["mode"] for c, _ in h2} == {"two", "single"}


def test_sinkhorn_panel_and_cost_split_edges():
    panel = {R.panel_workgroups(c["N"]) + (c["N"] % R.panel_workgroups(c["N"])[0],) for c in R.CASES if R.sinkhorn_route(c["N"]) == "panel"}
    assert any(r == 2 and rag for _, r, rag in panel) and any(r > 2 and rag for _, r, rag in panel) and any(not rag for _, _, rag in panel)
    fp32 = [c for c in R.CASES if R.expected_route(c, None if None in c["ranges"] else c["ranges"][0], False)[0].startswith("fp32")]
    assert any(R.cost_splits(c) == 1 for c in fp32) and any(R.cost_splits(c) > 1 for c in fp32)    # fused epilogue / partial sums


def test_engine_row_ranges_are_ragged():
    """launch_apply_x3: fewer rows than a 256-row tile, a count that is no multiple of 16, a range ending on the last row"""
    x3 = [(c, rng) for c, rng, kp in ALL_CALLS if rng is not None and R.expected_route(c, rng, kp)[2] == "x3"]
    assert any(rng[1] < 256 for _, rng in x3) and any(rng[1] % 16 for _, rng in x3)
    assert any((rng[0] + rng[1]) % c["N"] == 0 for c, rng in x3)
    assert any(c["N"] % 256 for c, _ in x3)


def test_shipped_routes_are_pinned():
    """the benchmarked calls: N = 128 full calls, N = 256 / 1024 with 256-row ranges, ld == D, packed and aligned"""
    for c, rng, want in R.SHIPPED:
        assert R.expected_route(c, rng, c["k_pre"][0]) == want, c["name"]


def test_twins_exist_for_the_pitched_cases():
    twins = {c["name"] for c in R.CASES if R.packed_twin(c)}
    assert {"tile_h2_pitch", "x3_pitch", "single_tile_pitch", "panel2_k144", "single_k144"} <= twins, twins
    assert "tile_scalar_pitch" not in twins and "x3_fallback_ldo" not in twins


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_reference_alone_is_well_inside_the_tolerance(case):
    """the oracle's differences of a range, rounded to fp32, are within REL_DIFF_INJECTED / 10 of their fp64 values, and no
    range is a near-zero denominator: its rows carry at least 1e-3 of their share of the half's norm"""
    ref = R.reference(case)
    N = case["N"]
    for name, diff in (("a", ref["aa"] - ref["ab"]), ("b", ref["bb"] - ref["ba"])):
        for rng in case["ranges"]:
            b, n = (0, R.problem_rows(case)) if rng is None else rng
            rows = diff[b:b + n]
            nrm = np.linalg.norm(rows)
            err = np.linalg.norm(rows.astype(np.float32).astype(np.float64) - rows) / nrm
            assert err < REL_DIFF_INJECTED / 10, (case["name"], name, rng, err)
            half = diff[(b // N) * N:(b // N + 1) * N] if rng is not None else diff[:N]
            share = np.sqrt(min(n, N) / N) * np.linalg.norm(half)
            assert nrm >= 1e-3 * share, (case["name"], name, rng, nrm, share)
    assert np.isfinite(ref["dist"]) and np.isfinite(ref["entropy"])
