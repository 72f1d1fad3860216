"""CPU: the case table of tests/conv_routes.py stays on the kernel routes it claims.  tests/test_conv_routes_gpu.py runs the
table; this file checks, without a device,
  - that the table is well-formed and that every route written beside a case is what the restated predicates give;
  - that the restated predicates (conv_routes.make_geo ... plan_wgrad) agree with the library's host queries over a grid of
    descriptors on both sides of every threshold;
  - that the table reaches every route an admissible call can take, per pass, and that the routes listed as impossible do not
    occur;
  - that the convolutions of the benchmarked models keep their routes;
  - that the fp64 oracle (oracle/nets_torch.py) is right for the filters the table adds (1x1, even, non-square) and leaves
    the 2e-5 bound to the kernels."""
import ctypes
import inspect
import itertools
import random
import re

import numpy as np
import pytest
import torch

import conv_routes as R

TOL = 2e-5                      # tests/test_layers_gpu.py
PASS = ("forward", "input gradient", "weight gradient")


# ------------------------------------------------------------------------------------------------------------------
# the library's host queries (no device needed: tests/test_abi_cpu.py)
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def Q():
    from otgan_amd import _lib, _lib_layers
    L = _lib.lib()

    class Queries:
        @staticmethod
        def desc(fields, **extra):
            d = _lib_layers.ConvDesc()
            for k, v in dict(fields, **extra).items():
                setattr(d, k, v)
            return d

        def workspace(self, fields, which):
            return int(L.otgan_conv2d_workspace_bytes(ctypes.byref(self.desc(fields)), which))

        def filter_bytes(self, fields, which):
            return int(L.otgan_conv2d_filter_bytes(ctypes.byref(self.desc(fields)), which))

        def operand_bytes(self, fields):
            return int(L.otgan_conv2d_operand_bytes(ctypes.byref(self.desc(fields))))

        def folded(self, fields):
            return int(L.otgan_conv2d_folded_weight_elems(ctypes.byref(self.desc(fields))))

        def amax_fused(self, fields, which):
            return int(L.otgan_conv2d_amax_fused(ctypes.byref(self.desc(fields)), which))

        def glu_fused(self, fields):
            return int(L.otgan_conv2d_glu_fused(ctypes.byref(self.desc(fields))))

        def h2_ok(self, fields, **extra):
            return int(L.otgan_dense16_h2_ok(ctypes.byref(self.desc(fields, **extra))))

        def dense16(self, d, g):
            return R.dense16_of(self.workspace, d, g, lambda f: bool(L.otgan_dense16_h2_ok(ctypes.byref(self.desc(f)))))

    return Queries()


def _route(Q, case, which):
    d = R.desc_fields(case)
    g = R.make_geo(d)
    d16 = Q.dense16(d, g) if isinstance(g, dict) else (False, 0)
    assert d16[0] is not None, ("dense16_tiling undecidable from the workspace query", case["name"])
    return R.expected_route(case, which, d16, Q.operand_bytes(d) > 0)


# ------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------
def test_table_is_well_formed():
    names = [c["name"] for c in R.CASES]
    assert len(set(names)) == len(names)
    for c in R.CASES:
        d = R.desc_fields(c)
        g = R.make_geo(d)
        assert isinstance(g, dict), (c["name"], g)                       # every descriptor passes make_geo
        assert set(c["off"]) == set(R.OPERANDS) and all(0 <= v <= 3 for v in c["off"].values()), c["name"]
        assert c["ws"] in ("full", "short", "null") and c["filters"] in (None, "own", "unfolded", "dummy") and c["cmap"] in ("auto", "identity")
        assert c["passes"] and set(c["passes"]) <= {0, 1, 2} and set(c["expect"]) == set(c["passes"]), c["name"]
        assert c["xpad"] >= 0 and c["ypad"] >= 0 and c["dxpad"] >= 0 and c["y_coff"] >= 0
        assert d["ldx"] >= d["C"] and d["ldy"] >= d["y_coff"] + d["Cout"] and R.lddx(c) >= d["C"]
        # pitches and offsets against the buffers the GPU test lays out: the last valid float of the last row lies inside
        for name, (rows, width, pitch, first) in ((k, v) for k, v in R.shapes(c).items() if isinstance(v, tuple)):
            assert first + width <= pitch and rows > 0, (c["name"], name)
            last = R.GUARD + c["off"][name] + (rows - 1) * pitch + first + width
            assert last <= R.buffer_floats(c, name) - R.GUARD, (c["name"], name)
        if c["cmap"] == "identity":
            assert len(c["segs"]) == 1, c["name"]                        # an explicit map equal to the default ordering
        # shapes stay small unless a tile-count threshold needs them
        big = d["N"] * d["H"] * d["W"] > 4 * 16 * 16 or d["C"] > 128 or d["Cout"] > 256
        if big and re.match(r"p[012]_", c["name"]):
            # the cases that complete the (family, configuration) pairs: large only behind a tile-count threshold of
            # launch_igemm / igemm_fwd_ksplit / plan_wgrad (Main16, the exact-width tiles, K splits, pixel splits)
            assert re.search(r"Main16_x|W160|W224|_split|ksplit", str(c["expect"])), c["name"]
        else:
            assert not big or c["name"] in BIG_ON_PURPOSE, c["name"]
    for a, b in R.TWINS:
        A, B = R.BY_NAME[a], R.BY_NAME[b]
        assert R.base_name(dict(A, cmap="auto")) == R.base_name(dict(B, cmap="auto")), (a, b)


# cases above N = 4, 16 x 16, 128 channels: the smallest shape that crosses the threshold named
BIG_ON_PURPOSE = {
    "s2_crelu_xop": "a shared x operand needs a multiple of 32 Winograd tiles (otgan_conv2d_operand_bytes > 0): N = 32 at 8 x 8",
    "s2_xop_x_off": "as s2_crelu_xop", "s2_xop_cmap": "as s2_crelu_xop",
    "up3": "wino_up3_wgrad_ok: N * (2H / 4) * (2W / 4) % 32 == 0 -> N = 8 at 4 x 4",
    "rgbin_tpb2": "launch_rgbin_fwd: (tiles / 2) * (Cout / 64) >= 1024 at Cout = 128 -> 1024 tiles of 256 pixels",
    "tiles128_512": "launch_igemm: ceil(rows / 128) * ntiles * ncls >= 512 with one column tile -> 65536 rows",
    "tiles128_511": "the other side: 32768 rows",
    "w160_256": "launch_igemm: ceil(rows / 128) * ncls >= 256 -> 32768 rows",
    "w160_128": "the other side: 16384 rows",
    "ksplit_w224": "igemm_fwd_ksplit = 8 needs 64 channel slices (Ceff = 1024); ceil(rows / 128) * 8 >= 256 -> 4096 rows",
    "ksplit_main16": "the same with one column tile: ceil(rows / 128) * 8 >= 512 -> 8192 rows",
    "w224_256": "as w160_256", "tiles128_512_ws_null": "as tiles128_512", "w160_256_ws_null": "as w160_256",
    "w224_256_ws_null": "as w160_256", "dg_tiles128_512": "as tiles128_512, input gradient", "dg_tiles128_512_ws_null": "as tiles128_512", "w224_ck48": "as w160_256, Ck % 32 != 0", "w160_ck16": "as w160_256, Ck % 32 != 0: no exact-width tile",
    "wg_main16_split": "plan_wgrad: nkt / nsplit >= 16 with 1 x 1 taps in one K (scalar path) -> 2048 pixels",
    "rgbin_w64_k3": "W = 64", "rgbin_w128": "W = 128", "rgbout_w128": "W = 128",
    "fold_3x2_split": "plan_wgrad: nkt / nsplit >= 16 on the small grid -> 512 pixels", "wg_fold_main_split": "1024 pixels (BK = 32)",
    "up3_nofilters": "as up3", "up3_x_off": "as up3", "up3_y_off": "as up3", "up3_ws_short": "as up3", "up3_lddx": "as up3",
    "up3_dw_off": "as up3", "wg_n16_scalar_split": "1024 pixels", "wg_narrow_scalar_split": "1024 pixels",
}


def _fmt(route):
    return "ERR%d:%s" % route if R.is_error(route) else route


def test_expected_outcomes_are_what_the_restated_predicates_give(Q):
    """double entry: the route written beside each case (read off csrc/conv.hip by hand) against expected_route"""
    bad = []
    for c in R.CASES:
        for which in c["passes"]:
            got = _route(Q, c, which)
            if got != c["expect"][which]:
                bad.append((c["name"], PASS[which], _fmt(c["expect"][which]), _fmt(got)))
    assert not bad, "\n".join("%s %s: table %s, predicates %s" % b for b in bad)


def test_refused_calls_differ_from_a_call_that_succeeds_by_one_property(Q):
    for c in R.CASES:
        refused = [w for w in c["passes"] if R.is_error(c["expect"][w])]
        if not refused:
            continue
        base = c["base"]
        assert base is not None, c["name"]
        changed = [k for k in c if k not in ("name", "expect", "base", "passes") and c[k] != base[k]]
        assert len(changed) == 1, (c["name"], changed)
        if changed == ["off"]:
            assert sum(1 for k in c["off"] if c["off"][k] != base["off"][k]) == 1, c["name"]
        for w in refused:
            assert not R.is_error(_route(Q, base, w)), (c["name"], PASS[w])


def test_twins_leave_the_winograd_route():
    for a, b in R.TWINS:
        A, B = R.BY_NAME[a], R.BY_NAME[b]
        left = [w for w in B["passes"] if R.is_wino(A["expect"][w]) and not R.is_wino(B["expect"][w])]
        assert left, (a, b)


# ------------------------------------------------------------------------------------------------------------------
# the grid
# ------------------------------------------------------------------------------------------------------------------
def _grid():
    """descriptors on both sides of every threshold of the predicates: every table case, and a seeded sample of the product of
    the values below"""
    out = [R.desc_fields(c) for c in R.CASES]
    rnd = random.Random(20240607)
    Ns, HW = (1, 2, 3, 4, 8, 16, 32, 64), ((4, 4), (8, 8), (16, 16), (32, 32), (4, 64), (8, 4), (64, 64), (8, 128), (2, 2), (16, 8), (8, 16), (4, 32), (2, 64))
    Cs = (1, 2, 3, 4, 6, 8, 12, 16, 20, 32, 40, 48, 64, 128)
    Couts = (1, 2, 3, 4, 8, 12, 16, 20, 24, 32, 36, 40, 64, 128, 132, 144, 160, 164, 192, 196, 224, 228, 256)
    Ks = ((1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (1, 5), (5, 1), (2, 3), (3, 2), (3, 5))
    for _ in range(30000):
        H, W = rnd.choice(HW)
        C, Cout = rnd.choice(Cs), rnd.choice(Couts)
        y_coff = rnd.choice((0, 0, 1, 4, 16))
        out.append(dict(N=rnd.choice(Ns), H=H, W=W, C=C, ldx=C + rnd.choice((0, 0, 1, 2, 4)), upsample=rnd.choice((0, 0, 1)),
                        KH=0, KW=0, stride=rnd.choice((1, 1, 2)), Cout=Cout, ldy=y_coff + Cout + rnd.choice((0, 0, 2, 4, 16)),
                        y_coff=y_coff, preact=rnd.choice((0, 1, 1, 2, 3, 4)), list_quads=rnd.choice((1, 1, 0)),
                        y_accumulate=rnd.choice((0, 0, 0, 1))))
        out[-1]["KH"], out[-1]["KW"] = rnd.choice(Ks)
    return out


GRID = _grid()


def test_restated_geometry_and_eligibility_agree_with_the_library(Q):
    n_fold = n_wino = n_ks = 0
    for d in GRID:
        g = R.make_geo(d)
        assert isinstance(g, dict), d
        # exact: pure functions of the descriptor
        assert Q.folded(d) == R.folded_weight_elems(d, g), d
        for which in (-1, 0, 1, 2, 3, 4):
            assert (Q.filter_bytes(d, which) > 0) == R.filter_bytes_positive(d, g, which), (d, which)
        # (whether a Winograd layer's forward and weight gradient share an operand is winograd.hip's decision -- tile count,
        # GEMM engine: only the necessary condition can be restated)
        assert Q.operand_bytes(d) == 0 or R.operand_bytes_possible(d, g), d
        assert Q.glu_fused(d) == int(R.glu_fused(d, g)), d
        for which in (0, 1):
            assert Q.amax_fused(d, which) == R.amax_fused(d, g, which), (d, which)
        assert Q.amax_fused(d, 2) == 0
        wino = R.wino_ok(d, g) or R.wino_s2_ok(d, g) or R.wino_up3_ok(d, g)
        n_fold += g["fold"]
        n_wino += wino
        # workspace: exact where no Winograd pass exists (the Winograd formulas are the library's: there the query is the
        # larger of the two, or the Winograd size alone for the folded 5x5 layers -- only "at least" can be said)
        ws = [Q.workspace(d, w) for w in (0, 1, 2)]
        gen = [R.generic_fwd_workspace(d, g), R.generic_dgrad_workspace(d, g)]
        if not wino:
            assert ws[0] == gen[0] and ws[1] == gen[1], (d, ws, gen)
            vec = R.map_quads(d) and g["Ceff"] % 16 == 0 and d["ldx"] % 4 == 0
            ks = R.igemm_fwd_ksplit(d, g, vec, d["N"] * g["OH"] * g["OW"])
            n_ks += ks > 1
            # the query grows by the K-split partial sums exactly when the restated igemm_fwd_ksplit exceeds 1
            assert (ws[0] > R.RECS_BYTES) == (ks > 1), (d, ws[0], ks)
            if ks > 1:
                assert ws[0] - R.align_up(R.RECS_BYTES, 256) == 4 * ks * d["N"] * g["OH"] * g["OW"] * d["Cout"], d
        elif not R.wino_ok(d, g):
            assert ws[0] >= gen[0] and ws[1] >= gen[1], (d, ws, gen)
        else:
            assert min(ws) > 256, (d, ws)
        # weight gradient: plan_wgrad's slabs, with dense16_tiling taken from the library
        if not wino:
            d16 = Q.dense16(d, g) if R.dense16_wgrad_desc(d) else (False, 0)
            if d16[0] is not None:
                assert ws[2] == R.wgrad_workspace_generic(d, g, R.plan_wgrad(d, g, d16)), (d, ws[2], d16)
    assert n_fold > 500 and n_wino > 100 and n_ks > 20, (n_fold, n_wino, n_ks)     # the grid reaches what it is for


def test_growth_kernel_queries(Q):
    """otgan_dense16_h2_ok cannot be predicted from the route alone (its tile search is dense16.hip's); what must hold: it
    accepts only growth layers (16 outputs, 3x3, CReLU over 16-wide list elements, accumulating), and wherever it accepts,
    dense16_tiling -- the same tile search behind the fp32 growth kernels -- accepts the geometry too"""
    seen = 0
    for N, (H, W), nsl in itertools.product((1, 2, 4, 32), ((8, 8), (16, 16), (32, 32), (4, 4), (4, 64), (16, 8), (64, 64)), (1, 3)):
        C = 16 * nsl
        d = dict(N=N, H=H, W=W, C=C, ldx=C + 16, upsample=0, KH=3, KW=3, stride=1, Cout=16, ldy=C + 16, y_coff=C, preact=R.ACT_CRELU,
                 list_quads=1, y_accumulate=1)
        g = R.make_geo(d)
        ok = Q.h2_ok(d, list_width=16)
        assert Q.h2_ok(d, list_width=0) == 0 and Q.h2_ok(dict(d, y_accumulate=0), list_width=16) == 0
        assert Q.h2_ok(dict(d, preact=R.ACT_CELU), list_width=16) == 0 and Q.h2_ok(dict(d, KH=5, KW=5), list_width=16) == 0
        if ok:
            seen += 1
            assert Q.dense16(d, g)[0] is not False, d
    assert seen >= 8


def _call_variants(d):
    """the ways a descriptor can be called: alignment of each operand, the channel map, the workspace, `filters`, lddx"""
    segs = (d["C"],)
    base = dict(R._c("grid", d["N"], d["H"], d["W"], segs, d["Cout"], (d["KH"], d["KW"]), stride=d["stride"], up=d["upsample"],
                     pre=d["preact"], xpad=d["ldx"] - d["C"], ypad=d["ldy"] - d["y_coff"] - d["Cout"], y_coff=d["y_coff"]))
    if not d["list_quads"] and R.doubled(d["preact"]) and d["C"] >= 2:
        base["segs"] = (1, d["C"] - 1)                                    # a list with an element that is no multiple of 4
    yield base
    yield dict(base, filters="unfolded")
    yield dict(base, filters="unfolded", x_operand=True)
    if len(base["segs"]) == 1:
        yield dict(base, cmap="identity", x_operand=True)
        yield dict(base, cmap="identity", filters="unfolded")
    for name in R.OPERANDS:
        yield dict(base, off=dict(base["off"], **{name: 1}), filters="unfolded")
    yield dict(base, ws="null")
    yield dict(base, ws="short", filters="unfolded")
    yield dict(base, dxpad=2, filters="unfolded")
    yield dict(base, bias=False, off=dict(base["off"], bias=1))


# Route names no call can take in the default environment, with the reason and the source line.
IMPOSSIBLE = {
    "rgbin_fwd": "conv_rgbin_fwd_kernel needs W % 16 != 0 with 16 <= W <= 64 (launch_rgbin_fwd, conv.hip:1812-1842) and make_geo "
                 "admits powers of two only (:2361): W is 16, 32 or 64",
    "wino_fold5_unfold": "unfold_wgrad_kernel behind wino_wgrad needs KH = KW = 5 with pad != 2 (conv.hip:3709); wino_ok admits "
                         "stride 1 only, where TF 'SAME' pads a 5-tap filter by 2 on either side (:2357-2359)",
}
IMPOSSIBLE.update(R.IGEMM_UNREACHABLE)


def _admissible(Q):
    got = [set(), set(), set()]
    sample = GRID[:len(R.CASES)] + GRID[len(R.CASES)::6]
    for d in sample:
        g = R.make_geo(d)
        d16 = Q.dense16(d, g)
        if d16[0] is None:
            continue
        if d["y_accumulate"]:
            continue                                                      # (covered by the table's own y_accumulate cases below)
        for c in _call_variants(d):
            for which in (0, 1, 2):
                got[which].add(_fmt(R.expected_route(c, which, d16, Q.operand_bytes(d) > 0)))
    return got


def _split(route):
    """(family, tile configuration or None): the implicit-GEMM families share launch_igemm, whose choice depends on the
    family only through its arguments (rows, columns, classes, records)"""
    fam, _, cfg = route.partition(":")
    return fam, (cfg or None)


def test_every_admissible_route_is_in_the_table(Q):
    """per pass: every route -- (family, tile configuration and main loop), what expected_route returns and what the kernel
    template is instantiated on -- that an admissible call of the grid can take is in the table"""
    admissible = _admissible(Q)
    problems = []
    for which in (0, 1, 2):
        covered = {_fmt(c["expect"][which]) for c in R.CASES if which in c["passes"]}
        missing = sorted(admissible[which] - covered)
        print("%s: %d admissible routes, the table reaches %d of them (%d table routes in all)"
              % (PASS[which], len(admissible[which]), len(admissible[which] & covered), len(covered)))
        if missing:
            problems.append((PASS[which], missing))
        fam_a, fam_c = {_split(r)[0] for r in admissible[which]}, {_split(r)[0] for r in covered}
        stray = sorted(fam_c - fam_a)
        assert not stray, ("the table claims routes the enumeration never meets", PASS[which], stray)
        for name in IMPOSSIBLE:
            assert name not in fam_a and name not in fam_c, name
    assert not problems, problems
    for name, why in sorted(IMPOSSIBLE.items()):
        print("impossible: %s -- %s" % (name, why))
    # the kernel named in the first entry really is out of reach: no power of two in [16, 64] leaves a remainder modulo 16
    assert all(w % 16 == 0 for w in (16, 32, 64))
    # every epilogue of the input-gradient implicit GEMM on the vector and on the scalar loaders
    dg = {_split(c["expect"][1]) for c in R.CASES if 1 in c["passes"] and not R.is_error(c["expect"][1])}
    for epi in ("plain", "act", "pair"):
        cfgs = {cfg for fam, cfg in dg if fam.endswith("." + epi)}
        assert any(c.endswith("scalar") for c in cfgs) and any(not c.endswith("scalar") for c in cfgs), (epi, cfgs)
    # ... and the y_accumulate routes the header names are in the table, with the rejection beside them
    fwd = {c["name"]: c["expect"].get(0) for c in R.CASES if c["y_acc"]}
    assert "wino_plain3" in fwd.values() and "dense16" in fwd.values() and any(R.is_error(v) for v in fwd.values()), fwd


def test_winograd_routes_are_the_ones_with_filters(Q):
    """for aligned, map-free calls with a full workspace: the forward / input-gradient route is a Winograd one exactly when
    the layer has Winograd-domain filters for that pass, the weight-gradient route exactly when forward and weight gradient
    shares an operand"""
    for d in GRID[::3]:
        if d["y_accumulate"]:
            continue
        g = R.make_geo(d)
        d16 = Q.dense16(d, g)
        if d16[0] is None:
            continue
        c = next(_call_variants(dict(d, list_quads=1)))
        c = dict(c, filters="unfolded")
        routes = [R.expected_route(c, w, d16, Q.operand_bytes(d) > 0) for w in (0, 1, 2)]
        assert R.is_wino(routes[0]) == (Q.filter_bytes(d, 0) > 0 or Q.filter_bytes(d, 2) > 0), (d, routes)
        assert R.is_wino(routes[1]) == (Q.filter_bytes(d, 1) > 0 or Q.filter_bytes(d, 3) > 0), (d, routes)
        assert R.is_wino(routes[2]) or Q.operand_bytes(d) == 0, (d, routes)      # (the operand: a necessary condition only)


# ------------------------------------------------------------------------------------------------------------------
# the benchmarked layers
# ------------------------------------------------------------------------------------------------------------------
def _model_layers():
    """(name, case) of every convolution the models run through ops.conv2d_op, shapes read from the model files; the dense
    blocks' own layers belong to the dense-block planner of ops.py"""
    from otgan_amd.models import dcgan, densenet
    out = []
    for size, nb in ((32, 256), (64, 512)):                               # BASELINE.json: 32 x 32 at 2 x 128, 64 x 64 at 2 x 256
        C, H = 3, size
        for k, (filters, s, act) in enumerate(dcgan._CRITIC):
            for n in (nb, 2 * nb):
                out.append(("dcgan%d critic conv2d_%d N=%d" % (size, k, n),
                            R._c("m", n, H, H, (C,), filters, 5, stride=s, pre=R.ACT_CRELU if act else R.ACT_NONE, filters="own")))
            C, H = filters, H // s
        C, H = 1024, size // 8
        for k, filters in enumerate(dcgan._GEN):
            out.append(("dcgan%d generator conv2d_%d N=%d" % (size, k, nb), R._c("m", nb, H, H, (C,), filters, 5, up=1, filters="unfolded")))
            C, H = filters // 2, 2 * H
        out.append(("dcgan%d generator conv2d_3 N=%d" % (size, nb), R._c("m", nb, H, H, (C,), 3, 5)))
    sig = inspect.signature(densenet.disc_spec).parameters
    L, F = sig["layers_per_block"].default, sig["filters_per_layer"].default
    assert densenet.IMAGE_SIZES == (32, 64)
    for size, nb in ((32, 256), (64, 256)):
        room = L * F
        for n in (nb, 2 * nb):
            out.append(("densenet%d critic conv2d_0 N=%d" % (size, n), R._c("m", n, size, size, (3,), 2 * F, 3, ypad=room)))
            C, H = 2 * F, size
            for stage in range(3):
                segs = (C,) + (F,) * L
                width = sum(segs)
                out.append(("densenet%d critic transition %d N=%d" % (size, stage, n),
                            R._c("m", n, H, H, segs, width // 2, 3, stride=2, pre=R.ACT_CRELU, ypad=room if stage < 2 else 0)))
                C, H = width // 2, H // 2
        C, H = F, size // 4
        for stage in range(2):
            segs = (C, F) + (F,) * L
            width = sum(segs)
            out.append(("densenet%d generator transition %d N=%d" % (size, stage, nb),
                        R._c("m", nb, H, H, segs, width // 2, 3, up=1, pre=R.ACT_CRELU, ypad=F + L * F, filters="unfolded")))
            C, H = width // 2, 2 * H
        out.append(("densenet%d generator conv2d_last N=%d" % (size, nb), R._c("m", nb, H, H, (C, F) + (F,) * L, 3, 3, pre=R.ACT_CRELU)))
    return out


PINNED = """
dcgan32 critic conv2d_0 N=256: rgbin_mfma_tpb2 | fewin_mfma | outer2_mfma
dcgan32 critic conv2d_0 N=512: rgbin_mfma_tpb2 | fewin_mfma | outer2_mfma
dcgan32 critic conv2d_1 N=256: wino_s2 | wino_s2 | wino_s2
dcgan32 critic conv2d_1 N=512: wino_s2 | wino_s2 | wino_s2
dcgan32 critic conv2d_2 N=256: wino_s2 | wino_s2 | wino_s2
dcgan32 critic conv2d_2 N=512: wino_s2 | wino_s2 | wino_s2
dcgan32 critic conv2d_3 N=256: wino_s2 | wino_s2 | wino_s2
dcgan32 critic conv2d_3 N=512: wino_s2 | wino_s2 | wino_s2
dcgan32 generator conv2d_0 N=256: wino_fold5 | wino_fold5 | wino_fold5_fused
dcgan32 generator conv2d_1 N=256: wino_fold5 | wino_fold5 | wino_fold5_fused
dcgan32 generator conv2d_2 N=256: wino_fold5 | wino_fold5 | wino_fold5_fused
dcgan32 generator conv2d_3 N=256: fewout_mfma | rgbout_dgrad | outer1_mfma
dcgan64 critic conv2d_0 N=512: rgbin_mfma_tpb2 | fewin_mfma | outer2_mfma
dcgan64 critic conv2d_0 N=1024: rgbin_mfma_tpb2 | fewin_mfma | outer2_mfma
dcgan64 critic conv2d_1 N=512: wino_s2 | wino_s2 | wino_s2
dcgan64 critic conv2d_1 N=1024: wino_s2 | wino_s2 | wino_s2
dcgan64 critic conv2d_2 N=512: wino_s2 | wino_s2 | wino_s2
dcgan64 critic conv2d_2 N=1024: wino_s2 | wino_s2 | wino_s2
dcgan64 critic conv2d_3 N=512: wino_s2 | wino_s2 | wino_s2
dcgan64 critic conv2d_3 N=1024: wino_s2 | wino_s2 | wino_s2
dcgan64 generator conv2d_0 N=512: wino_fold5 | wino_fold5 | wino_fold5_fused
dcgan64 generator conv2d_1 N=512: wino_fold5 | wino_fold5 | wino_fold5_fused
dcgan64 generator conv2d_2 N=512: wino_fold5 | wino_fold5 | wino_fold5_fused
dcgan64 generator conv2d_3 N=512: fewout_mfma | rgbout_dgrad | outer1_mfma
densenet32 critic conv2d_0 N=256: igemm:Narrow_scalar | fewin_tile | outer2_mfma
densenet32 critic transition 0 N=256: igemm:W160_x2h | igemm.pair:Main16_x2h | igemm:W160_vec_split
densenet32 critic transition 1 N=256: igemm_ksplit:W224_x2h | igemm.pair:Main16_x2h | igemm:W224_vec_split
densenet32 critic transition 2 N=256: igemm_ksplit:Small16_x2h | igemm.pair:Main16_x2h | igemm:Main_vec_split
densenet32 critic conv2d_0 N=512: igemm:Narrow_scalar | fewin_tile | outer2_mfma
densenet32 critic transition 0 N=512: igemm:W160_x2h | igemm.pair:Main16_x2h | igemm:W160_vec_split
densenet32 critic transition 1 N=512: igemm_ksplit:W224_x2h | igemm.pair:Main16_x2h | igemm:W224_vec_split
densenet32 critic transition 2 N=512: igemm_ksplit:Main16_x2h | igemm.pair:Main16_x2h | igemm:Main_vec_split
densenet32 generator transition 0 N=256: wino_up3 | wino_up3 | wino_up3
densenet32 generator transition 1 N=256: wino_up3 | wino_up3 | wino_up3
densenet32 generator conv2d_last N=256: fewout_mfma | rgbout_dgrad | outer1_mfma
densenet64 critic conv2d_0 N=256: igemm:Narrow_scalar | fewin_tile | outer2_mfma
densenet64 critic transition 0 N=256: igemm:W160_x2h | igemm.pair:Main16_x2h | igemm:W160_vec_split
densenet64 critic transition 1 N=256: igemm:W224_x2h | igemm.pair:Main16_x2h | igemm:W224_vec_split
densenet64 critic transition 2 N=256: igemm_ksplit:Main16_x2h | igemm.pair:Main16_x2h | igemm:Main_vec_split
densenet64 critic conv2d_0 N=512: igemm:Narrow_scalar | fewin_tile | outer2_mfma
densenet64 critic transition 0 N=512: igemm:W160_x2h | igemm.pair:Main16_x2h | igemm:W160_vec_split
densenet64 critic transition 1 N=512: igemm:W224_x2h | igemm.pair:Main16_x2h | igemm:W224_vec_split
densenet64 critic transition 2 N=512: igemm_ksplit:Main16_x2h | igemm.pair:Main16_x2h | igemm:Main_vec_split
densenet64 generator transition 0 N=256: wino_up3 | wino_up3 | wino_up3
densenet64 generator transition 1 N=256: wino_up3 | wino_up3 | wino_up3
densenet64 generator conv2d_last N=256: fewout_mfma | rgbout_dgrad | outer1_mfma
"""


def test_benchmarked_layers_keep_their_routes(Q):
    lines = []
    for name, c in _model_layers():
        lines.append("%s: %s" % (name, " | ".join(_fmt(_route(Q, c, w)) for w in (0, 1, 2))))
    got = "\n".join(lines)
    if got != PINNED.strip():
        print(got)
    assert got == PINNED.strip()


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
def _loop_conv(xs, w, b, pre, stride, up):
    """plain fp64 loops: explicit TF 'SAME' padding (the extra pixel after), nearest-neighbour doubling, the per-element
    [x, -x] interleave of CReLU / CELU (reference utils/nn.py:190-206, 234-241)"""
    xs = [np.asarray(x, np.float64) for x in xs]
    if up:
        x = np.concatenate(xs, 3)
        big = np.zeros((x.shape[0], 2 * x.shape[1], 2 * x.shape[2], x.shape[3]))
        for i in range(big.shape[1]):
            for j in range(big.shape[2]):
                big[:, i, j] = x[:, i // 2, j // 2]
        xs = [big]
    if pre in ("crelu", "celu"):
        xs = [s for x in xs for s in (x, -x)]
    a = np.concatenate(xs, 3)
    if pre in ("crelu", "relu"):
        a = np.maximum(a, 0.0)
    elif pre in ("celu", "elu"):
        a = np.where(a > 0, a, np.expm1(np.minimum(a, 0.0)))
    N, H, W, C = a.shape
    KH, KW, _, Cout = w.shape
    OH, OW = -(-H // stride), -(-W // stride)
    ph, pw = max((OH - 1) * stride + KH - H, 0), max((OW - 1) * stride + KW - W, 0)
    pad = np.zeros((N, H + ph, W + pw, C))
    pad[:, ph // 2:ph // 2 + H, pw // 2:pw // 2 + W] = a
    y = np.zeros((N, OH, OW, Cout))
    for oh in range(OH):
        for ow in range(OW):
            for kh in range(KH):
                for kw in range(KW):
                    y[:, oh, ow] += pad[:, oh * stride + kh, ow * stride + kw] @ w[kh, kw]
    return y + b


@pytest.mark.parametrize("K", [(1, 1), (2, 2), (4, 4), (1, 5), (5, 1), (2, 3)], ids=lambda k: "%dx%d" % k)
def test_oracle_against_plain_loops(K):
    """oracle.nets_torch.conv2d in fp64 against the loops above: relative L2 below 1e-12 (fp64 rounding of sums of at most a few
    hundred terms)"""
    from oracle import nets_torch as NT
    gen = torch.Generator().manual_seed(K[0] * 7 + K[1])
    for stride, up, pre, segs in ((1, False, "crelu", (3, 5)), (2, False, "celu", (3, 5)), (1, True, "crelu", (5, 3)), (2, True, None, (7,)),
                                  (2, False, "relu", (1, 2, 3)), (1, True, "elu", (3,))):
        C = sum(segs)
        mult = 2 if pre in ("crelu", "celu") else 1
        xs = [torch.randn(2, 4, 8, s, generator=gen, dtype=torch.float64) for s in segs]
        V = torch.randn(K[0], K[1], C * mult, 5, generator=gen, dtype=torch.float64)
        g = torch.rand(5, generator=gen, dtype=torch.float64) + 0.5
        b = torch.randn(5, generator=gen, dtype=torch.float64)
        y = NT.conv2d(xs, dict(V=V, g=g, b=b), pre, stride, up)
        w = NT.weight_norm(V, g)
        # with upsampling the reference concatenates the list BEFORE the activation (nn.py:235-236): [x, -x] of the whole
        ref = _loop_conv([x.numpy() for x in xs], w.numpy(), b.numpy(), pre, stride, up)
        e = np.linalg.norm(y.numpy() - ref) / np.linalg.norm(ref)
        assert y.shape == ref.shape and e < 1e-12, (K, stride, up, pre, e)
        # the composition the table's reference differentiates (conv_routes.oracle_pieces) is the same function
        y2 = R.oracle_pieces(NT, xs, w, b, pre, stride, up)
        assert float((y2 - y).norm() / y.norm()) < 1e-14


_GEOMETRIES = {}
for _case in R.CASES:
    _GEOMETRIES.setdefault(R.base_name(_case), _case)


@pytest.mark.parametrize("case", list(_GEOMETRIES.values()), ids=[c["name"] for c in _GEOMETRIES.values()])
def test_reference_alone_is_well_inside_the_tolerance(case):
    """the oracle evaluated in fp32 on the table's inputs is within TOL / 10 of its fp64 value for y, dx and dw: the bound is
    left to the kernels; the gradients satisfy the adjoint identities of the forward map (bilinear in (act(x), w))"""
    grads = case["N"] * case["H"] * case["W"] <= 8192 or any(w in c["passes"] for c in R.CASES if R.base_name(c) == R.base_name(case)
                                                             for w in (1, 2))
    ref = R.oracle(case, grads=grads) if not grads else R.reference(case)
    low = R.oracle(case, dtype=torch.float32, grads=grads)
    worst = {}
    for k in ref:
        e = float((low[k].double() - ref[k]).norm() / ref[k].norm())
        worst[k] = e
        assert torch.isfinite(ref[k]).all() and float(ref[k].norm()) > 0
        assert e < TOL / 10, (case["name"], k, e)
    print(case["name"], " ".join("%s %.1e" % kv for kv in sorted(worst.items())))
    if grads:
        inp = R.inputs(case)
        b = inp["bias"].double() if case["bias"] else 0.0
        lhs = float(((ref["y"] - b) * inp["dy"].double()).sum())
        assert abs(lhs - float((inp["w"].double() * ref["dw"]).sum())) <= 1e-10 * max(abs(lhs), 1.0)        # linear in w
        if case["pre"] in (R.ACT_NONE, R.ACT_CRELU, R.ACT_RELU):                                           # positively homogeneous in x
            assert abs(lhs - float((inp["x"].double() * ref["dx"]).sum())) <= 1e-10 * max(abs(lhs), 1.0)
