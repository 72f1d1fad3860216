"""The calls that pin the three convolution passes (otgan_conv2d_fwd_pf_f32, otgan_conv2d_dgrad_pf_f32, otgan_conv2d_wgrad_f32)
to every kernel route of csrc/conv.hip, and the route predicates restated in Python.  tests/test_conv_routes_cpu.py keeps the
table on the routes it claims and compares the restatement with the library's host queries; tests/test_conv_routes_gpu.py runs
the table through the C ABI; tests/test_conv_sparse_gpu.py runs its non-Winograd routes a second time, on the sparse inputs of
tests/conv_sparse.py with one error bar per output element (worst error / bar per route family: in its docstring), and
tests/test_amax_bounds_gpu.py its two-fp16-piece routes under amax records above the exact maximum.  No GPU and no library is
needed to import this module.

The three bodies (conv2d_fwd_body, conv2d_dgrad_body, otgan_conv2d_wgrad_f32) choose among about thirty kernels from the
descriptor, the alignment of every pointer, the pitches ldx / ldy / y_coff / lddx, the channel map, the workspace, `filters` and
tile counts.  ops.conv2d_op only ever passes packed, 16-byte aligned tensors with y_coff = 0, lddx = C, a full workspace and square
3x3 / 5x5 filters; everything else is reachable through the C ABI only.

A case (see `_c`): geometry N, H, W, segs (list-element widths, C = sum), Cout, KH, KW, stride, up, pre (OTGAN_ACT_*); pitch
paddings xpad / ypad / dxpad (floats added to C / y_coff + Cout / C); y_coff; `off`: floats (0..3) by which each operand pointer
(x, w, bias, y, dy, dx, dw, ws) is shifted from a 16-byte aligned base; ws: full / short (one byte under the query) / null;
filters: None / "own" (which = 0 forward, 1 input gradient: made from what the pass itself takes) / "unfolded" (which = 2, 3) /
"dummy" (an aligned buffer on a layer that has no Winograd filters); cmap: "auto" (the per-element interleave map exactly when
the reference interleaves: CReLU / CELU over a list without upsampling) or "identity" (an explicit map equal to the default
ordering); acc (dx += ...), y_acc, x_operand, bias; passes; and `expect`: per pass a route name or (code, fragment of
otgan_last_error()).  Route names assume the default environment (no OTGAN_* switch set).

Worst relative L2 error against the fp64 oracle per route family, measured on an MI355X by tests/test_conv_routes_gpu.py
(bound 2e-5, TOL of tests/test_layers_gpu.py):
  Winograd passes            wino_s2 1.2e-6 (forward), wino_plain3 8.8e-7, wino_up3 8.2e-7, wino_fold5 / _fused 8.6e-7
  folded implicit GEMM       fold4 / fold_percls 2.6e-7, fold.plain / .act / .pair 8.8e-7, igemm_fold (+ unfold_wgrad_kernel) 5.8e-7
  implicit GEMM, forward     every tile configuration, both main loops, K split, gather through the upsample: 6.5e-7 at most
  implicit GEMM, dgrad       4.8e-7 at most; through the virtual grid and pool2_sum_kernel (igemm_pool, with accumulate) 4.6e-7
  implicit GEMM, wgrad       4.0e-7 at most (W160_vec), with and without K splits
  few-channel kernels        fewout_mfma / _tile / _plain 3.7e-7, rgbin_mfma 1.5e-7, fewin_* 4.4e-7, rgbout_dgrad 1.5e-7,
                             outer1_* / outer2_* 2.2e-7
  growth kernels             dense16 forward 2.1e-7, input gradient 2.1e-7, weight gradient 6.7e-8 (one slab) / 8.1e-8 (slabs)
More than an order of magnitude under the bound on every route.  Before few_quads_ok (csrc/conv.hip) kept CReLU / CELU inputs
whose aligned quads of effective channels are not four consecutive source channels of one sign off the few-output kernels,
cout3_crelu_c6 returned relative errors of 5.7 (forward) and 4.8 (weight gradient), cout3_crelu_list_2_2 1.0 and 0.97.
"""
import math

OK, ERR_INVALID, ERR_WORKSPACE = 0, -1, -2
ACT_NONE, ACT_CRELU, ACT_CELU, ACT_ELU, ACT_RELU = 0, 1, 2, 3, 4
PRE_NAME = {0: None, 1: "crelu", 2: "celu", 3: "elu", 4: "relu"}
OPERANDS = ("x", "w", "bias", "y", "dy", "dx", "dw", "ws")
AMAX_RECORD_FLOATS = 512          # OTGAN_AMAX_RECORD_FLOATS, include/otgan_layers.h:126
FWD, DGRAD, WGRAD = 0, 1, 2


def _c(name, N, H, W, segs, Cout, K, stride=1, up=0, pre=0, xpad=0, ypad=0, dxpad=0, y_coff=0, off=None, ws="full",
       filters=None, cmap="auto", acc=0, y_acc=0, x_operand=False, bias=True, passes=(0, 1, 2), expect=None):
    KH, KW = (K, K) if isinstance(K, int) else K
    o = dict.fromkeys(OPERANDS, 0)
    o.update(off or {})
    return dict(name=name, N=N, H=H, W=W, segs=tuple(segs), Cout=Cout, KH=KH, KW=KW, stride=stride, up=up, pre=pre, xpad=xpad,
                ypad=ypad, dxpad=dxpad, y_coff=y_coff, off=o, ws=ws, filters=filters, cmap=cmap, acc=acc, y_acc=y_acc,
                x_operand=x_operand, bias=bias, passes=tuple(passes), expect=dict(expect or {}), base=None)


def variant(base, name, expect, **changes):
    """the case `base` with one property changed (a route twin or a refused call); `off` entries are merged"""
    c = dict(base, name=name, expect=dict(expect), base=base)
    off = dict(base["off"])
    off.update(changes.pop("off", {}))
    c.update(changes)
    c["off"] = off
    c["passes"] = tuple(c["passes"])
    c["expect"] = {w: e for w, e in c["expect"].items() if w in c["passes"]}
    return c


# ------------------------------------------------------------------------------------------------------------------
# geometry: make_geo, conv.hip:2344-2369
# ------------------------------------------------------------------------------------------------------------------
def doubled(pre):
    """conv.hip:2326 doubled_act"""
    return pre in (ACT_CRELU, ACT_CELU)


def act_kind(pre):
    """conv.hip:2327-2331: 0 none, 1 relu-type, 2 elu-type"""
    return 1 if pre in (ACT_CRELU, ACT_RELU) else (2 if pre in (ACT_CELU, ACT_ELU) else 0)


def is_pow2(v):
    return v >= 1 and (v & (v - 1)) == 0


def desc_fields(case):
    """the otgan_conv_desc of a case (geometry fields only)"""
    C = sum(case["segs"])
    return dict(N=case["N"], H=case["H"], W=case["W"], C=C, ldx=C + case["xpad"], upsample=case["up"], KH=case["KH"], KW=case["KW"],
                stride=case["stride"], Cout=case["Cout"], ldy=case["y_coff"] + case["Cout"] + case["ypad"], y_coff=case["y_coff"],
                preact=case["pre"], list_quads=1 if all(s % 4 == 0 for s in case["segs"]) else 0, y_accumulate=case["y_acc"])


def lddx(case):
    return sum(case["segs"]) + case["dxpad"]


def has_cmap(case):
    """whether the call passes a channel map (forward, weight gradient) / an inverse map (input gradient)"""
    if case["cmap"] == "identity":
        return True
    return doubled(case["pre"]) and len(case["segs"]) > 1 and not case["up"]


def map_quads(d):
    """conv.hip:2335"""
    return (not doubled(d["preact"])) or d["list_quads"] != 0


def make_geo(d):
    """conv.hip:2344-2369 -> dict, or the text of the check that fails"""
    if not (d["N"] > 0 and d["H"] > 0 and d["W"] > 0 and d["C"] > 0 and d["Cout"] > 0):
        return "bad conv sizes"
    if d["stride"] not in (1, 2):
        return "stride must be 1 or 2"
    if d["upsample"] not in (0, 1):
        return "upsample must be 0 or 1"
    if not (d["KH"] >= 1 and d["KW"] >= 1 and d["KH"] * d["KW"] <= 25):
        return "filter too large"
    if not (d["ldx"] >= d["C"] and d["ldy"] >= d["y_coff"] + d["Cout"]):
        return "bad leading dimensions"
    if not 0 <= d["preact"] <= 4:
        return "unknown pre-activation"
    g = dict(logUp=d["upsample"], Hin=d["H"] << d["upsample"], Win=d["W"] << d["upsample"])
    s = d["stride"]
    g["OH"], g["OW"] = (g["Hin"] + s - 1) // s, (g["Win"] + s - 1) // s
    ph, pw = (g["OH"] - 1) * s + d["KH"] - g["Hin"], (g["OW"] - 1) * s + d["KW"] - g["Win"]
    g["pad_t"], g["pad_l"] = max(ph, 0) // 2, max(pw, 0) // 2
    g["Ceff"] = d["C"] * (2 if doubled(d["preact"]) else 1)
    if not all(is_pow2(v) for v in (g["OH"], g["OW"], g["Hin"], g["Win"])):
        return "spatial sizes must be powers of two"
    g["fold"] = (d["upsample"] == 1 and s == 1 and map_quads(d) and g["Ceff"] % 16 == 0 and d["ldx"] % 4 == 0 and
                 d["Cout"] % 4 == 0 and d["ldy"] % 4 == 0 and d["y_coff"] % 4 == 0 and d["KH"] >= 2 and d["KW"] >= 2)   # :2366
    return g


def fold_delta(p, k, pad):
    """conv.hip:2240-2243: floor((p + k - pad) / 2)"""
    v = p + k - pad
    return v // 2 if v >= 0 else -((1 - v) // 2)


def fold_taps(d, g):
    """make_fold, conv.hip:2371-2389: (taps along h per parity, taps along w per parity, taps of the four classes)"""
    nth = [fold_delta(p, d["KH"] - 1, g["pad_t"]) - fold_delta(p, 0, g["pad_t"]) + 1 for p in (0, 1)]
    ntw = [fold_delta(p, d["KW"] - 1, g["pad_l"]) - fold_delta(p, 0, g["pad_l"]) + 1 for p in (0, 1)]
    return nth, ntw, [nth[c >> 1] * ntw[c & 1] for c in range(4)]


def folded_weight_elems(d, g):
    """make_fold(...).total, conv.hip:2381-2387"""
    return sum(fold_taps(d, g)[2]) * g["Ceff"] * d["Cout"] if g["fold"] else 0


# ------------------------------------------------------------------------------------------------------------------
# Winograd eligibility (kWinoM = 4, winograd.h:33)
# ------------------------------------------------------------------------------------------------------------------
def wino_ok(d, g):
    """conv.hip:2392-2395: folded 5x5 upsampling layers without pre-activation"""
    return (g["fold"] and d["KH"] == 5 and d["KW"] == 5 and d["preact"] == ACT_NONE and d["C"] % 32 == 0 and d["Cout"] % 4 == 0 and
            d["H"] % 4 == 0 and d["W"] % 4 == 0 and d["H"] >= 4 and d["W"] >= 4)


def wino_plain3_ok(d, g):
    """conv.hip:2411-2415 (thresholds :2409-2410)"""
    return (d["stride"] == 1 and d["upsample"] == 0 and d["KH"] == 3 and d["KW"] == 3 and d["C"] % 4 == 0 and g["Ceff"] % 16 == 0 and
            g["Ceff"] >= 64 and d["Cout"] % 32 == 0 and d["Cout"] >= 128 and d["H"] % 4 == 0 and d["W"] % 4 == 0 and
            d["ldx"] % 4 == 0 and d["ldy"] % 4 == 0 and d["y_coff"] % 4 == 0)


def wino_s2_ok(d, g):
    """conv.hip:2416-2421"""
    if wino_plain3_ok(d, g):
        return True
    return (d["stride"] == 2 and d["upsample"] == 0 and d["KH"] == 5 and d["KW"] == 5 and d["C"] % 4 == 0 and g["Ceff"] % 32 == 0 and
            d["Cout"] % 4 == 0 and d["H"] % 8 == 0 and d["W"] % 8 == 0 and d["ldx"] % 4 == 0 and d["ldy"] % 4 == 0 and
            d["y_coff"] % 4 == 0)


def wino_up3_ok(d, g):
    """conv.hip:2438-2442"""
    return (d["upsample"] == 1 and d["stride"] == 1 and d["KH"] == 3 and d["KW"] == 3 and d["preact"] == ACT_CRELU and
            d["C"] % 4 == 0 and g["Ceff"] == 2 * d["C"] and g["Ceff"] % 32 == 0 and d["Cout"] % 4 == 0 and (2 * d["H"]) % 4 == 0 and
            (2 * d["W"]) % 4 == 0 and d["ldx"] % 4 == 0 and d["ldy"] % 4 == 0 and d["y_coff"] % 4 == 0)


def wino_up3_wgrad_ok(d, g):
    """conv.hip:2454-2456"""
    return wino_up3_ok(d, g) and d["Cout"] % 16 == 0 and (d["N"] * (2 * d["H"] // 4) * (2 * d["W"] // 4)) % 32 == 0


def wino_up3_dgrad_ok(d, g):
    """conv.hip:2466-2468"""
    return wino_up3_ok(d, g) and d["Cout"] % 4 == 0


def filter_bytes_positive(d, g, which):
    """otgan_conv2d_filter_bytes > 0, conv.hip:2983-2994 (the sizes themselves are the library's)"""
    if which not in (0, 1, 2, 3):
        return False
    if wino_s2_ok(d, g):
        return which < 2
    if wino_ok(d, g):
        return True
    if wino_up3_ok(d, g):
        return which == 2 or (which == 3 and wino_up3_dgrad_ok(d, g))
    return False


def operand_bytes_possible(d, g):
    """necessary for otgan_conv2d_operand_bytes > 0, conv.hip:2996-3003; whether the Winograd passes of such a layer do share an
    operand is decided by winograd.hip's size formulas (tile counts, GEMM engine), which the tests ask the library for"""
    return wino_s2_ok(d, g) or wino_ok(d, g) or (wino_up3_ok(d, g) and wino_up3_wgrad_ok(d, g))


def glu_fused(d, g):
    """otgan_conv2d_glu_fused, conv.hip:3130-3134"""
    return wino_ok(d, g) and d["Cout"] % 8 == 0 and d["y_coff"] == 0 and d["ldy"] == d["Cout"] and not d.get("y_accumulate", 0)


def rgbin_shape(d):
    """the RGB-in clause of otgan_conv2d_amax_fused, conv.hip:3031-3033 == the refusal list of launch_rgbin_fwd, :1812-1829"""
    return (d["C"] == 3 and d["stride"] == 1 and d["upsample"] == 0 and d["KH"] == d["KW"] and d["KH"] in (3, 5) and
            d["Cout"] % 128 == 0 and 16 <= d["W"] <= 64 and 256 // d["W"] >= 4 and 256 // d["W"] <= d["H"] and
            d["H"] % (256 // d["W"]) == 0)


def amax_fused(d, g, which):
    """otgan_conv2d_amax_fused, conv.hip:3022-3050"""
    if which == 0:
        if d["Cout"] % 4 or d["ldy"] % 4 or d["y_coff"] % 4:
            return 0
        if wino_s2_ok(d, g):
            return 1
        if wino_up3_ok(d, g) and not wino_ok(d, g) and not d.get("y_accumulate", 0):
            return 1
        if d.get("y_accumulate", 0):
            return int(d["Cout"] == 16)
        if d["preact"] == ACT_NONE and rgbin_shape(d):
            return 1
        return int(not wino_ok(d, g) and not g["fold"] and not wino_up3_ok(d, g) and d["Cout"] > 4)
    if which == 1:
        if d["C"] % 4:
            return 0
        if wino_s2_ok(d, g):
            return 1
        if wino_up3_dgrad_ok(d, g) and not wino_ok(d, g):
            return 1
        if (d["Cout"] == 3 and d["stride"] == 1 and d["upsample"] == 0 and d["KH"] == d["KW"] and d["KH"] in (3, 5) and
                d["W"] % 16 == 0 and d["H"] % 4 == 0):
            return 1
        return int(not wino_ok(d, g) and not g["fold"] and not wino_up3_dgrad_ok(d, g) and not d["upsample"] and d["C"] > 4 and
                   d["Cout"] > 4 and not (d["Cout"] == 16 and d["KH"] == 3 and d["KW"] == 3 and d["stride"] == 1))
    return 0


# ------------------------------------------------------------------------------------------------------------------
# the implicit-GEMM tile choice: launch_igemm, conv.hip:2675-2739, in the default environment (igemm_x3s() true, :2664)
# ------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def igemm_cfg(epi_fwd, vec, Ck, rows, ncols, paired, ncls, recs, cmap=False):
    """tile configuration and main loop.  `recs`: both amax records at hand (igemm_records, conv.hip:1784-1806) -> the
    two-scaled-fp16-piece loop ("x2h"), else three bf16 pieces ("x3s") (launch_igemm3_x3s, :2650-2663)"""
    ntiles = cdiv(ncols, 64) if paired else cdiv(ncols, 128)
    loop = "x2h" if recs and (not cmap or 4 * Ck <= 8192) else "x3s"                                      # :2654
    if not paired and ncols <= 32:                                                                        # :2679-2692
        return ("N16" if ncols <= 16 else "Narrow") + ("_vec" if vec and Ck % 16 == 0 else "_scalar")
    if epi_fwd and not paired and vec:
        if Ck % 32 == 0 and 128 < ncols <= 160 and cdiv(rows, 128) * ncls >= 256:                         # :2695
            return "W160_" + loop
        if Ck % 16 == 0 and 192 < ncols <= 224 and cdiv(rows, 128) * ncls >= 256:                         # :2701
            return "W224_" + loop
    if vec and Ck % 4 == 0:                                                                               # :2708-2718
        return ("Small16_" if cdiv(rows, 128) * ntiles * ncls < 512 else "Main16_") + loop
    return "Main16_scalar"                                                                                # :2736-2738


# launch_igemm branches no call reaches in the default environment (tests/test_conv_routes_cpu.py IMPOSSIBLE quotes these)
IGEMM_UNREACHABLE = {
    "CfgSmall / CfgMain (fp32 MFMA, BK = 32), conv.hip:2719-2729": "vec_ok && Ck % 32 == 0 implies vec_ok && Ck % 4 == 0, which "
    "returns at :2708-2718 while OTGAN_IGEMM_X3 is unset",
    "CfgSmall16 on the fp32 loop, conv.hip:2730-2735": "the same: vec_ok && Ck % 16 == 0 returns at :2708-2718",
    "CfgMain16 <VEC = true> on the fp32 loop, conv.hip:2737": "the same: vec_ok && Ck % 4 == 0 returns at :2708-2718",
    "CfgW160 (BK = 32) / CfgW224 on the fp32 loop, conv.hip:2698,2704": "igemm_x3s() is true unless OTGAN_IGEMM_X3=0",
}


def igemm_fwd_ksplit(d, g, vec, Mtot):
    """conv.hip:2809-2827"""
    if not vec or g["fold"] or d["upsample"] or d["Cout"] % 4 or d["ldy"] % 4 or d["y_coff"] % 4 or g["Ceff"] % 4:
        return 1
    if d["Cout"] <= 32:
        return 1
    tiles = cdiv(Mtot, 64) * cdiv(d["Cout"], 128)
    if tiles >= 2048:
        return 1
    nsl = cdiv(g["Ceff"], 16)
    ks = min(2048 // tiles, nsl // 8, 8)
    return 1 if ks < 2 else ks


RECS_BYTES = 256 + 2 * 4 * AMAX_RECORD_FLOATS        # conv.hip:2848


def align_up(x, a):
    return cdiv(x, a) * a


def generic_fwd_workspace(d, g):
    """the non-Winograd part of otgan_conv2d_workspace_bytes(d, 0), conv.hip:2864-2870"""
    vec = map_quads(d) and g["Ceff"] % 16 == 0 and d["ldx"] % 4 == 0
    Mtot = d["N"] * g["OH"] * g["OW"]
    ks = igemm_fwd_ksplit(d, g, vec, Mtot)
    return align_up(RECS_BYTES, 256) + 4 * ks * Mtot * d["Cout"] if ks > 1 else RECS_BYTES


def generic_dgrad_workspace(d, g):
    """conv.hip:2849-2854: the virtual-grid gradient of an un-folded upsampling layer, then the scratch records"""
    return (align_up(4 * d["N"] * g["Hin"] * g["Win"] * d["C"], 256) if d["upsample"] and not g["fold"] else 0) + RECS_BYTES


# ------------------------------------------------------------------------------------------------------------------
# plan_wgrad, conv.hip:2483-2579.  `dense16`: (ok, nsplit) of dense16_tiling for this geometry -- not restated; the tests get it
# from the library (otgan_conv2d_workspace_bytes(d, 2), see dense16_from_query)
# ------------------------------------------------------------------------------------------------------------------
def dense16_wgrad_desc(d):
    """conv.hip:2488-2489"""
    return (d["Cout"] == 16 and d["KH"] == 3 and d["KW"] == 3 and d["stride"] == 1 and d["upsample"] == 0 and d["C"] % 4 == 0 and
            d["ldx"] % 4 == 0 and d["ldy"] % 4 == 0 and d["y_coff"] % 4 == 0)


def plan_wgrad(d, g, dense16=(False, 0)):
    taps = d["KH"] * d["KW"]
    p = dict(dense16=False, outer=0, wide=0, vec=False, fold=False, narrow=False, n16=False)
    if dense16_wgrad_desc(d) and dense16[0]:
        p.update(dense16=True, nsplit=dense16[1], slab_elems=taps * g["Ceff"] * d["Cout"], M=d["N"] * d["H"] * d["W"])
        return p
    p["vec"] = (map_quads(d) and g["Ceff"] % 4 == 0 and d["Cout"] % 4 == 0 and d["ldy"] % 4 == 0 and d["y_coff"] % 4 == 0 and
                d["ldx"] % 4 == 0 and g["Ceff"] >= 32)                                                    # :2500-2501
    p["fold"] = g["fold"] and p["vec"]
    if d["upsample"] == 0:                                                                                # :2505-2508
        if d["Cout"] <= 4 and fewout_quads_ok(d):
            p["outer"] = 1
        elif g["Ceff"] <= 4 and d["preact"] == ACT_NONE:
            p["outer"] = 2
    if p["outer"]:                                                                                        # :2509-2530
        M = d["N"] * g["OH"] * g["OW"]
        nchunks = 256 if M >= 256 * 64 else cdiv(M, 64)
        if d["stride"] == 1 and M >= 512 * 64:
            nchunks = 512
        chunk = cdiv(M, nchunks)
        if d["stride"] == 1:
            unit = outer_unit_rows(d["H"]) * d["W"]
            chunk = cdiv(chunk, unit) * unit
        nchunks = cdiv(M, chunk)
        p.update(fold=False, vec=False, M=M, chunk=chunk, nsplit=nchunks, slab_elems=taps * g["Ceff"] * d["Cout"])
        return p
    p["narrow"], p["n16"] = d["Cout"] <= 32, d["Cout"] <= 16
    if p["vec"] and 128 < d["Cout"] <= 160:
        p["wide"] = 160
    if p["vec"] and 192 < d["Cout"] <= 224:
        p["wide"] = 224
    BM = 256 if p["narrow"] else 128                                                                      # CfgNarrow::BM, :49
    BN = p["wide"] or (16 if p["n16"] else (32 if p["narrow"] else 128))
    bk = 16 if p["wide"] == 224 else (32 if p["vec"] and not p["narrow"] else 16)                         # :2539
    if p["fold"]:
        cls_taps = fold_taps(d, g)[2]
        p["slab_elems"], nz, M = folded_weight_elems(d, g), sum(cls_taps), d["N"] * d["H"] * d["W"]
        tiles_m = cdiv(g["Ceff"], BM)
    else:
        p["slab_elems"], M = taps * g["Ceff"] * d["Cout"], d["N"] * g["OH"] * g["OW"]
        tiles_m, nz = (cdiv(g["Ceff"], BM), taps) if p["vec"] else (cdiv(taps * g["Ceff"], BM), 1)
    tiles_n = cdiv(d["Cout"], BN)
    nkt = cdiv(M, bk)
    blocks = tiles_m * tiles_n * nz
    per_round = 256 * (2 if p["vec"] and not p["narrow"] else 4)
    want, best = 1, -1.0
    for ns in range(1, 17):                                                                               # :2567-2575
        if ns > 1 and nkt // ns < 16:
            break
        b = blocks * ns
        eff = b / (cdiv(b, per_round) * per_round) - 0.004 * (ns - 1)
        if eff > best + 1e-9:
            best, want = eff, ns
    kt_per_split = cdiv(nkt, want)
    p.update(M=M, bk=bk, nsplit=cdiv(nkt, kt_per_split))
    return p


def outer_unit_rows(H):
    """conv.hip:2470"""
    return 8 if H >= 8 else H


def fewout_quads_ok(d):
    """The few-output kernels (conv_fewout_kernel and its tile / MFMA variants, conv_outer_kernel and its variants with the
    layer input as the wide operand) read the effective channels four at a time through ONE channel-map entry: every aligned
    quad must be four consecutive source channels with one sign (conv.hip: few_quads_ok)."""
    return map_quads(d) and (not doubled(d["preact"]) or d["C"] % 4 == 0)


def wgrad_workspace_generic(d, g, p):
    """the non-Winograd part of otgan_conv2d_workspace_bytes(d, 2), conv.hip:2856-2863"""
    slabs = p["slab_elems"] * p["nsplit"] if (p["nsplit"] > 1 or p["fold"] or p["outer"]) else 0
    if p["fold"] and p["nsplit"] > 1:
        slabs += p["slab_elems"]
    return align_up(4 * slabs, 256) + 256


def dense16_from_query(d, g, wgrad_bytes):
    """(ok, nsplit) of dense16_tiling from otgan_conv2d_workspace_bytes(d, 2) of a descriptor that passes dense16_wgrad_desc and
    no Winograd predicate: with the dense16 plan the query is 256 (nsplit == 1) or align_up(4 * nsplit * 9 * Ceff * 16, 256) + 256,
    with the generic plan what wgrad_workspace_generic gives.  (None, 0): both plans give the same size -- undecidable."""
    slab_bytes = 4 * 9 * g["Ceff"] * 16                   # a multiple of 256: C % 4 == 0
    gen = wgrad_workspace_generic(d, g, plan_wgrad(d, g, (False, 0)))
    body = wgrad_bytes - 256
    if body == 0:
        nsplit = 1
    elif body % slab_bytes == 0 and body // slab_bytes >= 2:
        nsplit = body // slab_bytes
    else:
        assert wgrad_bytes == gen, (d, wgrad_bytes, gen)
        return False, 0
    return (True, nsplit) if wgrad_bytes != gen else (None, 0)


def canonical_dense16_desc(d, g):
    """a growth-layer descriptor of the same N, H, W, Ceff that passes dense16_wgrad_desc and no Winograd predicate"""
    return dict(N=d["N"], H=d["H"], W=d["W"], C=g["Ceff"], ldx=g["Ceff"], upsample=0, KH=3, KW=3, stride=1, Cout=16, ldy=16, y_coff=0,
                preact=ACT_NONE, list_quads=1, y_accumulate=0)


def dense16_of(query, d, g, h2_ok=None):
    """(ok, nsplit) of dense16_tiling(N, H, W, Ceff) through `query(desc_fields, which) -> bytes` (the library's
    otgan_conv2d_workspace_bytes); (False, 0) at once where no route asks (16 outputs, 3x3, stride 1 only).  Where both plans
    ask for the same workspace, `h2_ok(desc_fields) -> bool` (otgan_dense16_h2_ok of a growth layer of this N, H, W) decides
    if it says yes: the fp16 growth kernels take a subset of the geometries of the fp32 ones (dense16_h2_shape_ok,
    dense16.hip:1810-1814, against dense16_tiling, :1936-1943: the same tile search, fewer widths)."""
    if not (d["Cout"] == 16 and d["KH"] == 3 and d["KW"] == 3 and d["stride"] == 1 and d["upsample"] == 0) or g["Ceff"] % 4:
        return False, 0
    cd = canonical_dense16_desc(d, g)
    bytes2 = query(cd, 2)
    ok, nsplit = dense16_from_query(cd, make_geo(cd), bytes2)
    if ok is None and h2_ok is not None:
        hd = dict(cd, C=16, ldx=16, preact=ACT_CRELU, y_accumulate=1, list_width=16)
        if h2_ok(hd):
            return True, 1 if bytes2 == 256 else (bytes2 - 256) // (4 * 9 * g["Ceff"] * 16)
    return ok, nsplit


# ------------------------------------------------------------------------------------------------------------------
# the few-channel launchers' refusal lists
# ------------------------------------------------------------------------------------------------------------------
def fewout_descent(sa, logUp, so, J, KH, KW, gridH, gridW, srcH, srcW, N, Ck, ld, sJ, dws, boff_quads, dh_ok):
    """launch_fewout_mfma (conv.hip:1452-1485), then launch_fewout_tile (:1274-1307), then conv_fewout_kernel"""
    mfma = (sa == 1 and logUp == 0 and so == 1 and J >= 1 and KW * J <= 16 and KH in (3, 5) and gridW == srcW and gridH == srcH and
            gridW in (16, 32, 64) and gridH % 4 == 0 and Ck % 64 == 0 and ld % 4 == 0 and sJ % 4 == 0 and
            all(-2 <= v <= 2 for v in dws) and boff_quads and dh_ok and (N * gridH) % 16 == 0)
    if mfma:
        return "mfma"
    tile = sa == 1 and logUp == 0 and J in (3, 4) and so == 1 and gridW == srcW and gridH == srcH and 16 <= gridW <= 64
    if tile:
        TR = 256 // gridW
        tile = TR <= gridH and gridH % TR == 0 and TR % 2 == 0
        lds = 16 * (5 * (TR + KH - 1) * (gridW + KW - 1) + KH * KW * (3 if J == 3 else 4) * 4)
        tile = tile and lds <= 80 * 1024
    return "tile" if tile else "plain"


def fewout_fwd(d, g):
    """the descent as conv2d_fwd_body calls it (conv.hip:3287-3310): ga from fill_gather_x(GH = OH, GW = OW, sa = stride)"""
    dws = [kw - g["pad_l"] for kw in range(d["KW"])]
    return fewout_descent(d["stride"], g["logUp"], 1, d["Cout"], d["KH"], d["KW"], g["OH"], g["OW"], d["H"], d["W"], d["N"], g["Ceff"],
                          d["ldx"], d["KH"] * d["KW"] * g["Ceff"], dws, g["Ceff"] % 4 == 0, g["pad_t"] == (d["KH"] - 1) // 2)


def fewin_dgrad(d, g):
    """the descent as conv2d_dgrad_body calls it (conv.hip:3445-3470): source dy, J = C outputs, taps (pad - kh, pad - kw)"""
    dws = [g["pad_l"] - kw for kw in range(d["KW"])]
    flip_ok = g["pad_t"] == (d["KH"] - 1) // 2 if g["pad_t"] > 0 else d["KH"] == 1       # :1457,1461 (KH = 1 is refused anyway)
    return fewout_descent(1, 0, 1, d["C"], d["KH"], d["KW"], g["Hin"], g["Win"], g["OH"], g["OW"], d["N"], d["Cout"], d["ldy"],
                          d["Cout"], dws, (g["Ceff"] * d["Cout"]) % 4 == 0, flip_ok)


def rgbin_fwd(d):
    """launch_rgbin_fwd, conv.hip:1810-1845: None (refused), "rgbin_mfma_tpb1" / "_tpb2", or "rgbin_fwd" (W % 16 != 0)"""
    if not rgbin_shape(d):
        return None
    tiles = d["N"] * (d["H"] // (256 // d["W"]))
    if d["W"] % 16 == 0:
        return "rgbin_mfma_tpb2" if tiles % 2 == 0 and (tiles // 2) * (d["Cout"] // 64) >= 1024 else "rgbin_mfma_tpb1"
    return "rgbin_fwd"


def outer_kernel(d, g, p, wide_aligned):
    """the kernel of the few-channel weight gradient, conv.hip:3772-3825"""
    wide_is_x = p["outer"] == 1
    ldw, wideC, J = (d["ldx"], g["Ceff"], d["Cout"]) if wide_is_x else (d["ldy"], d["Cout"], d["C"])
    H, W, KH, KW = d["H"], d["W"], d["KH"], d["KW"]
    if (d["stride"] == 1 and KW in (3, 5) and KH <= 5 and g["pad_t"] <= 2 and g["pad_l"] <= 2 and KH - 1 - g["pad_t"] <= 2 and
            KW - 1 - g["pad_l"] <= 2 and H % outer_unit_rows(H) == 0 and ldw % 4 == 0 and wide_aligned and wideC % 4 == 0):
        if KH == KW and KW * J <= 16 and W % 4 == 0 and (outer_unit_rows(H) * W) % 16 == 0:
            return "mfma"
        return "outer2"
    return "plain"


# ------------------------------------------------------------------------------------------------------------------
# expected_route
# ------------------------------------------------------------------------------------------------------------------
def err(code, fragment):
    return (code, fragment)


def _al(case, *names):
    """every named operand pointer is 16-byte aligned (a NULL pointer counts as aligned: conv.hip:2638)"""
    for n in names:
        if n == "bias" and not case["bias"]:
            continue
        if n == "ws" and case["ws"] == "null":
            continue
        if case["off"][n] % 4:
            return False
    return True


def _ws_full(case):
    """workspace non-null and at least the size the query reports"""
    return case["ws"] == "full"


def expected_route(case, which, dense16=(False, 0), operand=None):
    """route name of one call, or (error code, fragment of the error text).  From the library: `dense16` = (ok, nsplit) of
    dense16_tiling (dense16_of) and `operand` = otgan_conv2d_operand_bytes(d) > 0 (default: wherever it can be)"""
    d = desc_fields(case)
    g = make_geo(d)
    if isinstance(g, str):
        return err(ERR_INVALID, g)
    case = dict(case, _operand=operand_bytes_possible(d, g) if operand is None else bool(operand))
    return (_fwd_route, _dgrad_route, _wgrad_route)[which](case, d, g, dense16)


def _fwd_route(case, d, g, dense16):
    """conv2d_fwd_body, conv.hip:3161-3366"""
    cmap = has_cmap(case)
    growth16 = (d["Cout"] == 16 and d["KH"] == 3 and d["KW"] == 3 and d["stride"] == 1 and d["upsample"] == 0 and d["C"] % 8 == 0 and
                d["ldx"] % 4 == 0 and _al(case, "x", "w"))                                                # :3169-3170
    s2_taken = (wino_s2_ok(d, g) and not cmap and _al(case, "x", "w", "y", "bias", "ws") and _ws_full(case))   # :3171-3173
    if case["y_acc"] and not (growth16 or (s2_taken and wino_plain3_ok(d, g))):                           # :3174
        return err(ERR_INVALID, "y_accumulate")
    if s2_taken:
        return "wino_plain3" if d["stride"] == 1 else "wino_s2"
    real_filters = case["filters"] in ("own", "unfolded")
    if real_filters and wino_up3_ok(d, g) and not wino_ok(d, g):                                          # :3201-3216
        if not (not cmap and _al(case, "x", "y", "bias", "ws") and _ws_full(case)):
            return err(ERR_INVALID, "winograd forward of a 3x3 upsampling layer")
        return "wino_up3"
    if not wino_ok(d, g) and case["x_operand"] and case["_operand"]:                          # :3217
        return err(ERR_INVALID, "x_operand given")
    if wino_ok(d, g):                                                                                     # :3220-3238
        if not _al(case, "x", "w", "y", "bias", "ws"):
            return err(ERR_INVALID, "winograd conv needs 16-byte aligned operands")
        if not _ws_full(case):
            return err(ERR_WORKSPACE, "conv2d fwd workspace too small")
        return "wino_fold5"
    if g["fold"]:                                                                                         # :3239-3274
        if not _al(case, "x", "w"):
            return err(ERR_INVALID, "folded conv needs 16-byte aligned operands")
        cls_taps = fold_taps(d, g)[2]
        rows = d["N"] * d["H"] * d["W"]
        if len(set(cls_taps)) == 1:
            return "fold4:" + igemm_cfg(True, True, g["Ceff"], rows, d["Cout"], False, 4, False, cmap)
        return "fold_percls:" + igemm_cfg(True, True, g["Ceff"], rows, d["Cout"], False, 1, False, cmap)
    Mtot = d["N"] * g["OH"] * g["OW"]
    if not cmap and d["preact"] == ACT_NONE:                                                              # :3279-3286
        r = rgbin_fwd(d)
        if r:
            return r
    if (d["Cout"] <= 4 and d["upsample"] == 0 and g["Ceff"] % 4 == 0 and d["ldx"] % 4 == 0 and _al(case, "x", "w") and
            fewout_quads_ok(d)):                                                                          # :3287-3310
        return "fewout_" + fewout_fwd(d, g)
    if growth16:                                                                                          # :3311-3331 (no amax record in
        return "dense16"                                                                                  # this table: never the h2 kernel)
    vec = map_quads(d) and g["Ceff"] % 16 == 0 and d["ldx"] % 4 == 0 and _al(case, "x", "w")              # :3334
    recs = vec and igemm_records_ok(case, d, FWD, 0, d["C"], d["ldx"], "x", d["KH"] * d["KW"] * g["Ceff"] * d["Cout"])
    ks = igemm_fwd_ksplit(d, g, vec, Mtot)
    if ks > 1 and _ws_full(case) and _al(case, "ws", "y", "bias"):                                        # :3346-3361
        return "igemm_ksplit:" + igemm_cfg(True, vec, g["Ceff"], Mtot, d["Cout"], False, ks, recs, cmap)
    return ("igemm_up:" if d["upsample"] else "igemm:") + igemm_cfg(True, vec, g["Ceff"], Mtot, d["Cout"], False, 1, recs, cmap)


def query_generic(case, d, g, which, dense16=(False, 0)):
    """the workspace the GPU test passes for a call on a non-Winograd descriptor (the library's query gives the size at test
    time; this is its generic part, enough to tell whether the scratch records fit)"""
    if which == 0:
        return generic_fwd_workspace(d, g)
    if which == 1:
        return generic_dgrad_workspace(d, g)
    return wgrad_workspace_generic(d, g, plan_wgrad(d, g, dense16))


def igemm_records_ok(case, d, which, used, a_C, a_ld, a_name, b_elems):
    """igemm_records, conv.hip:1784-1806, with no record given by the caller: both reductions need room in the workspace
    behind `used` bytes, a_C, a_ld and b_elems multiples of 4 and 16-byte aligned a, b (the workspace pointer itself may be
    misaligned: the records are read and written float by float)"""
    g = make_geo(d)
    if case["ws"] == "null":
        return False
    have = max(query_generic(case, d, g, which), 0) - (1 if case["ws"] == "short" else 0)
    if align_up(used, 256) + 2 * 4 * AMAX_RECORD_FLOATS > have:
        return False
    a_off = case["off"][a_name] + (d["y_coff"] if a_name == "dy" else 0)
    return a_C % 4 == 0 and a_ld % 4 == 0 and a_off % 4 == 0 and b_elems % 4 == 0 and case["off"]["w"] % 4 == 0


def _dgrad_route(case, d, g, dense16):
    """conv2d_dgrad_body, conv.hip:3404-3653"""
    inv = has_cmap(case)
    kind, paired = act_kind(d["preact"]), doubled(d["preact"])
    L = lddx(case)
    vec = d["Cout"] % 4 == 0 and d["ldy"] % 4 == 0 and d["y_coff"] % 4 == 0 and _al(case, "dy", "w")      # :3438-3439
    if d["C"] <= 4 and kind == 0 and d["stride"] == 1 and d["upsample"] == 0 and vec:                     # :3445-3470
        return "fewin_" + fewin_dgrad(d, g)
    if (d["Cout"] == 3 and d["stride"] == 1 and d["upsample"] == 0 and d["KH"] == d["KW"] and d["KH"] in (3, 5) and d["C"] % 4 == 0 and
            L % 4 == 0 and _al(case, "dx") and (kind == 0 or (_al(case, "x") and d["ldx"] % 4 == 0)) and (not inv or paired) and
            d["W"] % 16 == 0 and d["H"] % 4 == 0):                                                        # :3471-3495
        return "rgbout_dgrad"
    if (d["Cout"] == 16 and d["KH"] == 3 and d["KW"] == 3 and d["stride"] == 1 and d["upsample"] == 0 and d["ldy"] % 4 == 0 and
            d["y_coff"] % 4 == 0 and d["C"] % 4 == 0 and d["ldx"] % 4 == 0 and L % 4 == 0 and _al(case, "dy", "w", "x", "dx") and
            dense16[0]):                                                                                  # :3496-3508
        return "dense16"
    real_filters = case["filters"] in ("own", "unfolded")
    if real_filters and not wino_ok(d, g) and wino_up3_dgrad_ok(d, g):                                    # :3509-3522
        if not (not inv and L % 4 == 0 and _al(case, "dy", "dx", "x", "ws") and _ws_full(case)):
            return err(ERR_INVALID, "winograd dgrad of a 3x3 upsampling layer")
        return "wino_up3"
    if (wino_s2_ok(d, g) and not inv and L % 4 == 0 and _al(case, "dy", "w", "dx", "x", "ws") and _ws_full(case)):   # :3523-3531
        return "wino_plain3" if d["stride"] == 1 else "wino_s2"
    if wino_ok(d, g):                                                                                     # :3532-3546
        if not (_al(case, "dy", "w", "dx", "ws") and L % 4 == 0):
            return err(ERR_INVALID, "winograd dgrad needs 16-byte aligned operands")
        if not _ws_full(case):
            return err(ERR_WORKSPACE, "conv2d dgrad workspace too small")
        return "wino_fold5"
    epi = "pair" if paired else ("act" if kind else "plain")
    if g["fold"]:                                                                                         # :3547-3575: no records
        return "fold.%s:" % epi + igemm_cfg(False, vec, d["Cout"], d["N"] * d["H"] * d["W"], d["C"], paired, 1, False)
    used = 0
    if d["upsample"]:                                                                                     # :3579-3588
        if not _ws_full(case):
            return err(ERR_WORKSPACE, "conv2d dgrad workspace too small")
        used = 4 * d["N"] * g["Hin"] * g["Win"] * d["C"]
    st = d["stride"]
    rows = d["N"] * (g["Hin"] // st) * (g["Win"] // st)
    recs = vec and igemm_records_ok(case, d, DGRAD, used, d["Cout"], d["ldy"], "dy", d["KH"] * d["KW"] * g["Ceff"] * d["Cout"])
    return ("igemm_pool.%s:" if d["upsample"] else "igemm.%s:") % epi + igemm_cfg(False, vec, d["Cout"], rows, d["C"], paired,
                                                                                 st * st, recs)


def _wgrad_route(case, d, g, dense16):
    """otgan_conv2d_wgrad_f32, conv.hip:3655-3887"""
    cmap = has_cmap(case)
    p = plan_wgrad(d, g, dense16)
    if p["vec"] and not _al(case, "x", "dy"):                                                             # :3664
        return err(ERR_INVALID, "operands must be 16-byte aligned")
    if (p["nsplit"] > 1 or p["fold"] or p["outer"]) and not _ws_full(case):                               # :3666-3669
        return err(ERR_WORKSPACE, "conv2d wgrad workspace too small")
    wino_pre = not cmap and _al(case, "x", "dy", "dw", "ws") and _ws_full(case)
    if wino_up3_wgrad_ok(d, g) and wino_pre:                                                              # :3670-3678
        return "wino_up3"
    if wino_s2_ok(d, g) and wino_pre:                                                                     # :3679-3687
        return "wino_plain3" if d["stride"] == 1 else "wino_s2"
    if not wino_ok(d, g) and case["x_operand"] and case["_operand"]:                          # :3688
        return err(ERR_INVALID, "x_operand given")
    if wino_ok(d, g):                                                                                     # :3691-3725
        if not _al(case, "x", "dy", "dw", "ws"):
            return err(ERR_INVALID, "winograd wgrad needs 16-byte aligned operands")
        if not _ws_full(case):
            return err(ERR_WORKSPACE, "conv2d wgrad workspace too small")
        return "wino_fold5_fused" if g["pad_t"] == 2 and g["pad_l"] == 2 else "wino_fold5_unfold"        # :3709
    if p["dense16"]:                                                                                      # :3726-3747
        if not _al(case, "x", "dy"):
            return err(ERR_INVALID, "operands must be 16-byte aligned")
        return "dense16_slabs" if p["nsplit"] > 1 else "dense16"
    if p["outer"]:                                                                                        # :3750-3829
        wide = "x" if p["outer"] == 1 else "dy"
        wide_al = (case["off"][wide] + (d["y_coff"] if wide == "dy" else 0)) % 4 == 0
        return "outer%d_%s" % (p["outer"], outer_kernel(d, g, p, wide_al))
    fam = "igemm_fold:" if p["fold"] else ("igemm_up:" if d["upsample"] else "igemm:")
    if p["vec"]:                                                                                          # :3860-3870
        cfg = ("N16" if p["n16"] else ("Narrow" if p["narrow"] else ("W%d" % p["wide"] if p["wide"] else "Main"))) + "_vec"
    else:
        cfg = ("N16" if p["n16"] else ("Narrow" if p["narrow"] else "Main16")) + "_scalar"
    return fam + cfg + ("_split" if p["nsplit"] > 1 else "")


def is_error(route):
    return isinstance(route, tuple)


def is_wino(route):
    return isinstance(route, str) and route.startswith("wino_")


# ------------------------------------------------------------------------------------------------------------------
# executed FLOP as the three bodies report them to the profiler (ProfScope).  Routes that share a formula: every forward route
# that is neither Winograd nor folded reports 2 M Ktot Cout; every un-folded implicit-GEMM input gradient the sum over its
# parity classes; dense16, the outer kernels and the generic weight gradient 2 M slab_elems.  For those the predicates checked on
# the CPU are the evidence of the route; the FLOP figure separates Winograd / folded / generic.
# ------------------------------------------------------------------------------------------------------------------
def flops(case, which, route, dense16=(False, 0)):
    d = desc_fields(case)
    g = make_geo(d)
    N, H, W, C, Cout, Ceff = d["N"], d["H"], d["W"], d["C"], d["Cout"], g["Ceff"]
    taps = d["KH"] * d["KW"]
    if route == "wino_s2":                                            # 2 * kWinoS2Blocks * tiles * Ceff * Cout, :3195,3526,3683
        return 2.0 * 121 * N * (H // 2 // 4) * (W // 2 // 4) * Ceff * Cout
    if route == "wino_plain3":
        return 2.0 * 36 * N * (H // 4) * (W // 4) * Ceff * Cout
    if route == "wino_up3":                                           # :3211,3517,3674
        return 2.0 * 36 * N * (2 * H // 4) * (2 * W // 4) * Ceff * Cout
    if route.startswith("wino_fold5"):                                # :3234,3542,3705
        return 2.0 * 36 * N * (H // 4) * (W // 4) * 4.0 * Cout * C
    if which == FWD:
        if route.startswith("fold"):                                  # :3249
            return sum(2.0 * N * H * W * t * Ceff * Cout for t in fold_taps(d, g)[2])
        return 2.0 * N * g["OH"] * g["OW"] * taps * Ceff * Cout      # (the RGB-in scope opens only where rgbin_fwd_takes)
    if which == DGRAD:
        if route.startswith("fewin"):                                 # :3465
            return 2.0 * N * g["Hin"] * g["Win"] * taps * Cout * C
        if route in ("rgbout_dgrad", "dense16"):                      # :3485,3504
            return 2.0 * N * H * W * taps * Cout * Ceff
        if route.startswith("fold"):                                  # :3575
            return 2.0 * N * H * W * sum(fold_taps(d, g)[2]) * Cout * Ceff
        st = d["stride"]
        rows, total = N * (g["Hin"] // st) * (g["Win"] // st), 0.0
        for cls in range(st * st):                                    # :3598-3619
            ph, pw = cls // st, cls % st
            nt = sum(1 for kh in range(d["KH"]) if (ph + g["pad_t"] - kh) % st == 0) * \
                sum(1 for kw in range(d["KW"]) if (pw + g["pad_l"] - kw) % st == 0)
            total += 2.0 * rows * nt * Cout * Ceff
        return total
    p = plan_wgrad(d, g, dense16)
    return 2.0 * p["M"] * p["slab_elems"]                             # :3734,3796,3807,3820,3859


# ------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------
INV, WSP = ERR_INVALID, ERR_WORKSPACE

# ---- Winograd bases (aligned, map-free, y_coff / ldy / lddx > 0 and accumulate on every one: branches 9 and 10)
S2 = _c("s2", 2, 8, 8, (32,), 24, 5, stride=2, ypad=4, y_coff=4, dxpad=4, acc=1, filters="own",
        expect={0: "wino_s2", 1: "wino_s2", 2: "wino_s2"})
S2_CRELU = _c("s2_crelu_xop", 32, 8, 8, (16,), 48, 5, stride=2, pre=ACT_CRELU, x_operand=True,
              expect={0: "wino_s2", 1: "wino_s2", 2: "wino_s2"})
PLAIN3 = _c("plain3", 1, 8, 8, (64,), 128, 3, ypad=8, y_coff=8, dxpad=4, acc=1, y_acc=1,
            expect={0: "wino_plain3", 1: "wino_plain3", 2: "wino_plain3"})
UP3 = _c("up3", 8, 4, 4, (16,), 16, 3, up=1, pre=ACT_CRELU, filters="unfolded", ypad=4, y_coff=4, dxpad=4, acc=1,
         expect={0: "wino_up3", 1: "wino_up3", 2: "wino_up3"})
FOLD5 = _c("fold5", 2, 4, 4, (32,), 8, 5, up=1, ypad=4, y_coff=4, dxpad=4, acc=1, filters="own",
           expect={0: "wino_fold5", 1: "wino_fold5", 2: "wino_fold5_fused"})

FOLD3 = _c("fold_3x3_relu", 2, 4, 4, (32,), 12, 3, up=1, pre=ACT_RELU, dxpad=4, acc=1,
           expect={0: "fold4:N16_vec", 1: "fold.act:Narrow_scalar", 2: "igemm_fold:N16_vec"})
GROWTH_RELU = _c("growth16_relu", 2, 8, 8, (16,), 16, 3, pre=ACT_RELU, expect={0: "dense16", 1: "dense16", 2: "dense16_slabs"})

S2_FB = {0: "igemm:Narrow_vec", 1: "igemm.plain:Narrow_scalar", 2: "igemm:Narrow_vec"}
PLAIN3_FB = {0: "igemm:Small16_x2h", 1: "igemm.plain:Small16_x2h", 2: "igemm:Main_vec"}

CASES = [
    # ---- 5. the strided 5x5 Winograd passes and each way out of them, one condition at a time
    S2, S2_CRELU,
    variant(S2, "s2_cmap", S2_FB, cmap="identity"),
    variant(S2, "s2_x_off", {0: "igemm:Narrow_scalar", 1: "igemm.plain:Narrow_scalar", 2: (INV, "operands must be 16-byte aligned")}, off={"x": 1}),
    variant(S2, "s2_w_off", {0: "igemm:Narrow_scalar", 1: "igemm.plain:Narrow_scalar"}, off={"w": 1}, passes=(0, 1)),
    variant(S2, "s2_y_off", {0: S2_FB[0]}, off={"y": 1}, passes=(0,)),
    variant(S2, "s2_bias_off", {0: S2_FB[0]}, off={"bias": 2}, passes=(0,)),
    variant(S2, "s2_dy_off", {1: "igemm.plain:Narrow_scalar", 2: (INV, "operands must be 16-byte aligned")}, off={"dy": 1}, passes=(1, 2)),
    variant(S2, "s2_dx_off", {1: S2_FB[1]}, off={"dx": 3}, passes=(1,)),
    variant(S2, "s2_dw_off", {2: S2_FB[2]}, off={"dw": 1}, passes=(2,)),
    variant(S2, "s2_ws_off", S2_FB, off={"ws": 1}),
    variant(S2, "s2_ws_null", S2_FB, ws="null"),
    variant(S2, "s2_ws_short", S2_FB, ws="short"),
    variant(S2, "s2_lddx", {1: S2_FB[1]}, dxpad=2, passes=(1,)),
    variant(S2_CRELU, "s2_xop_x_off", {0: (INV, "x_operand given"), 2: (INV, "operands must be 16-byte aligned")}, off={"x": 2}, passes=(0, 2)),
    variant(S2_CRELU, "s2_xop_cmap", {0: (INV, "x_operand given"), 2: (INV, "x_operand given")}, cmap="identity", passes=(0, 2)),
    # ---- the wide 3x3 stride-1 passes (y_accumulate only on the Winograd route)
    PLAIN3,
    variant(PLAIN3, "plain3_cmap", PLAIN3_FB, cmap="identity", y_acc=0),
    variant(PLAIN3, "plain3_yacc_fallback", {0: (INV, "y_accumulate")}, off={"y": 1}, passes=(0,)),
    variant(PLAIN3, "plain3_ws_short", {0: (INV, "y_accumulate"), 1: PLAIN3_FB[1], 2: PLAIN3_FB[2]}, ws="short"),
    variant(PLAIN3, "plain3_x_off", {0: "igemm:Main16_scalar", 1: PLAIN3_FB[1]}, off={"x": 1}, y_acc=0, passes=(0, 1)),
    # ---- 3x3 on an upsampled CReLU input: Winograd exactly when `filters` is given, rejected (never rerouted) otherwise
    UP3,
    variant(UP3, "up3_nofilters", {0: "fold4:N16_vec", 1: "fold.pair:Small16_x3s", 2: "wino_up3"}, filters=None),
    variant(UP3, "up3_x_off", {0: (INV, "winograd forward of a 3x3 upsampling layer"), 1: (INV, "winograd dgrad of a 3x3 upsampling layer"), 2: (INV, "operands must be 16-byte aligned")},
            off={"x": 1}),
    variant(UP3, "up3_y_off", {0: (INV, "winograd forward of a 3x3 upsampling layer")}, off={"y": 1}, passes=(0,)),
    variant(UP3, "up3_ws_short", {0: (INV, "winograd forward of a 3x3 upsampling layer"), 1: (INV, "winograd dgrad of a 3x3 upsampling layer"),
                                  2: (WSP, "conv2d wgrad workspace too small")}, ws="short"),
    variant(UP3, "up3_lddx", {1: (INV, "winograd dgrad of a 3x3 upsampling layer")}, dxpad=2, passes=(1,)),
    variant(UP3, "up3_dw_off", {2: "igemm_fold:N16_vec"}, off={"dw": 1}, passes=(2,)),
    variant(UP3, "up3_n2_wgrad", {2: "igemm_fold:N16_vec"}, N=2, passes=(2,)),
    # ---- the folded 5x5 passes: reject, never reroute
    FOLD5,
    variant(FOLD5, "fold5_unfolded_filters", FOLD5["expect"], filters="unfolded", passes=(0, 1)),
    variant(FOLD5, "fold5_nofilters", FOLD5["expect"], filters=None, passes=(0, 1)),
    variant(FOLD5, "fold5_x_off", {0: (INV, "winograd conv needs 16-byte aligned operands"), 2: (INV, "operands must be 16-byte aligned")}, off={"x": 1}, passes=(0, 2)),
    variant(FOLD5, "fold5_bias_off", {0: (INV, "winograd conv needs 16-byte aligned operands")}, off={"bias": 1}, passes=(0,)),
    variant(FOLD5, "fold5_dx_off", {1: (INV, "winograd dgrad needs 16-byte aligned operands")}, off={"dx": 1}, passes=(1,)),
    variant(FOLD5, "fold5_lddx", {1: (INV, "winograd dgrad needs 16-byte aligned operands")}, dxpad=1, passes=(1,)),
    variant(FOLD5, "fold5_dw_off", {2: (INV, "winograd wgrad needs 16-byte aligned operands")}, off={"dw": 1}, passes=(2,)),
    variant(FOLD5, "fold5_ws_short", {0: (WSP, "conv2d fwd workspace too small"), 1: (WSP, "conv2d dgrad workspace too small"),
                                      2: (WSP, "conv2d wgrad workspace too small")}, ws="short"),
    variant(FOLD5, "fold5_ws_null", {0: (WSP, "conv2d fwd workspace too small"), 1: (WSP, "conv2d dgrad workspace too small"),
                                     2: (WSP, "conv2d wgrad workspace too small")}, ws="null"),
    # ---- 5. continued: the remaining conditions on the wide 3x3, the 3x3-upsampling (with `filters`) and the folded 5x5 passes
    variant(PLAIN3, "plain3_w_off", {0: "igemm:Main16_scalar", 1: "igemm.plain:Main16_scalar"}, off={"w": 1}, y_acc=0, passes=(0, 1)),
    variant(PLAIN3, "plain3_bias_off", {0: PLAIN3_FB[0]}, off={"bias": 1}, y_acc=0, passes=(0,)),
    variant(PLAIN3, "plain3_dy_off", {1: "igemm.plain:Main16_scalar", 2: (INV, "operands must be 16-byte aligned")}, off={"dy": 2}, passes=(1, 2)),
    variant(PLAIN3, "plain3_dx_off", {1: PLAIN3_FB[1]}, off={"dx": 1}, y_acc=0, passes=(1,)),
    variant(PLAIN3, "plain3_dw_off", {2: PLAIN3_FB[2]}, off={"dw": 3}, y_acc=0, passes=(2,)),
    variant(PLAIN3, "plain3_ws_off", PLAIN3_FB, off={"ws": 1}, y_acc=0),
    variant(PLAIN3, "plain3_ws_null", {**PLAIN3_FB, 0: "igemm:Small16_x3s", 1: "igemm.plain:Small16_x3s"}, ws="null", y_acc=0),
    variant(PLAIN3, "plain3_lddx", {1: PLAIN3_FB[1]}, dxpad=2, y_acc=0, passes=(1,)),
    variant(UP3, "up3_cmap", {0: (INV, "winograd forward of a 3x3 upsampling layer"), 1: (INV, "winograd dgrad of a 3x3 upsampling layer"),
                              2: "igemm_fold:N16_vec"}, cmap="identity"),
    variant(UP3, "up3_bias_off", {0: (INV, "winograd forward of a 3x3 upsampling layer")}, off={"bias": 1}, passes=(0,)),
    variant(UP3, "up3_dy_off", {1: (INV, "winograd dgrad of a 3x3 upsampling layer"), 2: (INV, "operands must be 16-byte aligned")},
            off={"dy": 1}, passes=(1, 2)),
    variant(UP3, "up3_dx_off", {1: (INV, "winograd dgrad of a 3x3 upsampling layer")}, off={"dx": 1}, passes=(1,)),
    variant(UP3, "up3_ws_off", {0: (INV, "winograd forward of a 3x3 upsampling layer"), 1: (INV, "winograd dgrad of a 3x3 upsampling layer"),
                                2: "igemm_fold:N16_vec"}, off={"ws": 1}),
    variant(UP3, "up3_ws_null", {0: (INV, "winograd forward of a 3x3 upsampling layer"), 1: (INV, "winograd dgrad of a 3x3 upsampling layer"),
                                 2: (WSP, "conv2d wgrad workspace too small")}, ws="null"),
    variant(UP3, "up3_w_off", {0: "wino_up3", 1: "wino_up3"}, off={"w": 1}, passes=(0, 1)),
    # (the folded 5x5 passes take a channel map and never look at it: no pre-activation, the map is the identity)
    variant(FOLD5, "fold5_cmap", FOLD5["expect"], cmap="identity"),
    variant(FOLD5, "fold5_w_off", {0: (INV, "winograd conv needs 16-byte aligned operands"), 1: (INV, "winograd dgrad needs 16-byte aligned operands")},
            off={"w": 1}, passes=(0, 1)),
    variant(FOLD5, "fold5_y_off", {0: (INV, "winograd conv needs 16-byte aligned operands")}, off={"y": 1}, passes=(0,)),
    variant(FOLD5, "fold5_dy_off", {1: (INV, "winograd dgrad needs 16-byte aligned operands"), 2: (INV, "operands must be 16-byte aligned")},
            off={"dy": 1}, passes=(1, 2)),
    variant(FOLD5, "fold5_ws_off", {0: (INV, "winograd conv needs 16-byte aligned operands"), 1: (INV, "winograd dgrad needs 16-byte aligned operands"),
                                    2: (INV, "winograd wgrad needs 16-byte aligned operands")}, off={"ws": 1}),
    # ---- 1. un-folded upsampling: the gather through logUp, the virtual-grid gradient and pool2_sum_kernel
    _c("up_unfold_c6", 2, 4, 4, (6,), 8, 3, up=1, pre=ACT_CRELU, xpad=2, dxpad=3, acc=1, ypad=3, y_coff=1,
       expect={0: "igemm_up:N16_scalar", 1: "igemm_pool.pair:Main16_scalar", 2: "igemm_up:N16_scalar"}),
    _c("up_unfold_pitch", 2, 4, 8, (16,), 40, 5, up=1, xpad=2, dxpad=1, acc=1,
       expect={0: "igemm_up:Main16_scalar", 1: "igemm_pool.plain:N16_scalar", 2: "igemm_up:Main16_scalar"}),
    _c("up_unfold_1x1", 1, 8, 4, (32,), 48, 1, up=1, pre=ACT_ELU, acc=1,
       expect={0: "igemm_up:Small16_x2h", 1: "igemm_pool.act:Narrow_vec", 2: "igemm_up:Main_vec"}),
    _c("up_unfold_5x1", 2, 4, 4, (16,), 36, (5, 1), up=1, pre=ACT_RELU,
       expect={0: "igemm_up:Small16_x2h", 1: "igemm_pool.act:N16_scalar", 2: "igemm_up:Main16_scalar"}),
    variant(_c("up_unfold_ws", 2, 4, 4, (6,), 8, 3, up=1, pre=ACT_CRELU), "up_unfold_ws_short",
            {1: (WSP, "conv2d dgrad workspace too small")}, ws="short", passes=(1,)),
    # ---- 2. folded layers with even / non-square filters: per-class forward launches, folded dgrad, folded wgrad, un-fold
    _c("fold_2x2", 2, 4, 4, (16,), 8, 2, up=1, dxpad=4, acc=1,
       expect={0: "fold_percls:N16_vec", 1: "fold.plain:N16_scalar", 2: "igemm_up:N16_scalar"}),
    _c("fold_2x3_crelu", 2, 4, 4, (16,), 36, (2, 3), up=1, pre=ACT_CRELU, ypad=4, y_coff=8,
       expect={0: "fold_percls:Small16_x3s", 1: "fold.pair:Small16_x3s", 2: "igemm_fold:Main_vec"}),
    _c("fold_4x4_celu", 1, 4, 4, (8, 8), 20, 4, up=1, pre=ACT_CELU,
       expect={0: "fold_percls:Narrow_vec", 1: "fold.pair:Small16_x3s", 2: "igemm_fold:Narrow_vec"}),
    _c("fold_3x2_split", 2, 16, 16, (32,), 8, (3, 2), up=1, passes=(0, 2),
       expect={0: "fold_percls:N16_vec", 2: "igemm_fold:N16_vec_split"}),
    FOLD3,
    variant(FOLD3, "fold_3x3_relu_dy_off", {1: "fold.act:Narrow_scalar", 2: (INV, "operands must be 16-byte aligned")}, off={"dy": 1},
            passes=(1, 2)),
    variant(_c("fold_x", 2, 4, 4, (16,), 8, 2, up=1), "fold_x_off", {0: (INV, "folded conv needs 16-byte aligned operands")}, off={"x": 1}, passes=(0,)),
    # ---- 3. / 4. implicit GEMM with misaligned x / y / bias and odd pitches; the K split and its ways out
    _c("igemm_y_bias_off", 2, 8, 8, (16,), 40, 3, off={"y": 1, "bias": 3}, ypad=3, y_coff=2, passes=(0,),
       expect={0: "igemm:Small16_x2h"}),
    _c("filters_ignored", 2, 8, 8, (16,), 40, 3, filters="dummy", passes=(0, 1), expect={0: "igemm:Small16_x2h", 1: "igemm.plain:N16_scalar"}),
    _c("dg_act_ldx", 2, 8, 8, (12,), 24, 3, pre=ACT_RELU, xpad=1, off={"x": 1, "dx": 1}, dxpad=1, acc=1,
       expect={0: "igemm:Narrow_scalar", 1: "igemm.act:N16_scalar", 2: "igemm:Narrow_scalar"}),
    _c("dg_pair_c40", 2, 8, 8, (40,), 24, 3, pre=ACT_CRELU, xpad=3, off={"x": 3}, dxpad=2, acc=1,
       expect={0: "igemm:Narrow_scalar", 1: "igemm.pair:Small16_x2h", 2: "igemm:Narrow_scalar"}),
    _c("list_widths_odd", 2, 8, 8, (3, 5, 8), 40, 3, pre=ACT_CELU, stride=2,
       expect={0: "igemm:Main16_scalar", 1: "igemm.pair:Small16_x2h", 2: "igemm:Main16_scalar"}),
    _c("ksplit2", 1, 8, 8, (128,), 48, 3, pre=ACT_CRELU, ypad=4, y_coff=4, passes=(0,), expect={0: "igemm_ksplit:Small16_x2h"}),
    variant(_c("ksplit2", 1, 8, 8, (128,), 48, 3, pre=ACT_CRELU, passes=(0,)), "ksplit_y_off", {0: "igemm:Small16_x2h"}, off={"y": 1}),
    variant(_c("ksplit2", 1, 8, 8, (128,), 48, 3, pre=ACT_CRELU, passes=(0,)), "ksplit_bias_off", {0: "igemm:Small16_x2h"},
            off={"bias": 1}),
    variant(_c("ksplit2", 1, 8, 8, (128,), 48, 3, pre=ACT_CRELU, passes=(0,)), "ksplit_ws_short", {0: "igemm:Small16_x2h"}, ws="short"),
    variant(_c("ksplit2", 1, 8, 8, (128,), 48, 3, pre=ACT_CRELU, passes=(0,)), "ksplit_ws_null", {0: "igemm:Small16_x3s"}, ws="null"),
    variant(_c("ksplit2", 1, 8, 8, (128,), 48, 3, pre=ACT_CRELU, passes=(0,)), "ksplit_ldy", {0: "igemm:Small16_x2h"}, ypad=2),
    # ---- 6. the few-channel kernels off the models' shapes
    _c("rgbin_w16", 2, 16, 16, (3,), 128, 5, xpad=1, ypad=4, y_coff=4, dxpad=1, acc=1,
       expect={0: "rgbin_mfma_tpb1", 1: "fewin_mfma", 2: "outer2_mfma"}),
    _c("rgbin_w64_k3", 1, 4, 64, (3,), 128, 3, off={"x": 1, "y": 1, "bias": 1},
       expect={0: "rgbin_mfma_tpb1", 1: "fewin_tile", 2: "outer2_mfma"}),
    _c("rgbin_tpb2", 64, 64, 64, (3,), 128, 3, passes=(0,), expect={0: "rgbin_mfma_tpb2"}),
    _c("rgbin_w8", 2, 8, 8, (3,), 128, 5, expect={0: "igemm:Main16_scalar", 1: "fewin_plain", 2: "outer2_mfma"}),
    _c("rgbin_w128", 1, 8, 128, (3,), 128, 3, passes=(0, 1), expect={0: "igemm:Main16_scalar", 1: "fewin_plain"}),
    _c("fewin_c1", 2, 16, 16, (1,), 64, 3, expect={0: "igemm:Main16_scalar", 1: "fewin_mfma", 2: "outer2_mfma"}),
    _c("fewin_c2_k5", 2, 16, 16, (2,), 36, 5, dxpad=2, acc=1, expect={0: "igemm:Main16_scalar", 1: "fewin_plain", 2: "outer2_mfma"}),
    _c("fewin_c4_tile", 2, 16, 16, (4,), 40, 3, off={"dx": 1}, dxpad=3, acc=1, expect={0: "igemm:Main16_scalar", 1: "fewin_tile", 2: "outer2_mfma"}),
    _c("fewin_c4_k5", 2, 16, 16, (4,), 36, 5, expect={0: "igemm:Main16_scalar", 1: "fewin_tile", 2: "outer2_outer2"}),
    _c("fewin_c4_s2", 2, 16, 16, (4,), 40, 3, stride=2, expect={0: "igemm:Main16_scalar", 1: "igemm.plain:N16_scalar", 2: "outer2_plain"}),
    _c("fewin_dy_off", 2, 16, 16, (3,), 40, 3, off={"dy": 1}, passes=(1, 2), expect={1: "igemm.plain:N16_scalar", 2: "outer2_plain"}),
    _c("rgbout_w16", 2, 16, 16, (64,), 3, 5, ypad=4, y_coff=1, dxpad=4, acc=1,
       expect={0: "fewout_mfma", 1: "rgbout_dgrad", 2: "outer1_mfma"}),
    _c("rgbout_crelu_list", 2, 16, 16, (16, 16), 3, 3, pre=ACT_CRELU, expect={0: "fewout_mfma", 1: "rgbout_dgrad", 2: "outer1_mfma"}),
    _c("rgbout_c32_tile", 2, 16, 16, (32,), 3, 5, pre=ACT_ELU, ypad=2, y_coff=3, expect={0: "fewout_tile", 1: "rgbout_dgrad", 2: "outer1_mfma"}),
    _c("rgbout_w8", 4, 8, 8, (64,), 3, 3, ypad=1, y_coff=2, expect={0: "fewout_plain", 1: "igemm.plain:Main16_scalar",
                                                  2: "outer1_mfma"}),
    _c("rgbout_w128", 1, 4, 128, (16,), 3, 3, pre=ACT_RELU, expect={0: "fewout_plain", 1: "rgbout_dgrad", 2: "outer1_mfma"}),
    # H < TR = 256 / W: launch_rgbin_fwd and launch_fewout_tile refuse
    _c("rgbin_h8_w16", 2, 8, 16, (3,), 128, 3, expect={0: "igemm:Main16_scalar", 1: "fewin_mfma", 2: "outer2_mfma"}),
    _c("rgbout_h4_w32", 4, 4, 32, (32,), 3, 3, ypad=1, expect={0: "fewout_plain", 1: "rgbout_dgrad", 2: "outer1_mfma"}),
    _c("fewin_h2_w64", 2, 2, 64, (4,), 24, 3, dxpad=4, acc=1, expect={0: "igemm:Narrow_scalar", 1: "fewin_plain", 2: "outer2_mfma"}),
    # a wide operand of 6 channels: the last quad of a row is ragged (conv_outer_kernel, load_quad)
    _c("outer1_widec6", 2, 8, 8, (6,), 3, 3, pre=ACT_RELU, expect={0: "igemm:N16_scalar", 1: "igemm.act:N16_scalar", 2: "outer1_plain"}),
    _c("outer2_cout6", 2, 8, 8, (3,), 6, 3, expect={0: "igemm:N16_scalar", 1: "igemm.plain:N16_scalar", 2: "outer2_plain"}),
    _c("cout1", 2, 16, 16, (64,), 1, 5, expect={0: "fewout_mfma", 1: "igemm.plain:Main16_scalar", 2: "outer1_mfma"}),
    _c("cout2_tile_refused", 2, 16, 16, (32,), 2, 3, expect={0: "fewout_plain", 1: "igemm.plain:Narrow_scalar", 2: "outer1_mfma"}),
    _c("cout4_k5", 2, 16, 16, (32,), 4, 5, pre=ACT_CRELU, ypad=4, expect={0: "fewout_tile", 1: "igemm.pair:Small16_x2h", 2: "outer1_outer2"}),
    _c("cout4_s2", 2, 16, 16, (32,), 4, 3, stride=2, expect={0: "fewout_plain", 1: "igemm.plain:Narrow_scalar",
                                                              2: "outer1_plain"}),
    _c("cout3_x_off", 2, 16, 16, (32,), 3, 3, off={"x": 1}, passes=(0, 2), expect={0: "igemm:N16_scalar", 2: "outer1_plain"}),
    _c("cout3_2x2", 2, 8, 8, (16,), 3, 2, expect={0: "fewout_plain", 1: "igemm.plain:N16_scalar", 2: "outer1_plain"}),
    # CReLU over 6 channels: an aligned quad of effective channels straddles +x / -x -- not for the quad-wise few-output kernels
    _c("cout3_crelu_c6", 2, 8, 8, (6,), 3, 3, pre=ACT_CRELU, xpad=2,
       expect={0: "igemm:N16_scalar", 1: "igemm.pair:Main16_scalar", 2: "igemm:N16_scalar"}),
    _c("cout3_crelu_list_2_2", 2, 8, 8, (2, 2), 3, 3, pre=ACT_CRELU,
       expect={0: "igemm:N16_scalar", 1: "igemm.pair:Main16_scalar", 2: "igemm:N16_scalar"}),
    # the smallest few-channel weight gradient: one chunk, its slab in the workspace all the same
    _c("outer_one_chunk", 1, 8, 8, (16,), 3, 3, passes=(2,), expect={2: "outer1_mfma"}),
    variant(_c("outer_one_chunk", 1, 8, 8, (16,), 3, 3, passes=(2,)), "outer_one_chunk_ws_null", {2: (WSP, "conv2d wgrad workspace too small")},
            ws="null"),
    # ---- growth layers (16 outputs, 3x3): the streaming kernels of dense16.hip and the ways out of them
    _c("growth16", 4, 16, 16, (16, 16), 16, 3, pre=ACT_CRELU, ypad=16, y_coff=32, dxpad=16, acc=1, y_acc=1,
       expect={0: "dense16", 1: "dense16", 2: "dense16_slabs"}),
    _c("growth16_one_tile", 1, 8, 8, (16,), 16, 3, pre=ACT_CRELU, expect={0: "dense16", 1: "dense16", 2: "dense16"}),
    _c("growth16_c12", 2, 8, 8, (12,), 16, 3, pre=ACT_CRELU, expect={0: "igemm:N16_scalar", 1: "dense16", 2: "dense16_slabs"}),
    GROWTH_RELU,
    variant(GROWTH_RELU, "growth16_x_off", {0: "igemm:N16_scalar", 1: "igemm.act:N16_vec", 2: (INV, "operands must be 16-byte aligned")},
            off={"x": 1}),
    # ---- 7. launch_igemm thresholds (the smallest shapes that cross them)
    _c("tiles128_512", 64, 32, 32, (16,), 64, 1, passes=(0, 1), expect={0: "igemm:Main16_x2h", 1: "igemm.plain:N16_vec"}),
    _c("tiles128_511", 32, 32, 32, (16,), 64, 1, passes=(0,), expect={0: "igemm:Small16_x2h"}),
    _c("w160_256", 32, 32, 32, (32,), 144, 1, passes=(0,), expect={0: "igemm:W160_x2h"}),
    _c("w160_128", 16, 32, 32, (32,), 144, 1, passes=(0,), expect={0: "igemm:Small16_x2h"}),
    _c("w224_256", 32, 32, 32, (16,), 200, 1, pre=ACT_RELU, passes=(0,), expect={0: "igemm:W224_x2h"}),
    _c("w224_ck48", 32, 32, 32, (48,), 196, 1, cmap="identity", passes=(0,), expect={0: "igemm:W224_x2h"}),
    _c("w160_ck16", 32, 32, 32, (16,), 144, 1, passes=(0,), expect={0: "igemm:Main16_x2h"}),
    variant(_c("tiles128_512", 64, 32, 32, (16,), 64, 1, passes=(0,)), "tiles128_512_ws_null", {0: "igemm:Main16_x3s"}, ws="null"),
    variant(_c("w160_256", 32, 32, 32, (32,), 144, 1, passes=(0,)), "w160_256_ws_null", {0: "igemm:W160_x3s"}, ws="null"),
    variant(_c("w224_256", 32, 32, 32, (16,), 200, 1, pre=ACT_RELU, passes=(0,)), "w224_256_ws_null", {0: "igemm:W224_x3s"}, ws="null"),
    _c("dg_tiles128_512", 64, 32, 32, (64,), 16, 1, passes=(1,), dxpad=4, acc=1, expect={1: "igemm.plain:Main16_x2h"}),
    variant(_c("dg_tiles128_512", 64, 32, 32, (64,), 16, 1, passes=(1,)), "dg_tiles128_512_ws_null", {1: "igemm.plain:Main16_x3s"}, ws="null"),
    _c("ksplit_w224", 16, 16, 16, (512,), 200, 1, pre=ACT_CRELU, passes=(0,), expect={0: "igemm_ksplit:W224_x2h"}),
    _c("ksplit_main16", 32, 16, 16, (512,), 64, 1, pre=ACT_CRELU, passes=(0,), expect={0: "igemm_ksplit:Main16_x2h"}),
    _c("narrow_cout20", 2, 8, 8, (8,), 20, 3, pre=ACT_CRELU, expect={0: "igemm:Narrow_vec", 1: "igemm.pair:Small16_x2h",
                                                                      2: "igemm:Narrow_scalar"}),
    # ---- 8. plan_wgrad classes, one split and several
    _c("wg_n16", 1, 16, 16, (32,), 12, 3, passes=(2,), expect={2: "igemm:N16_vec"}),
    _c("wg_n16_split", 2, 16, 16, (32,), 12, 3, passes=(2,), expect={2: "igemm:N16_vec_split"}),
    _c("wg_narrow_split", 2, 16, 16, (16,), 32, 3, pre=ACT_CRELU, passes=(2,), expect={2: "igemm:Narrow_vec_split"}),
    _c("wg_main", 2, 16, 16, (32,), 64, 3, passes=(2,), expect={2: "igemm:Main_vec"}),
    _c("wg_main_split", 4, 16, 16, (32,), 64, 3, passes=(2,), expect={2: "igemm:Main_vec_split"}),
    _c("wg_w160", 2, 16, 16, (32,), 132, 1, passes=(2,), expect={2: "igemm:W160_vec"}),
    _c("wg_w160_split", 4, 16, 16, (32,), 160, 3, passes=(2,), expect={2: "igemm:W160_vec_split"}),
    _c("wg_w224", 1, 16, 16, (32,), 196, 1, passes=(2,), expect={2: "igemm:W224_vec"}),
    _c("wg_w224_split", 2, 16, 16, (32,), 224, 3, passes=(2,), expect={2: "igemm:W224_vec_split"}),
    _c("wg_main16_scalar", 2, 16, 16, (6,), 40, 3, pre=ACT_CELU, stride=2, xpad=1, passes=(2,), expect={2: "igemm:Main16_scalar"}),
    _c("wg_n16_scalar_split", 4, 16, 16, (64,), 12, 5, xpad=1, passes=(2,), expect={2: "igemm:N16_scalar_split"}),
    _c("wg_narrow_scalar_split", 4, 16, 16, (64,), 24, 5, xpad=1, passes=(2,), expect={2: "igemm:Narrow_scalar_split"}),
    _c("wg_main16_split", 2, 16, 16, (64,), 40, 3, xpad=1, passes=(2,), expect={2: "igemm:Main16_scalar_split"}),
    _c("wg_fold_main_split", 4, 16, 16, (32,), 64, 2, up=1, passes=(2,), expect={2: "igemm_fold:Main_vec_split"}),
    # ---- every remaining (family, tile configuration) pair the three passes can reach: the cheapest call of the CPU test's grid
    # on each (the shapes above 4 x 16 x 16 pixels are the ones whose configuration sits behind a tile-count threshold)
    _c("p0_fold4_main16_x3s", 64, 4, 64, (32,), 192, 3, up=1, pre=4, xpad=4, passes=(0,), expect={0: "fold4:Main16_x3s"}),
    _c("p0_fold4_narrow_vec", 8, 2, 2, (128,), 20, 3, up=1, pre=4, xpad=4, passes=(0,), expect={0: "fold4:Narrow_vec"}),
    _c("p0_fold4_small16_x3s", 2, 2, 2, (48,), 128, (3, 5), up=1, pre=1, xpad=4, ypad=4, passes=(0,), expect={0: "fold4:Small16_x3s"}),
    _c("p0_fold_percls_main16_x3s", 64, 32, 32, (48,), 36, 2, up=1, pre=4, passes=(0,), expect={0: "fold_percls:Main16_x3s"}),
    _c("p0_igemm_n16_vec", 1, 2, 2, (32,), 8, 3, pre=4, xpad=4, passes=(0,), expect={0: "igemm:N16_vec"}),
    _c("p0_igemm_ksplit_w160_x2h", 16, 16, 16, (512,), 144, 1, pre=1, passes=(0,), expect={0: "igemm_ksplit:W160_x2h"}),
    _c("p0_igemm_up_main16_x2h", 64, 16, 8, (48,), 132, 1, up=1, ypad=4, y_coff=4, passes=(0,), expect={0: "igemm_up:Main16_x2h"}),
    _c("p0_igemm_up_main16_x3s", 64, 16, 8, (48,), 132, 1, up=1, ypad=4, y_coff=4, ws='null', passes=(0,), expect={0: "igemm_up:Main16_x3s"}),
    _c("p0_igemm_up_n16_vec", 2, 2, 2, (32,), 2, 3, up=1, pre=2, y_coff=4, passes=(0,), expect={0: "igemm_up:N16_vec"}),
    _c("p0_igemm_up_narrow_scalar", 2, 4, 4, (8,), 20, 1, up=1, y_coff=4, passes=(0,), expect={0: "igemm_up:Narrow_scalar"}),
    _c("p0_igemm_up_narrow_vec", 1, 2, 2, (48,), 20, (2, 3), stride=2, up=1, pre=3, passes=(0,), expect={0: "igemm_up:Narrow_vec"}),
    _c("p0_igemm_up_small16_x3s", 1, 8, 4, (32,), 48, 1, up=1, pre=3, ws='null', passes=(0,), expect={0: "igemm_up:Small16_x3s"}),
    _c("p0_igemm_up_w160_x2h", 16, 8, 128, (32,), 160, 1, up=1, pre=3, y_coff=4, passes=(0,), expect={0: "igemm_up:W160_x2h"}),
    _c("p0_igemm_up_w160_x3s", 16, 8, 128, (32,), 160, 1, up=1, pre=3, y_coff=4, ws='null', passes=(0,), expect={0: "igemm_up:W160_x3s"}),
    _c("p1_fold_act_main16_scalar", 1, 2, 2, (48,), 40, (2, 3), up=1, pre=3, y_coff=16, filters='unfolded', off={'w': 1}, passes=(1,), expect={1: "fold.act:Main16_scalar"}),
    _c("p1_fold_act_main16_x3s", 64, 32, 32, (48,), 36, 2, up=1, pre=4, passes=(1,), expect={1: "fold.act:Main16_x3s"}),
    _c("p1_fold_act_n16_scalar", 2, 8, 4, (16,), 20, 4, up=1, pre=3, xpad=4, ypad=16, y_coff=4, passes=(1,), expect={1: "fold.act:N16_scalar"}),
    _c("p1_fold_act_narrow_vec", 8, 2, 2, (32,), 160, 5, up=1, pre=3, xpad=4, y_coff=4, passes=(1,), expect={1: "fold.act:Narrow_vec"}),
    _c("p1_fold_act_small16_x3s", 1, 2, 2, (48,), 40, (2, 3), up=1, pre=3, y_coff=16, passes=(1,), expect={1: "fold.act:Small16_x3s"}),
    _c("p1_fold_pair_main16_scalar", 1, 8, 16, (8,), 8, 3, up=1, pre=1, ypad=16, y_coff=16, filters='unfolded', off={'w': 1}, passes=(1,), expect={1: "fold.pair:Main16_scalar"}),
    _c("p1_fold_plain_main16_scalar", 1, 8, 16, (48,), 4, 4, up=1, xpad=4, filters='unfolded', off={'w': 1}, passes=(1,), expect={1: "fold.plain:Main16_scalar"}),
    _c("p1_fold_plain_n16_vec", 2, 4, 4, (16,), 32, 2, up=1, passes=(1,), expect={1: "fold.plain:N16_vec"}),
    _c("p1_fold_plain_narrow_scalar", 2, 16, 16, (32,), 8, (3, 2), up=1, passes=(1,), expect={1: "fold.plain:Narrow_scalar"}),
    _c("p1_fold_plain_narrow_vec", 4, 8, 16, (32,), 32, 2, up=1, xpad=4, passes=(1,), expect={1: "fold.plain:Narrow_vec"}),
    _c("p1_fold_plain_small16_x3s", 1, 8, 16, (48,), 4, 4, up=1, xpad=4, passes=(1,), expect={1: "fold.plain:Small16_x3s"}),
    _c("p1_igemm_act_main16_scalar", 1, 2, 2, (40,), 1, 3, pre=3, xpad=1, y_coff=4, passes=(1,), expect={1: "igemm.act:Main16_scalar"}),
    _c("p1_igemm_act_main16_x2h", 64, 32, 32, (128,), 4, 4, stride=2, pre=4, xpad=2, ypad=4, passes=(1,), expect={1: "igemm.act:Main16_x2h"}),
    _c("p1_igemm_act_main16_x3s", 64, 32, 32, (128,), 4, 4, stride=2, pre=4, xpad=2, ypad=4, ws='null', passes=(1,), expect={1: "igemm.act:Main16_x3s"}),
    _c("p1_igemm_act_narrow_scalar", 3, 2, 2, (20,), 12, 1, stride=2, pre=4, xpad=2, passes=(1,), expect={1: "igemm.act:Narrow_scalar"}),
    _c("p1_igemm_act_narrow_vec", 8, 2, 2, (32,), 224, 1, pre=3, xpad=2, ypad=4, y_coff=4, passes=(1,), expect={1: "igemm.act:Narrow_vec"}),
    _c("p1_igemm_act_small16_x2h", 2, 2, 2, (128,), 32, 1, pre=4, passes=(1,), expect={1: "igemm.act:Small16_x2h"}),
    _c("p1_igemm_act_small16_x3s", 2, 2, 2, (128,), 32, 1, pre=4, ws='null', passes=(1,), expect={1: "igemm.act:Small16_x3s"}),
    _c("p1_igemm_pair_main16_x2h", 16, 64, 64, (1,), 4, 1, pre=2, xpad=1, passes=(1,), expect={1: "igemm.pair:Main16_x2h"}),
    _c("p1_igemm_pair_main16_x3s", 16, 64, 64, (1,), 4, 1, pre=2, xpad=1, ws='null', passes=(1,), expect={1: "igemm.pair:Main16_x3s"}),
    _c("p1_igemm_pair_small16_x3s", 2, 2, 2, (2,), 4, (1, 5), pre=1, xpad=1, y_coff=4, ws='null', passes=(1,), expect={1: "igemm.pair:Small16_x3s"}),
    _c("p1_igemm_plain_narrow_vec", 16, 8, 4, (32,), 32, 1, ypad=4, passes=(1,), expect={1: "igemm.plain:Narrow_vec"}),
    _c("p1_igemm_pool_act_main16_scalar", 1, 2, 2, (48,), 20, (2, 3), stride=2, up=1, pre=3, filters='unfolded', off={'w': 1}, passes=(1,), expect={1: "igemm_pool.act:Main16_scalar"}),
    _c("p1_igemm_pool_act_main16_x2h", 64, 4, 64, (40,), 164, (5, 1), up=1, pre=4, xpad=4, passes=(1,), expect={1: "igemm_pool.act:Main16_x2h"}),
    _c("p1_igemm_pool_act_n16_vec", 1, 8, 16, (1,), 16, 2, up=1, pre=3, y_coff=16, passes=(1,), expect={1: "igemm_pool.act:N16_vec"}),
    _c("p1_igemm_pool_act_narrow_scalar", 1, 8, 4, (20,), 4, (2, 3), up=1, pre=3, xpad=2, ypad=16, y_coff=4, passes=(1,), expect={1: "igemm_pool.act:Narrow_scalar"}),
    _c("p1_igemm_pool_act_small16_x2h", 1, 2, 2, (48,), 20, (2, 3), stride=2, up=1, pre=3, passes=(1,), expect={1: "igemm_pool.act:Small16_x2h"}),
    _c("p1_igemm_pool_pair_main16_x2h", 16, 32, 32, (3,), 16, 3, stride=2, up=1, pre=1, ypad=4, passes=(1,), expect={1: "igemm_pool.pair:Main16_x2h"}),
    _c("p1_igemm_pool_pair_small16_x2h", 1, 2, 2, (1, 3), 160, 1, stride=2, up=1, pre=1, y_coff=16, passes=(1,), expect={1: "igemm_pool.pair:Small16_x2h"}),
    _c("p1_igemm_pool_plain_main16_scalar", 1, 2, 2, (40,), 256, 1, up=1, xpad=1, ypad=4, filters='unfolded', off={'w': 1}, passes=(1,), expect={1: "igemm_pool.plain:Main16_scalar"}),
    _c("p1_igemm_pool_plain_main16_x2h", 4, 64, 64, (40,), 12, (3, 2), stride=2, up=1, xpad=1, y_coff=4, passes=(1,), expect={1: "igemm_pool.plain:Main16_x2h"}),
    _c("p1_igemm_pool_plain_n16_vec", 1, 8, 4, (1,), 192, 1, up=1, xpad=1, ypad=4, passes=(1,), expect={1: "igemm_pool.plain:N16_vec"}),
    _c("p1_igemm_pool_plain_narrow_scalar", 4, 4, 32, (20,), 1, 2, up=1, xpad=2, ypad=16, y_coff=16, passes=(1,), expect={1: "igemm_pool.plain:Narrow_scalar"}),
    _c("p1_igemm_pool_plain_narrow_vec", 4, 2, 2, (32,), 128, (3, 5), stride=2, up=1, xpad=2, ypad=4, passes=(1,), expect={1: "igemm_pool.plain:Narrow_vec"}),
    _c("p1_igemm_pool_plain_small16_x2h", 1, 2, 2, (40,), 256, 1, up=1, xpad=1, ypad=4, passes=(1,), expect={1: "igemm_pool.plain:Small16_x2h"}),
    _c("p2_igemm_fold_narrow_vec_split", 4, 8, 16, (32,), 32, 2, up=1, xpad=4, passes=(2,), expect={2: "igemm_fold:Narrow_vec_split"}),
    _c("p2_igemm_fold_w160_vec", 8, 2, 2, (32,), 160, 5, up=1, pre=3, xpad=4, y_coff=4, passes=(2,), expect={2: "igemm_fold:W160_vec"}),
    _c("p2_igemm_fold_w224_vec_split", 4, 64, 64, (32,), 224, (3, 2), up=1, ypad=4, passes=(2,), expect={2: "igemm_fold:W224_vec_split"}),
    _c("p2_igemm_up_main16_scalar_split", 3, 8, 8, (48,), 132, (2, 3), up=1, pre=3, xpad=4, y_coff=1, passes=(2,), expect={2: "igemm_up:Main16_scalar_split"}),
    _c("p2_igemm_up_main_vec_split", 64, 2, 2, (40,), 228, (1, 5), up=1, passes=(2,), expect={2: "igemm_up:Main_vec_split"}),
    _c("p2_igemm_up_n16_scalar_split", 1, 4, 32, (40,), 1, 5, up=1, pre=1, passes=(2,), expect={2: "igemm_up:N16_scalar_split"}),
    _c("p2_igemm_up_n16_vec", 2, 2, 2, (48,), 12, (1, 5), up=1, pre=2, ypad=4, y_coff=16, passes=(2,), expect={2: "igemm_up:N16_vec"}),
    _c("p2_igemm_up_n16_vec_split", 8, 2, 64, (16,), 4, (5, 1), up=1, pre=1, xpad=4, ypad=16, y_coff=16, passes=(2,), expect={2: "igemm_up:N16_vec_split"}),
    _c("p2_igemm_up_narrow_scalar", 2, 4, 4, (8,), 20, 1, up=1, y_coff=4, passes=(2,), expect={2: "igemm_up:Narrow_scalar"}),
    _c("p2_igemm_up_narrow_scalar_split", 16, 4, 4, (48,), 20, 5, up=1, xpad=2, ypad=16, y_coff=16, passes=(2,), expect={2: "igemm_up:Narrow_scalar_split"}),
    _c("p2_igemm_up_narrow_vec", 1, 2, 2, (48,), 20, (2, 3), stride=2, up=1, pre=3, passes=(2,), expect={2: "igemm_up:Narrow_vec"}),
    _c("p2_igemm_up_narrow_vec_split", 2, 8, 8, (16,), 20, (1, 5), up=1, pre=1, y_coff=4, passes=(2,), expect={2: "igemm_up:Narrow_vec_split"}),
    _c("p2_igemm_up_w160_vec", 1, 4, 32, (128,), 144, 1, up=1, pre=1, y_coff=16, passes=(2,), expect={2: "igemm_up:W160_vec"}),
    _c("p2_igemm_up_w160_vec_split", 3, 8, 16, (16,), 160, (5, 1), up=1, pre=1, passes=(2,), expect={2: "igemm_up:W160_vec_split"}),
    _c("p2_igemm_up_w224_vec", 32, 4, 4, (48,), 196, 1, stride=2, up=1, pre=1, xpad=4, y_coff=4, passes=(2,), expect={2: "igemm_up:W224_vec"}),
    _c("p2_igemm_up_w224_vec_split", 4, 8, 16, (20,), 224, (1, 5), up=1, pre=1, ypad=16, y_coff=4, passes=(2,), expect={2: "igemm_up:W224_vec_split"}),
]
BY_NAME = {c["name"]: c for c in CASES}

# Route twins (branch 5 of the issue): (the case on the Winograd route, the same call with one property changed)
TWINS = [("s2", "s2_cmap"), ("s2", "s2_x_off"), ("s2", "s2_dy_off"), ("s2", "s2_dx_off"), ("s2", "s2_dw_off"), ("s2", "s2_ws_off"),
         ("plain3", "plain3_cmap"), ("plain3", "plain3_x_off"), ("up3", "up3_nofilters"), ("up3", "up3_dw_off")]


def seed_of(name):
    s = 0
    for i, ch in enumerate(name):
        s = (s * 131 + ord(ch) + i) % 2147483629
    return s


def base_name(case):
    """cases that differ only in how the call is made share their inputs and their reference"""
    key = tuple((k, case[k]) for k in ("N", "H", "W", "segs", "Cout", "KH", "KW", "stride", "up", "pre", "cmap", "bias"))
    return repr(key)


# ------------------------------------------------------------------------------------------------------------------
# buffers: one flat allocation per operand: GUARD floats, `off` floats, the pitched tensor, GUARD floats
# ------------------------------------------------------------------------------------------------------------------
GUARD = 64


def shapes(case):
    """(rows, valid width, pitch, first valid column) of the pitched operands, element counts of the flat ones"""
    d = desc_fields(case)
    g = make_geo(d)
    return dict(x=(d["N"] * d["H"] * d["W"], d["C"], d["ldx"], 0),
                y=(d["N"] * g["OH"] * g["OW"], d["Cout"], d["ldy"], d["y_coff"]),
                dy=(d["N"] * g["OH"] * g["OW"], d["Cout"], d["ldy"], d["y_coff"]),
                dx=(d["N"] * d["H"] * d["W"], d["C"], lddx(case), 0),
                w=d["KH"] * d["KW"] * g["Ceff"] * d["Cout"], bias=d["Cout"])


def buffer_floats(case, name):
    """floats of the flat allocation the GPU test makes for operand `name` (x, y, dy, dx)"""
    rows, _, pitch, _ = shapes(case)[name]
    return 2 * GUARD + case["off"][name] + rows * pitch


# ------------------------------------------------------------------------------------------------------------------
# inputs and the fp64 reference (oracle/nets_torch.py), shared by the CPU and the GPU test, computed once per geometry
# ------------------------------------------------------------------------------------------------------------------
_cache = {}


def inputs(case):
    """dict of float32 torch tensors on the CPU: x [N, H, W, C], w [KH, KW, Ceff, Cout], bias [Cout], dy [N, OH, OW, Cout], and
    the prior contents y0 / dx0 for the accumulating calls"""
    import torch
    key = ("in", base_name(case))
    if key in _cache:
        return _cache[key]
    d = desc_fields(case)
    g = make_geo(d)
    gen = torch.Generator().manual_seed(seed_of(base_name(case)))
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    K = d["KH"] * d["KW"] * g["Ceff"]
    out = dict(x=r(d["N"], d["H"], d["W"], d["C"]), w=r(d["KH"], d["KW"], g["Ceff"], d["Cout"]) / math.sqrt(K),
               bias=r(d["Cout"]) * 0.1 if case["bias"] else None, dy=r(d["N"], g["OH"], g["OW"], d["Cout"]),
               y0=r(d["N"], g["OH"], g["OW"], d["Cout"]), dx0=r(d["N"], d["H"], d["W"], d["C"]))
    _cache[key] = out
    return out


def oracle(case, dtype=None, device="cpu", grads=True):
    """y, dx, dw of oracle.nets_torch.conv2d on the fp32 inputs, evaluated in `dtype` (default float64).  The weight is passed
    as p['V'] with g = the column norms, which weight_norm undoes (to one rounding); dw is the gradient with respect to the
    normalised weight, taken through the same composition with the weight as a leaf (oracle_pieces)."""
    import torch
    from oracle import nets_torch as NT
    dtype = dtype or torch.float64
    inp = inputs(case)
    x = inp["x"].to(device=device, dtype=dtype, copy=True).requires_grad_(True)
    w = inp["w"].to(device=device, dtype=dtype, copy=True).requires_grad_(True)
    b = inp["bias"].to(device=device, dtype=dtype) if case["bias"] else torch.zeros(case["Cout"], dtype=dtype, device=device)
    xs = list(torch.split(x, list(case["segs"]), dim=3))
    pre = PRE_NAME[case["pre"]]
    if case["Cout"] == 1:
        # (one output channel: the backward pass of torch's CPU convolution refuses the permuted weight; a second, zero
        # filter beside it changes no value)
        y = oracle_pieces(NT, xs, torch.cat([w, torch.zeros_like(w)], 3), torch.cat([b, torch.zeros_like(b)]), pre, case["stride"],
                          bool(case["up"]))[..., :1]
    else:
        y = oracle_pieces(NT, xs, w, b, pre, case["stride"], bool(case["up"]))
    out = dict(y=y.detach())
    if grads:
        dx, dw = torch.autograd.grad(y, [x, w], inp["dy"].to(device=device, dtype=dtype))
        out.update(dx=dx.detach(), dw=dw.detach())
    return out


def oracle_pieces(NT, xs, w, b, pre, stride, up):
    """oracle.nets_torch.conv2d (oracle/nets_torch.py:85-96) with the weight normalisation taken out: the same three calls on
    the same arguments.  tests/test_conv_routes_cpu.py checks that NT.conv2d itself gives the same y."""
    if up:
        xs = [NT.upsample2(__import__("torch").cat(list(xs), 3))]
    return NT.conv2d_nhwc(NT.apply_pre_activation(xs, pre, 3), w, stride) + b


def reference(case, device="cpu"):
    """fp64 oracle of a case's geometry: dict(y, dx, dw) of float64 tensors on `device`.  Not to be modified by callers."""
    key = ("ref", base_name(case), str(device))
    if key not in _cache:
        _cache[key] = oracle(case, device=device)
    return _cache[key]
