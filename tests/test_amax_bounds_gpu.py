"""GPU: amax records are bounds.  The kernels on two scaled fp16 pieces take the power-of-two scale of an operand from an amax
record, and the product passes maxima over groups of slices, shared records and records max-accumulated by several kernels:
values at or above the largest magnitude, never below, rarely equal.  Every other test passes the exact maximum.  Here each call
runs with NULL records (where the ABI allows it), with exact records, and with records multiplied by 2^1 and by 2^5, on the
sparse inputs of tests/conv_sparse.py (nonzeros within 2^-6 of the largest, a random 24-bit significand each).

What is expected, from the arithmetic (csrc/gemm_tile.h x2h_scale, x2h_store4): an operand element v is staged as
hi = fp16(v 2^s), lo = fp16(v 2^s - hi) with s = 14 - e, amax = m 2^e.  A record 2^k times larger lowers s by k.  As long as
v 2^(s - k) >= 1/2, its 24 significand bits lie at or above 2^-24, the spacing of fp16 subnormals, so both roundings see
the same bits against the same 11-bit grid and hi, lo are the earlier pieces times 2^-k exactly; the MFMAs add the same
products times 2^-k in fp32, and the epilogue multiplies by 2^k: the output is the same bit for bit.  With a nonzero
at least 2^-6 of the bound and k <= 5, v 2^(s - k) >= 2^13 2^-6 2^-5 = 4.
  - table cases on an `_x2h` route (forward: the record of x; input gradient: of dy), record of the sparse operand scaled and
    the weights' record exact: torch.equal to the exact-record result, which is torch.equal to the NULL-record one.
  - the same with the weights' record scaled as well: NOT bit-identical by this argument -- the weights are dense randn, a
    fraction 2^-8 or so of them lie below 2^-12 of their maximum, and with k = 5 such a weight is staged below 1/2, where its
    low bits fall under the fp16 subnormal spacing.  Each such weight is then off by at most 2^-25 2^(k - s), 2^-33 of the largest
    weight.  The bar of conv_sparse.bounds is asserted instead.
  - dense16 `h2` forward, otgan_dense16_bwd_slice_f32: the filters carry their own scale; the records bound the slices read,
    which are sparse: torch.equal.
  - otgan_dense16_chain_fwd_f32, otgan_dense16_chain_bwd_f32: the slices a chain produces are sums, dense in magnitude, and the
    next layer reads them under the same bound: small sums are staged below 1/2 once the bound grows.  Not bit-identical by
    the argument; every layer is held to the bar against fp64 computed from the GPU's own earlier slices.

Measured on an MI355X: all 44 x2h passes of the table are bit-identical under NULL, exact and inflated operand records (worst
error / bar 0.42, igemm:W224_x2h, as with NULL records in tests/test_conv_sparse_gpu.py).  With the weights' record inflated
too, a factor of 2 left every pass bit-identical and a factor of 32 changed 17 of them; worst error / bar 0.45
(igemm.act:Main16_x2h), but for the one run of WEAKER: 5.6, and 0.48 against its own bar.  dense16 h2 forward 0.24 and
bwd_slice 0.26, bit-identical; chain_fwd 0.30 (layer 1; 0.06 at layer 2, where every element has about 150 products),
chain_bwd 0.24 in one launch at 8 x 8 and 0.27 slice by slice at 16 x 16, the records the chains leave equal to the
largest magnitude written under every bound.
"""
import ctypes
import math

import pytest
import torch

import conv_routes as R
import conv_sparse as S
from conv_harness import Call
from test_conv_sparse_gpu import where
from tests import dense16_ref as D16

pytestmark = pytest.mark.gpu
F = 16
NREC = R.AMAX_RECORD_FLOATS
SCALES = (1, 2, 32)
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from otgan_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    for key in sorted(WORST):
        print("worst %-44s err/bar %.3f" % (key, WORST[key]))


def _note(key, worst):
    WORST[key] = max(WORST.get(key, 0.0), worst)


def _record(value, dev, slot=0):
    r = torch.zeros(NREC, device=dev)
    r[32 * slot] = value
    return r


# ------------------------------------------------------------------------------------------------------------------
# the table's x2h routes
# ------------------------------------------------------------------------------------------------------------------
# (case, run) asserted at a weaker bar, with the reason: one run of one of the 287 non-Winograd passes of the table
WEAKER = {
    ("p1_igemm_pool_act_main16_x2h", "both * 32"):
        "dx[27, 0, 18, 14] is one product, dy times a weight 2^-17 of the largest.  Under a weight record 32 times the maximum that "
        "weight is staged at 2^-9, its low piece below the fp16 subnormal spacing: it keeps 17 bits, and the element is off by 5.6 "
        "bars (5.56 in an fp64 emulation of the staging alone; 0.17 with records up to twice the maximum).  Asserted at the bar "
        "plus 2^-25 2^(e - 14) sum |dy| |act'|, the staging floor of the weights, e = frexp(32 max |w|).",
}

X2H = [c for c in R.CASES if any(isinstance(c["expect"][w], str) and c["expect"][w].endswith("_x2h") for w in c["passes"])]


@pytest.mark.parametrize("case", X2H, ids=[c["name"] for c in X2H])
def test_x2h_routes_take_records_as_bounds(dev, case):
    for which in case["passes"]:
        route = case["expect"][which]
        if R.is_error(route) or not route.endswith("_x2h"):
            continue
        variant = S.WHICH_OF_PASS[which][0]
        inp = S.inputs(case, variant)
        call = Call(case, dev, inp)
        b = S.bounds(case, variant, inp)
        a_field = "x_amax" if which == R.FWD else "dy_amax"
        a_max, w_max = float(inp[inp["sparse"]].abs().max()), float(inp["w"].abs().max())
        assert a_max == inp["amax"]
        runs = [("null", {})]
        runs += [("operand * %d" % k, {a_field: _record(a_max * k, dev), "w_amax": _record(w_max, dev, 3)}) for k in SCALES]
        runs += [("both * %d" % k, {a_field: _record(a_max * k, dev, 5), "w_amax": _record(w_max * k, dev)}) for k in SCALES[1:]]
        out = {}
        for name, recs in runs:
            what = "%s %s on %s, records %s" % (case["name"], ("fwd", "dgrad")[which], route, name)
            rc, text, got, flop, launches = call.run(which, **{k: v.data_ptr() for k, v in recs.items()})
            assert rc == R.OK, (what, rc, text)
            want = R.flops(case, which, route)
            assert abs(flop - want) <= 1e-9 * want, (what, flop, want)
            bb = b
            if (case["name"], name) in WEAKER:
                # the staged weights' absolute floor: half the fp16 subnormal spacing, 2^-25, under the scale 2^(14 - e) of the
                # inflated record, times the sum of |dy| |act'(x)| over the products of the element
                e = math.frexp(w_max * int(name.split()[-1]))[1]
                floor = 2.0 ** (e - 39) * S.evaluate(case, variant, dict(inp, w=torch.ones_like(inp["w"])), "abs")
                bb = dict(b, bar=b["bar"] + floor)
                print("%-90s err/bar %.3f at the bar of conv_sparse.bounds" % (what, S.over_bar(got, b, dev)[0]))
            worst, at, nwrong, first = S.over_bar(got, bb, dev)
            _note("%s %s" % (route, "both scaled" if name.startswith("both") else "operand scaled"), worst)
            print("%-90s err/bar %.3f%s" % (what, worst, "" if name in ("null", "operand * 1") else
                                            "  equal to exact records: %s" % torch.equal(got, out["operand * 1"])))
            assert worst <= 1.0, "%s: %.3f bars at (%s)" % (what, worst, where(at, tuple(b["ref"].shape), which))
            assert nwrong == 0, "%s: %d elements no product reaches are not bias + prior content" % (what, nwrong)
            out[name] = got
        assert torch.equal(out["null"], out["operand * 1"]), case["name"]
        for k in SCALES[1:]:
            assert torch.equal(out["operand * %d" % k], out["operand * 1"]), (case["name"], route, k)


# ------------------------------------------------------------------------------------------------------------------
# the growth kernels
# ------------------------------------------------------------------------------------------------------------------
def _eff(xs, mode):
    """[N,H,W,16 n] -> [N, 32 n, H, W]: crelu of the slices (D16.crelu_slices); "jac": a function whose Jacobian is |crelu'|;
    "ind": the indicator of crelu != 0"""
    parts = []
    for s in range(xs.shape[-1] // F):
        sl = xs[..., F * s:F * s + F]
        pos, neg = sl.clamp(min=0), (-sl).clamp(min=0)
        parts += {"ref": [pos, neg], "jac": [pos, -neg], "ind": [(pos > 0).to(sl.dtype), (neg > 0).to(sl.dtype)]}[mode]
    return torch.cat(parts, -1).permute(0, 3, 1, 2)


def _layer(eff, w):
    """conv3x3_same of effective channels [N, 32 k, H, W] with HWIO weights [9][32 k][16] -> NHWC"""
    k = eff.shape[1] // 32
    w4 = w.reshape(3, 3, 32 * k, F).permute(3, 2, 0, 1)
    return torch.nn.functional.conv2d(eff, w4, padding=1).permute(0, 2, 3, 1)


def _bounds(ref, A, n, prior):
    """conv_sparse.bounds for a growth layer (CReLU: e0 = 2^-20, no bias)"""
    ref = ref + prior.double()
    bar = (2.0 ** -20 + n.round() * S.U23) * A + S.U23 * (ref.abs() + prior.double().abs())
    return dict(ref=ref, A=A, n=n.round(), bar=bar, exact=A == 0, expected=prior.float())


def _forward_bounds(xs, w, prior):
    """layer: prior + conv3x3(crelu(xs), w); xs fp32 [N,H,W,16 k], w HWIO [9][32 k][16]"""
    xs, w = xs.double(), w.double()
    return _bounds(_layer(_eff(xs, "ref"), w), _layer(_eff(xs, "ref"), w.abs()), _layer(_eff(xs, "ind"), (w != 0).double()), prior)


def _gather_bounds(X, G, ws, c, prior):
    """gradient of slice c: prior + d/dx_c sum_{k > c} <G_k, conv3x3(crelu(slices [0, k)), w_k)> at the forward values X
    (fp32 [N,H,W,16 S]; G fp32 of the same shape; ws[k - 1] HWIO of layer k)"""
    S_ = X.shape[-1] // F
    X, G = X.double(), G.double()
    out = []
    for mode in ("ref", "abs", "ind"):
        xc = X[..., F * c:F * c + F].clone().requires_grad_(True)
        total = 0.0
        for k in range(c + 1, S_):
            xs = torch.cat([X[..., :F * c], xc, X[..., F * (c + 1):F * k]], -1)
            w, g = ws[k - 1].double(), G[..., F * k:F * k + F]
            if mode == "abs":
                w, g = w.abs(), g.abs()
            elif mode == "ind":
                w, g = (w != 0).double(), (g != 0).double()
            total = total + (_layer(_eff(xs, "ref" if mode == "ref" else "jac"), w) * g).sum()
        out.append(torch.autograd.grad(total, xc)[0])
    return _bounds(out[0], out[1], out[2], prior)


def _assert_bar(got, b, what, key):
    worst, at, nwrong, first = S.over_bar(got.cpu(), b, "cpu")
    _note(key, worst)
    reached = ~b["exact"]
    print("%-80s err/bar %.3f  median n %d  exact elements %d" % (what, worst, int(b["n"][reached].median()), int(b["exact"].sum())))
    assert worst <= 1.0, "%s: %.3f bars at (%s)" % (what, worst, where(at, tuple(b["ref"].shape), R.FWD))
    assert nwrong == 0, "%s: %d elements no product reaches are not their prior content" % (what, nwrong)


def _weights(nlayers, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(9, 2 * F * k, F, generator=g) * (0.05 / k ** 0.5) for k in range(1, nlayers + 1)]


def test_h2_forward_takes_records_as_bounds(dev, N=8, H=32, n_own=1):
    """dense16_fwd_h2_kernel through otgan_conv2d_fwd_pf_f32 (list_width = 16, prepared filters), one record per slice"""
    from otgan_amd import _lib, ops
    from otgan_amd._lib_layers import ConvDesc
    L = _lib.lib()
    C0, g0, k = 32, 1, 1 + n_own
    Ctot = C0 + (k + 2) * F
    w = _weights(n_own, 5)[n_own - 1]
    wT = w.reshape(-1, F).t().contiguous().to(dev)
    xs, amax = S.sparse_tensor((N, H, H, n_own * F), 501, 8.0 / (9 * F * n_own))
    buf0 = torch.randn(N, H, H, Ctot, generator=torch.Generator().manual_seed(6))
    buf0[..., C0 + g0 * F:C0 + k * F] = xs
    prior = buf0[..., C0 + k * F:C0 + (k + 1) * F].clone()
    b = _forward_bounds(xs, w, prior)
    desc = ConvDesc(N, H, H, n_own * F, Ctot, 0, 3, 3, 1, F, Ctot, C0 + k * F, ops.ACT["crelu"], 1)
    desc.y_accumulate, desc.list_width = 1, F
    assert L.otgan_dense16_h2_ok(ctypes.byref(desc)) == 1
    fq = torch.empty(int(L.otgan_dense16_filter_bytes(n_own)), dtype=torch.uint8, device=dev)
    pw, pn, pf = (ctypes.c_void_p * 1)(wT.data_ptr()), (ctypes.c_int * 1)(n_own), (ctypes.c_void_p * 1)(fq.data_ptr())
    _lib.check(L.otgan_dense16_prepare_filters_f32(ctypes.cast(pw, ctypes.c_void_p), ctypes.cast(pn, ctypes.c_void_p),
                                                   ctypes.cast(pf, ctypes.c_void_p), 1, _lib.stream_ptr()), "prepare")
    cmap, _inv = ops.channel_maps((F,) * n_own, ops.ACT["crelu"], dev)
    out = {}
    for s in SCALES:
        buf = buf0.to(dev)
        rec = torch.zeros((2 + n_own, NREC), device=dev)
        for j in range(n_own):
            rec[1 + j, 32 * (j % 16)] = xs[..., F * j:F * j + F].abs().max() * s
        desc.x_amax, desc.x_amax_count, desc.y_amax_out = rec[0].data_ptr(), 1 + n_own, rec[1 + n_own].data_ptr()
        ops.conv_fwd_raw(desc, buf[..., C0 + g0 * F:], cmap, wT, None, buf, fq)
        torch.cuda.synchronize()
        got = buf[..., C0 + k * F:C0 + (k + 1) * F].cpu()
        mask = torch.ones(Ctot, dtype=torch.bool)
        mask[C0 + k * F:C0 + (k + 1) * F] = False
        assert torch.equal(buf.cpu()[..., mask], buf0[..., mask])
        _assert_bar(got, b, "dense16 h2 forward N=%d H=%d slices=%d records * %d" % (N, H, n_own, s), "dense16 h2 forward")
        assert float(rec[1 + n_own].max()) == float(got.abs().max())
        out[s] = got
    for s in SCALES[1:]:
        assert torch.equal(out[s], out[1]), s


def test_bwd_slice_takes_records_as_bounds(dev, N=64, H=8, npairs=3):
    """dense16_bwd_h2_kernel through otgan_dense16_bwd_slice_f32: rec0 one bounding record, rec1 one record per source slice"""
    from otgan_amd import _lib
    L = _lib.lib()
    S_ = npairs + 1
    ld = S_ * F + 16
    ws = _weights(npairs, 7)
    X = torch.randn(N, H, H, ld, generator=torch.Generator().manual_seed(8))
    G, amax = S.sparse_tensor((N, H, H, ld), 502, 8.0 / (9 * F * npairs))
    G[..., :F] = torch.randn(N, H, H, F, generator=torch.Generator().manual_seed(9))      # the prior content of slice 0
    b = _gather_bounds(X[..., :S_ * F], G[..., :S_ * F], ws, 0, G[..., :F])
    Xd = X.to(dev)
    wd, fwd, pf = D16.prepare_filters(L, _lib, ws, dev)
    bq = D16.prepare_bwd_filters(L, _lib, wd, fwd, pf, 0, dev)
    out = {}
    for s in SCALES:
        Gd = G.to(dev)
        rec = torch.zeros((2 + npairs, NREC), device=dev)
        rec[0, 0] = G[..., F:S_ * F].abs().max() * s
        for j in range(npairs):
            rec[1 + j, 32 * (j % 16)] = G[..., (1 + j) * F:(2 + j) * F].abs().max() * s
        _lib.check(L.otgan_dense16_bwd_slice_f32(N, H, H, npairs, Gd.data_ptr() + 4 * F, ld, bq.data_ptr(), Xd.data_ptr(), ld,
                                                 Gd.data_ptr(), rec[0].data_ptr(), 1, rec[1].data_ptr(), npairs,
                                                 rec[1 + npairs].data_ptr(), _lib.stream_ptr()), "bwd_slice")
        torch.cuda.synchronize()
        assert torch.equal(Gd.cpu()[..., F:], G[..., F:])
        got = Gd[..., :F].cpu()
        _assert_bar(got, b, "dense16 bwd_slice N=%d H=%d pairs=%d records * %d" % (N, H, npairs, s), "dense16 bwd_slice")
        assert float(rec[1 + npairs].max()) == float(got.abs().max())
        out[s] = got
    for s in SCALES[1:]:
        assert torch.equal(out[s], out[1]), s


def test_chain_forward_takes_records_as_bounds(dev, N=37, H=16, nslices=3):
    """otgan_dense16_chain_fwd_f32: every layer against fp64 from the GPU's own earlier slices, under exact and inflated records"""
    from otgan_amd import _lib
    L = _lib.lib()
    C0 = 32
    Ctot = C0 + nslices * F + 16
    ws = _weights(nslices - 1, 11)
    grp0, amax = S.sparse_tensor((N, H, H, nslices * F), 503, 8.0 / (9 * F))
    buf0 = torch.randn(N, H, H, Ctot, generator=torch.Generator().manual_seed(12))
    buf0[..., C0:C0 + nslices * F] = grp0
    wd, fwd, pf = D16.prepare_filters(L, _lib, ws, dev)
    for s in SCALES:
        buf = buf0.to(dev)
        rec = torch.zeros((1 + nslices, NREC), device=dev)
        rec[0, 0] = grp0.abs().max() * s
        rec[1, 32] = grp0[..., :F].abs().max() * s
        _lib.check(L.otgan_dense16_chain_fwd_f32(N, H, H, nslices, buf.data_ptr() + 4 * C0, Ctot, ctypes.cast(pf, ctypes.c_void_p),
                                                 rec.data_ptr(), _lib.stream_ptr()), "chain_fwd")
        torch.cuda.synchronize()
        got = buf.cpu()
        assert torch.equal(got[..., :C0 + F], buf0[..., :C0 + F]) and torch.equal(got[..., C0 + nslices * F:], buf0[..., C0 + nslices * F:])
        grp = got[..., C0:C0 + nslices * F]
        for j in range(1, nslices):
            b = _forward_bounds(grp[..., :F * j].contiguous(), ws[j - 1], grp0[..., F * j:F * j + F])
            _assert_bar(grp[..., F * j:F * j + F], b, "dense16 chain_fwd N=%d H=%d layer %d records * %d" % (N, H, j, s), "dense16 chain_fwd")
            assert float(rec[1 + j].max()) == float(grp[..., F * j:F * j + F].abs().max()), j


@pytest.mark.parametrize("H", [8, 16], ids=["8x8_one_launch", "16x16_per_slice"])
def test_chain_backward_takes_records_as_bounds(dev, H, N=37, nslices=3):
    """otgan_dense16_chain_bwd_f32: every slice against fp64 from the GPU's own later slices, under exact and inflated records"""
    from otgan_amd import _lib
    L = _lib.lib()
    C0 = 32
    Ctot = C0 + nslices * F + 16
    ws = _weights(nslices - 1, 13)
    X = torch.randn(N, H, H, Ctot, generator=torch.Generator().manual_seed(14))
    G0 = torch.randn(N, H, H, Ctot, generator=torch.Generator().manual_seed(15))
    grp = slice(C0, C0 + nslices * F)
    G0[..., grp], amax = S.sparse_tensor((N, H, H, nslices * F), 504, 8.0 / (9 * F))
    wd, fwd, pf = D16.prepare_filters(L, _lib, ws, dev)
    bqs = [D16.prepare_bwd_filters(L, _lib, wd, fwd, pf, c, dev) for c in range(nslices - 1)]
    pb = (ctypes.c_void_p * (nslices - 1))(*[q.data_ptr() for q in bqs])
    Xd = X.to(dev)
    last = C0 + (nslices - 1) * F
    for s in SCALES:
        Gd = G0.to(dev)
        rec = torch.zeros((1 + nslices, NREC), device=dev)
        rec[0, 0] = G0[..., grp].abs().max() * s
        rec[nslices, 32] = G0[..., last:last + F].abs().max() * s
        _lib.check(L.otgan_dense16_chain_bwd_f32(N, H, H, nslices, Gd.data_ptr() + 4 * C0, Ctot, Xd.data_ptr() + 4 * C0, Ctot,
                                                 ctypes.cast(pb, ctypes.c_void_p), rec[0].data_ptr(), rec[1].data_ptr(),
                                                 _lib.stream_ptr()), "chain_bwd")
        torch.cuda.synchronize()
        got = Gd.cpu()
        assert torch.equal(got[..., :C0], G0[..., :C0]) and torch.equal(got[..., last:], G0[..., last:])
        for c in range(nslices - 2, -1, -1):
            b = _gather_bounds(X[..., grp], got[..., grp], ws, c, G0[..., C0 + F * c:C0 + F * c + F])
            _assert_bar(got[..., C0 + F * c:C0 + F * c + F], b, "dense16 chain_bwd N=%d H=%d slice %d records * %d" % (N, H, c, s),
                        "dense16 chain_bwd")
            assert float(rec[1 + c].max()) == float(got[..., C0 + F * c:C0 + F * c + F].abs().max()), c
