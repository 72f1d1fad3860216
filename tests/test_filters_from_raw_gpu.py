"""GPU: the Winograd filter operands made from the RAW weight-norm direction V and scale = g * inv_norm
(otgan_weightnorm_scale_amax_f32 + otgan_conv2d_prepare_filters_raw_f32) are the operands made from the normalised copies
w / wT (otgan_weightnorm_fwd_amax_f32 + otgan_conv2d_prepare_filters_f32), byte for byte: header scales and both fp16
planes, inv_norm, and the value of the amax record.

The record is compared by its VALUE (the maximum over its sub-slots, which is all any consumer reads: common.h
amax_record_value), not slot by slot: which sub-slot a workgroup commits to depends on its block index, and the two routes
reduce with different grids.  Filter buffers are pre-filled with one pattern on both routes, so the words neither route
writes (unused header words, structurally absent blocks of the strided layers) compare equal and a refused call can be
shown to have written nothing.

Shapes: the smallest at which each kernel can go wrong, from the GEMM's K granule X3_BK (gemm_x3.h) -- one granule, two
granules with a channel count that leaves partly filled workgroups, operands that fall back to the fp32 layout."""
import ctypes
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = 0x7FC0DEAD          # a NaN: an operand word left at it would poison the GEMM


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _x3_bk():
    src = open(os.path.join(ROOT, "ot-gan_amd", "csrc", "gemm_x3.h")).read()
    return int(re.search(r"\bX3_BK\s*=\s*(\d+)", src).group(1))


BK = _x3_bk()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rec_value(rec):
    """Value of an amax record as a bit pattern (sign-masked magnitudes: non-negative as int32, NaN above infinity)."""
    return int(_bits(rec).max())


def _guarded(nbytes, dev):
    return torch.full(((nbytes + 3) // 4,), PATTERN, dtype=torch.int32, device=dev)


def _layer(name, dev):
    """(descriptor, K, Cout, (forward which, dgrad which)) of a layer kind."""
    from otgan_amd import ops
    N, H, W, C, Cout, k, stride, up, pre = LAYERS[name]
    x = torch.empty(N, H, W, C, device=dev)
    mult = 2 if pre == "crelu" else 1
    desc = ops.make_desc(x, C, up, k, k, stride, Cout, Cout, 0, ops.ACT[pre])
    return desc, k * k * C * mult, Cout, ((2, 3) if up else (0, 1))


LAYERS = {
    # name: N, H, W, C, Cout, k, stride, upsample, preact
    "up5_one_granule": (2, 4, 4, BK, BK // 4, 5, 1, True, None),          # Cin = X3_BK, 4 * Cout = X3_BK
    "up5_ragged": (2, 4, 4, 2 * BK, 24, 5, 1, True, None),                # 24 of a workgroup's 32 / 64 columns in the last block
    "up5_fp32_dgrad_operand": (2, 4, 4, 2 * BK, 20, 5, 1, True, None),    # 4 * Cout % X3_BK != 0: that operand in the fp32 layout
    "s2_crelu_min": (2, 8, 8, 16, BK, 5, 2, False, "crelu"),              # Ceff = 32: the smallest the strided path takes
    "s2_crelu_narrow_out": (2, 8, 8, 16, 12, 5, 2, False, "crelu"),       # Cout % X3_BK != 0, partly filled row blocks
    "up3_crelu": (2, 4, 4, 16, 16, 3, 1, True, "crelu"),                  # only which = 2 / 3; dgrad operand padded to X3_BK
}


def _weights(K, Cout, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)
    V = (torch.randn(K, Cout, generator=gen) * 0.05).to(dev)
    g = (torch.rand(Cout, generator=gen) + 0.5).to(dev)
    return V, g


def _old_route(desc, V, g, whichs):
    """inv_norm, record and guarded filter buffers through the normalised copies."""
    from otgan_amd import ops, _lib
    L = _lib.lib()
    w, wT, inv = ops.weightnorm_fwd(V, g)
    rec = ops.amax_of(w)
    d = ops.launch_desc(desc, w_amax=rec)
    out = {}
    for which in whichs:
        nbytes = L.otgan_conv2d_filter_bytes(ctypes.byref(d), which)
        assert nbytes > 0
        buf = _guarded(nbytes, V.device)
        src = wT if which in (0, 2) else w
        _lib.check(L.otgan_conv2d_prepare_filters_f32(ctypes.byref(d), which, src.data_ptr(), buf.data_ptr(), buf.numel() * 4,
                                                      _lib.stream_ptr()), "old")
        out[which] = buf
    return inv, rec, out


def _new_route(desc, V, g, whichs):
    from otgan_amd import ops, _lib
    L = _lib.lib()
    scale, inv = ops.weightnorm_scale(V, g)
    rec = ops.amax_of(scale)
    d = ops.launch_desc(desc, w_amax=rec)
    out = {}
    for which in whichs:
        buf = _guarded(L.otgan_conv2d_filter_bytes(ctypes.byref(d), which), V.device)
        _lib.check(L.otgan_conv2d_prepare_filters_raw_f32(ctypes.byref(d), which, V.data_ptr(), scale.data_ptr(), buf.data_ptr(),
                                                          buf.numel() * 4, _lib.stream_ptr()), "new")
        out[which] = buf
    return inv, scale, rec, out


@pytest.mark.parametrize("order", ["fwd", "bwd", "fwd_bwd", "bwd_fwd"])
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_filters_byte_for_byte(dev, name, order):
    desc, K, Cout, (wf, wb) = _layer(name, dev)
    whichs = {"fwd": (wf,), "bwd": (wb,), "fwd_bwd": (wf, wb), "bwd_fwd": (wb, wf)}[order]
    V, g = _weights(K, Cout, dev, seed=len(name))
    g[Cout // 2] = -g[Cout // 2]
    inv_o, rec_o, old = _old_route(desc, V, g, whichs)
    inv_n, scale, rec_n, new = _new_route(desc, V, g, whichs)
    assert torch.equal(_bits(inv_o), _bits(inv_n))
    assert torch.equal(_bits(scale), _bits(g * inv_o))
    assert _rec_value(rec_o) == _rec_value(rec_n) and _rec_value(rec_n) > 0
    for which in whichs:
        assert old[which].numel() == new[which].numel()
        diff = (old[which] != new[which]).nonzero()
        assert diff.numel() == 0, f"which={which}: {diff.numel()} words differ, first at {int(diff[0])}"
        assert int((new[which] != PATTERN).sum()) > 0


def _norms_both(V, g):
    from otgan_amd import ops
    w, _wT, inv_o = ops.weightnorm_fwd(V, g)
    scale, inv_n = ops.weightnorm_scale(V, g)
    return w, inv_o, ops.amax_of(w), scale, inv_n, ops.amax_of(scale)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_planted_maximum_negative_gain_zero_column(dev, sign):
    """13 row chunks, two column blocks; the maximum of |w| sits in one (k, c) whose gain is negative; one column is zero (the
    1e-12 clamp)."""
    K, Cout = 25 * BK, 72
    V, g = _weights(K, Cout, dev, seed=5)
    g[70] = -40.0
    V[611, 70] = sign * 7.0
    V[:, 11] = 0.0
    w, inv_o, rec_o, scale, inv_n, rec_n = _norms_both(V, g)
    assert torch.equal(_bits(inv_o), _bits(inv_n)) and torch.equal(_bits(scale), _bits(g * inv_o))
    assert _rec_value(rec_o) == _rec_value(rec_n) == int(_bits(w.abs().max()))
    assert float(w.abs().max()) == abs(float(w[611, 70]))
    assert float(w[:, 11].abs().max()) == 0.0 and abs(float(inv_n[11]) - 1e6) < 1.0      # rsqrt(1e-12), to the unit's rounding


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nan_and_inf_are_as_loud(dev, bad):
    """As loud, not the same bits: either route leaves a NaN in the record and NaN in all 36 scales of both headers (the
    layer's output is then NaN); which NaN pattern is not compared.  inv_norm is finite on both routes and is compared bitwise."""
    desc, K, Cout, (wf, wb) = _layer("up5_one_granule", dev)
    V, g = _weights(K, Cout, dev, seed=9)
    V[77, 2] = bad
    inv_o, rec_o, old = _old_route(desc, V, g, (wf, wb))
    inv_n, scale, rec_n, new = _new_route(desc, V, g, (wf, wb))
    assert torch.equal(_bits(inv_o), _bits(inv_n))
    nan_from = 0x7F800001            # record values are magnitudes' bit patterns: above infinity = NaN
    assert _rec_value(rec_o) >= nan_from and _rec_value(rec_n) >= nan_from
    for which in (wf, wb):
        ho, hn = old[which][:128].view(torch.float32), new[which][:128].view(torch.float32)
        assert torch.isnan(ho[16:52]).all() and torch.isnan(hn[16:52]).all()      # the 36 scales


@pytest.mark.parametrize("case", ["cout_not_multiple_of_4", "misaligned_view"])
def test_scalar_reduction_path(dev, case):
    K = 25 * BK
    Cout = 6 if case == "cout_not_multiple_of_4" else 8
    V0, g = _weights(K, Cout, dev, seed=2)
    if case == "misaligned_view":
        store = torch.zeros(K * Cout + 1, device=dev)
        V = store[1:].view(K, Cout)
        V.copy_(V0)
        assert V.data_ptr() % 16 == 4
    else:
        V = V0
    w, inv_o, rec_o, scale, inv_n, rec_n = _norms_both(V, g)
    assert torch.equal(_bits(inv_o), _bits(inv_n)) and torch.equal(_bits(scale), _bits(g * inv_o))
    assert _rec_value(rec_o) == _rec_value(rec_n) == int(_bits(w.abs().max()))


def test_refusals(dev):
    from otgan_amd import ops, _lib
    L = _lib.lib()

    def both(desc, which, V, scale, w, buf, nbytes=None):
        nbytes = buf.numel() * 4 if nbytes is None else nbytes
        before = buf.clone()
        ro = L.otgan_conv2d_prepare_filters_f32(ctypes.byref(desc), which, w, buf.data_ptr(), nbytes, _lib.stream_ptr())
        rn = L.otgan_conv2d_prepare_filters_raw_f32(ctypes.byref(desc), which, V, scale, buf.data_ptr(), nbytes,
                                                    _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(buf, before), "a refused call wrote to the filter buffer"
        return ro, rn

    desc, K, Cout, _ = _layer("s2_crelu_min", dev)
    V, g = _weights(K, Cout, dev)
    scale, _inv = ops.weightnorm_scale(V, g)
    w, wT, _ = ops.weightnorm_fwd(V, g)
    d = ops.launch_desc(desc, w_amax=ops.amax_of(scale))
    buf = _guarded(L.otgan_conv2d_filter_bytes(ctypes.byref(d), 0), dev)
    assert both(d, 2, V.data_ptr(), scale.data_ptr(), wT.data_ptr(), buf) == (-1, -1)          # strided layers have no which = 2
    assert both(d, 0, V.data_ptr(), scale.data_ptr(), wT.data_ptr(), buf, 16) == (-2, -2)      # short buffer
    assert both(d, 0, None, scale.data_ptr(), None, buf) == (-1, -1)                           # null source
    assert both(d, 0, V.data_ptr() + 4, scale.data_ptr(), wT.data_ptr() + 4, buf) == (-1, -1)  # misaligned source
    plain = ops.launch_desc(ops.make_desc(torch.empty(2, 8, 8, 16, device=dev), 16, False, 3, 3, 1, 32, 32, 0, 0),
                            w_amax=ops.amax_of(scale))
    assert both(plain, 0, V.data_ptr(), scale.data_ptr(), wT.data_ptr(), buf) == (-1, -1)      # no Winograd path at all
    # the raw entry alone: no record, and filters that exist only from FOLDED weights
    before = buf.clone()
    assert L.otgan_conv2d_prepare_filters_raw_f32(ctypes.byref(desc), 0, V.data_ptr(), scale.data_ptr(), buf.data_ptr(),
                                                  buf.numel() * 4, _lib.stream_ptr()) == -1
    assert b"w_amax" in L.otgan_last_error()
    du, Ku, Cu, _ = _layer("up5_one_granule", dev)
    Vu, gu = _weights(Ku, Cu, dev)
    su, _ = ops.weightnorm_scale(Vu, gu)
    du = ops.launch_desc(du, w_amax=ops.amax_of(su))
    bu = _guarded(max(L.otgan_conv2d_filter_bytes(ctypes.byref(du), wh) for wh in range(4)), dev)
    bu0 = bu.clone()
    for which in (0, 1):
        assert L.otgan_conv2d_filter_bytes(ctypes.byref(du), which) > 0
        assert L.otgan_conv2d_prepare_filters_raw_f32(ctypes.byref(du), which, Vu.data_ptr(), su.data_ptr(), bu.data_ptr(),
                                                      bu.numel() * 4, _lib.stream_ptr()) == -4
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and torch.equal(bu, bu0)


WHOLE_LAYERS = {      # (as LAYERS; shapes whose three passes tests/test_layers_gpu.py runs too)
    "up5": (2, 4, 4, 2 * BK, 24, 5, 1, True, None),
    "s2_crelu": (3, 16, 16, 16, 48, 5, 2, False, "crelu"),
    "up3_crelu": (2, 4, 4, 32, 16, 3, 1, True, "crelu"),
}


@pytest.mark.parametrize("name", sorted(WHOLE_LAYERS))
def test_layer_forward_backward_equal(dev, name, monkeypatch):
    """One layer through Conv2dFunction on either route: output and every gradient bit-identical; the new route is the one
    taken, and its cache entry holds no normalised weights."""
    from otgan_amd import ops
    N, H, W, C, Cout, k, stride, up, pre = WHOLE_LAYERS[name]
    gen = torch.Generator().manual_seed(1)
    x0 = torch.randn(N, H, W, C, generator=gen).to(dev)
    mult = 2 if pre == "crelu" else 1
    V0 = (torch.randn(k, k, C * mult, Cout, generator=gen) * 0.05).to(dev)
    g0, b0 = (torch.rand(Cout, generator=gen) + 0.5).to(dev), torch.randn(Cout, generator=gen).to(dev)
    res = {}
    for raw in (False, True):
        monkeypatch.setattr(ops, "FILTERS_FROM_RAW", raw)
        x, V, g, b = (t.clone().requires_grad_(True) for t in (x0, V0, g0, b0))
        y = ops.conv2d_op(x, V, g, b, stride=stride, upsample=up, preact=ops.ACT[pre])
        assert ("raw" in y.grad_fn.filt) == raw and y.grad_fn.filt["fwd"] is not None
        if raw:
            ent = ops._wcache[id(V)][3]
            assert ent[0] is ent[1] and ent[0].numel() == Cout
        grads = torch.autograd.grad(y, [x, V, g, b], torch.ones_like(y) * 0.5 + y.detach() * 0.1)
        ops.join_side_stream(grads)
        assert y.grad_fn.filt["bwd"] is not None
        res[raw] = [y.detach()] + list(grads)
    for a, c, what in zip(res[False], res[True], ("y", "dx", "dV", "dg", "db")):
        assert torch.equal(_bits(a), _bits(c)), what


def test_entry_without_weights_serves_only_calls_that_read_none(dev, monkeypatch):
    """The cache is keyed by the parameter.  A call whose strided passes leave the Winograd route (a list input: the implicit
    GEMM reads weights) must not be served by an entry that holds none: same bits as on the old route, and the entry stays
    for the calls it was made for."""
    from otgan_amd import ops
    N, H, W, C, Cout, k, stride, up, pre = WHOLE_LAYERS["s2_crelu"]
    gen = torch.Generator().manual_seed(4)
    x0 = torch.randn(N, H, W, C, generator=gen).to(dev)
    V0 = (torch.randn(k, k, 2 * C, Cout, generator=gen) * 0.05).to(dev)
    g0, b0 = (torch.rand(Cout, generator=gen) + 0.5).to(dev), torch.randn(Cout, generator=gen).to(dev)
    res = {}
    for raw in (False, True):
        monkeypatch.setattr(ops, "FILTERS_FROM_RAW", raw)
        V, g, b = (t.clone().requires_grad_(True) for t in (V0, g0, b0))
        y1 = ops.conv2d_op(x0.clone().requires_grad_(True), V, g, b, stride=stride, preact=ops.ACT[pre])
        assert ("raw" in y1.grad_fn.filt) == raw
        x = x0.clone().requires_grad_(True)
        y = ops.conv2d_op(x, V, g, b, stride=stride, preact=ops.ACT[pre], segs=(C // 2, C // 2))
        assert "raw" not in y.grad_fn.filt and y.grad_fn.cmap is not None
        grads = torch.autograd.grad(y, [x, V, g], torch.ones_like(y) * 0.5 + y.detach() * 0.1)
        ops.join_side_stream(grads)
        assert ("raw" in ops._wcache[id(V)][3][3]) == raw
        res[raw] = [y1.detach(), y.detach()] + list(grads)
    for a, c, what in zip(res[False], res[True], ("y of the single-tensor call", "y", "dx", "dV", "dg")):
        assert torch.equal(_bits(a), _bits(c)), what


def _run(dev, graph, steps, ngd):
    from otgan_amd.trainer import OTGAN, default_args
    args = default_args(model="dcgan", batch_size=4, nr_gpu=2, sinkhorn_lambda=100.0, nr_sinkhorn_iter=20, nr_gen_per_disc=ngd,
                        seed=3, step_graph=graph)
    m = OTGAN(args, dev)
    gen = torch.Generator().manual_seed(11)
    xs = [(torch.rand(m.nb, 32, 32, 3, generator=gen) * 2 - 1).to(dev) for _ in range(3)]
    torch.manual_seed(7)
    dists = [m.step(xs[i % 3])["distance"].clone() for i in range(steps)]
    full = m.state_dict(full=True)
    out = {"state": {k: v.clone() for k, v in full.items() if torch.is_tensor(v)}, "opt": full["__optim__"],
           "dists": torch.stack(dists).cpu(), "captured": sorted(m.graphs.graphs) if m.graphs is not None else [],
           "dead": m.graphs.dead if m.graphs is not None else None}
    m.close()
    return out


def test_training_steps_equal(dev, monkeypatch):
    """DCGAN, 2 x 4 images, one critic step and two generator steps per period: eager on the old route against eager and
    step-graph replay on the new one.  Losses, parameters and Adam's moments (every gradient of every step went into them)
    bit-identical; the replayed run captured and replayed all three kinds of step ("disc", "gen1", "gen")."""
    from otgan_amd import ops
    ngd, steps = 2, 9            # eager period, three captures, then a replay of each kind
    monkeypatch.setattr(ops, "FILTERS_FROM_RAW", False)
    ref = _run(dev, False, steps, ngd)
    monkeypatch.setattr(ops, "FILTERS_FROM_RAW", True)
    for graph in (False, True):
        got = _run(dev, graph, steps, ngd)
        if graph:
            assert got["dead"] is None and got["captured"] == ["disc", "gen", "gen1"]
        assert torch.equal(ref["dists"], got["dists"]), (graph, ref["dists"], got["dists"])
        for k in ref["state"]:
            assert torch.equal(ref["state"][k], got["state"][k]), (graph, k)
        for net in ("gen", "disc"):
            assert ref["opt"][net]["t"] == got["opt"][net]["t"]
            for sa, sb in zip(ref["opt"][net]["slots"], got["opt"][net]["slots"]):
                for k in sa:
                    assert (sa[k] is None and sb[k] is None) or torch.equal(sa[k], sb[k]), (graph, net, k)
