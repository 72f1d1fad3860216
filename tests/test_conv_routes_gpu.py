"""GPU: the three convolution passes on every kernel route of csrc/conv.hip, through the C ABI (otgan_conv2d_fwd_pf_f32,
otgan_conv2d_dgrad_pf_f32, otgan_conv2d_wgrad_f32; otgan_conv2d_fold_weights_f32 and otgan_conv2d_prepare_filters_f32 where the
contract needs them): the calls of tests/conv_routes.py -- misaligned pointers, pitches that are no multiple of 4, y_coff > 0,
lddx > C, accumulate, short and null workspaces, channel maps, `filters`, x_operand, filters that are neither 3x3 nor 5x5, the
few-channel kernels off the models' shapes, both sides of every tile-count threshold -- against the fp64 oracle on the fp32
inputs (oracle/nets_torch.py).

Per call: the return code, and for a refused call the fragment of otgan_last_error() and every output bit for bit untouched
(then the same call without the offending property must succeed); y / dx / dw to TOL = 2e-5 relative L2 (the bar of
tests/test_layers_gpu.py, not loosened per route), with `accumulate` / `y_accumulate` against prior content + result; guard
floats, the pad channels [C, lddx) of dx, the channels of y outside [y_coff, y_coff + Cout), the workspace in front of the
pointer and beyond workspace_bytes, and every input buffer unchanged bit for bit; no valid element left unwritten; the FLOP
the pass reports to the profiler (otgan_prof_*) equal to the restated formula of the route the table names.  The route twins
of conv_routes.TWINS are ordinary table cases: each side meets the bound against the oracle on its own.

No environment variable is set here; every call runs once.
"""
import ctypes

import pytest
import torch

import conv_routes as R
from conv_harness import Call, Flat, Pitched, Workspace, _cdesc

pytestmark = pytest.mark.gpu
TOL = 2e-5               # tests/test_layers_gpu.py
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from otgan_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    for key in sorted(WORST):
        print("worst %-16s %-28s %.2e  (%s)" % (key + (WORST[key][0], WORST[key][1])))


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def _reference(case, which):
    ref, inp, d = R.reference(case), R.inputs(case), R.desc_fields(case)
    if which == 0:
        r = ref["y"].reshape(-1, d["Cout"])
        return r + inp["y0"].double().reshape(-1, d["Cout"]) if case["y_acc"] else r
    if which == 1:
        r = ref["dx"].reshape(-1, d["C"])
        return r + inp["dx0"].double().reshape(-1, d["C"]) if case["acc"] else r
    return ref["dw"].reshape(1, -1)


def _route_from_library(call, which):
    """expected_route with dense16_tiling and the operand decision taken from the library's host queries (bases of refused
    calls that are not table cases themselves)"""
    L = call.L
    query = lambda f, w: int(L.otgan_conv2d_workspace_bytes(ctypes.byref(_cdesc(f)), w))
    d16 = R.dense16_of(query, call.fields, call.geo, lambda f: bool(L.otgan_dense16_h2_ok(ctypes.byref(_cdesc(f)))))
    assert d16[0] is not None
    return R.expected_route(call.case, which, d16, int(L.otgan_conv2d_operand_bytes(ctypes.byref(call.desc))) > 0)


def _succeeds(call, which, route):
    case = call.case
    rc, text, got, flop, launches = call.run(which)
    what = "%s %s" % (case["name"], ("fwd", "dgrad", "wgrad")[which])
    assert rc == R.OK, (what, rc, text)
    e = _rel(got, _reference(case, which))
    want = R.flops(case, which, route)       # (dense16_tiling changes no FLOP figure: both plans report 2 M taps Ceff Cout)
    print("%-34s %-30s rel %.2e  FLOP %.6g (restated %.6g)  launches %d" % (what, route, e, flop, want, launches))
    key = (("fwd", "dgrad", "wgrad")[which], route)
    if e > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (e, case["name"])
    assert e < TOL, (what, route, e)
    assert abs(flop - want) <= 1e-9 * want, (what, route, flop, want)


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_conv_route(dev, case):
    call = Call(case, dev)
    base_call = None
    for which in case["passes"]:
        route = case["expect"][which]
        if not R.is_error(route):
            _succeeds(call, which, route)
            continue
        rc, text, got, flop, launches = call.run(which)
        what = "%s %s" % (case["name"], ("fwd", "dgrad", "wgrad")[which])
        print("%-34s refused: %d %s" % (what, rc, text))
        assert rc == route[0] and route[1] in text, (what, rc, text, route)
        # the same call without the one offending property succeeds on the route the table names for it
        base = case["base"]
        base_call = base_call or Call(base, dev)
        base_route = base["expect"][which] if which in base["expect"] else _route_from_library(base_call, which)
        assert not R.is_error(base_route), (what, base_route)
        _succeeds(base_call, which, base_route)
