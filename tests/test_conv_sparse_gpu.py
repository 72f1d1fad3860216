"""GPU: every non-Winograd route of tests/conv_routes.py a second time, on the sparse inputs of tests/conv_sparse.py, with one error
bar per output element (derived in that module's docstring, not tuned):

    |got_i - ref_i| <= bar_i = (e0 + n_i 2^-23) A_i + 2^-23 (|ref_i| + |bias| + |prior content|)

and, where no product reaches an element (A_i = 0), the output equal to fp32(bias + prior content) -- for the weight gradient
exactly 0.  Per pass also what tests/test_conv_routes_gpu.py asserts around the result: the return code, the FLOP figure of the
route the table names, guards, pad channels, workspace surroundings and inputs bit for bit, no element left unwritten.  The
weight gradient runs twice: sparse x with dense dy, dense x with sparse dy.  No environment variable is set; every call runs
once.  A failure names the worst element -- (image, row, column, channel) or (tap row, tap column, effective channel, output
channel) -- its error over its bar and the route; `pytest -s` prints the worst error / bar per route.

Worst error / bar per route family, measured on an MI355X (377 passes: the 287 non-Winograd passes of the table, the weight
gradients twice; 261 of them hold elements that no product reaches; none refused, skipped or held to a weaker bar):
  forward          implicit GEMM 0.42 (igemm:W224_x2h, w224_256), K split 0.31, through the upsample 0.31; folded fold4 0.25,
                   fold_percls 0.27; fewout_mfma 0.29, _tile 0.15, _plain 0.19; rgbin_mfma 0.24; dense16 0.24
  input gradient   implicit GEMM .plain 0.27, .act 0.39 (igemm.act:Main16_x2h), .pair 0.24; through pool2_sum_kernel 0.38;
                   folded 0.24; fewin_* 0.23; rgbout_dgrad 0.23; dense16 as the forward
  weight gradient  implicit GEMM 0.11, folded 0.10, upsampled 0.12 (with and without pixel splits); outer1_* 0.09,
                   outer2_* 0.10; dense16 0.09 (one slab) / 0.10 (slabs)
  by engine        two fp16 pieces (_x2h) 0.42, three bf16 pieces (_x3s) 0.27, fp32 scalar loaders 0.23, fp32 _vec 0.25
The fp32 oracle of tests/test_conv_sparse_cpu.py sits at 0.09 at most, the one-piece mutant over the bar on 87 % of the elements
or more.  One case takes 0.1 s on average, the largest under 2 s.
"""
import numpy as np
import pytest
import torch

import conv_routes as R
import conv_sparse as S
from conv_harness import Call
from test_conv_routes_cpu import BIG_ON_PURPOSE

pytestmark = pytest.mark.gpu
PASS = ("fwd", "dgrad", "wgrad")
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from otgan_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    for key in sorted(WORST):
        print("worst %-8s %-30s err/bar %.3f  (%s)" % (key + WORST[key]))


def where(index, shape, which):
    idx = tuple(int(v) for v in np.unravel_index(int(index), shape))
    names = ("tap row", "tap column", "effective channel", "output channel") if which == R.WGRAD else ("image", "row", "column", "channel")
    return ", ".join("%s %d" % nv for nv in zip(names, idx))


def _check(call, case, which, variant, route, dev):
    inp = call.inp
    rc, text, got, flop, launches = call.run(which)
    what = "%s %s (%s sparse)" % (case["name"], PASS[which], inp["sparse"])
    assert rc == R.OK, (what, rc, text)
    want = R.flops(case, which, route)
    assert abs(flop - want) <= 1e-9 * want, (what, route, flop, want)
    b = S.bounds(case, variant, inp, device=dev if case["name"] in BIG_ON_PURPOSE else "cpu")
    shape = tuple(b["ref"].shape)
    worst, at, nwrong, first = S.over_bar(got, b, dev)
    reached = ~b["exact"]
    print("%-44s %-30s err/bar %.3f at (%s)  median n %d  exact elements %d  launches %d"
          % (what, route, worst, where(at, shape, which), int(b["n"][reached].median()) if bool(reached.any()) else 0,
             int(b["exact"].sum()), launches))
    key = (PASS[which], route)
    if worst > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (worst, case["name"])
    g, r, n = (float(t.reshape(-1)[at]) for t in (got, b["ref"], b["n"]))
    assert worst <= 1.0, "%s on %s: error %.3g = %.3f bars at (%s): got %.9g, reference %.9g, n = %d" % (
        what, route, abs(g - r), worst, where(at, shape, which), g, r, n)
    assert nwrong == 0, "%s on %s: %d elements that no product reaches are not bias + prior content, the first at (%s): %.9g" % (
        what, route, nwrong, where(first, shape, which), float(got.reshape(-1)[first]))


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_conv_sparse(dev, case):
    for which in case["passes"]:
        route = case["expect"][which]
        if R.is_error(route) or R.is_wino(route):
            continue
        for variant in S.WHICH_OF_PASS[which]:
            _check(Call(case, dev, S.inputs(case, variant)), case, which, variant, route, dev)
