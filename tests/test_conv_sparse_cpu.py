"""CPU: the sparse inputs and the element-wise bars of tests/conv_sparse.py, for every geometry of the table of tests/conv_routes.py
and every pass some case runs on it (the weight gradient in both variants):
  (a) the oracle evaluated in float32 meets the bar at every element: a correct fp32 implementation can pass;
  (b) the oracle with the sparse operand replaced by its `hi` fp16 piece (conv_sparse.hi_piece: a lost `lo` piece) violates the
      bar on at least half of the elements that any product reaches: the bar has teeth;
  (c) the sparse operand is what the module says it is: values, the zero channel, corners and edges, and every weight
      (forward, input gradient) / every output pixel (weight gradient) met by a nonzero;
  (d) the median number of nonzero products over the elements that any product reaches is at most 32.
Measured here: (a) at most 0.09 of the bar, (b) 0.87 to 1.00 of the elements, (d) medians of 1 to 32.

Where (c) and (d) cannot both hold, (d) wins, because few products per element are what (b) needs:
  - PARTIAL: one image of 2 x 2 or 4 x 4 pixels with many channels.  Every output element reads most of the image, so one nonzero
    per weight already gives every element more than 32 products; covering nonzeros are dropped until the median is 32.
  - a weight gradient whose sparse operand has fewer than four usable channels (the few-channel kernels: RGB in, RGB out, one
    to four outputs): a nonzero at every output pixel would put hundreds of products into every element, so the covering
    lattice is thinned (lattice_step > 1) to 12 nonzeros per channel, first and last lattice point included."""
import numpy as np
import pytest
import torch

import conv_routes as R
import conv_sparse as S

_GEOMETRIES = {}
for _case in R.CASES:
    _GEOMETRIES.setdefault(R.base_name(_case), [_case, set()])[1].update(_case["passes"])

# (geometry, pass): weights left without a nonzero product, and why
PARTIAL = {
    ("p0_igemm_n16_vec", "fwd"): "1 x 2 x 2 x 32, ReLU, 3 x 3 taps: each tap reads one pixel at one output, every output reads all four",
    ("p1_fold_act_main16_scalar", "dgrad"): "dy 1 x 4 x 4 x 40 into 1 x 2 x 2 x 48: every dx element pools most of dy",
    ("p1_igemm_pool_pair_small16_x2h", "dgrad"): "dy 1 x 2 x 2 x 160 into 1 x 2 x 2 x 4 through a 1 x 1 filter: 160 weights per pixel",
}


def _weights_met(case, which, inp):
    """[KH, KW, Ceff, Cout] bool: (the weights that meet a nonzero product with this input, those a dense operand would meet)"""
    if which == "fwd":
        ones = torch.ones_like(inp["dy"])
        met = S.evaluate(case, "wgrad_x", dict(inp, dy=ones), "ind") > 0
        dense = sum(S.evaluate(case, "wgrad_x", dict(inp, dy=ones, x=sign * torch.ones_like(inp["x"])), "ind") for sign in (1.0, -1.0)) > 0
    else:
        met = S.evaluate(case, "wgrad_dy", inp, "ind") > 0
        dense = S.evaluate(case, "wgrad_dy", dict(inp, dy=torch.ones_like(inp["dy"])), "ind") > 0
    return met, dense


def _check_operand(case, which, inp):
    name = inp["sparse"]
    t = inp[name]
    N, Hs, Ws, Cs = t.shape
    nz = t[t != 0].double().abs()
    assert t.dtype == torch.float32 and torch.isfinite(t).all()
    assert float(nz.max()) == inp["amax"] and int((nz == inp["amax"]).sum()) == 1            # one planted largest element
    assert float(nz.min()) >= inp["amax"] * 2.0 ** -6 * (1 - 2.0 ** -23)                    # normals within 2^-6 of it
    assert float(nz.min()) > 2.0 ** -126
    if nz.numel() >= 64:
        low = np.frexp(nz.numpy())[0] * 2.0 ** 24 % 256                                      # the low significand bits are in use
        assert len(np.unique(low)) > 16
        assert bool((t > 0).any()) and bool((t < 0).any())
    z = inp["zero_channel"]
    assert (z is None) == (Cs == 1)
    if z is not None:
        assert not bool(t[..., z].any())
    for n in {0, N - 1}:
        for r, c in ((0, 0), (0, Ws - 1), (Hs - 1, 0), (Hs - 1, Ws - 1), (0, Ws // 2), (Hs - 1, Ws // 2), (Hs // 2, 0), (Hs // 2, Ws - 1)):
            assert bool(t[n, r, c].any()), (case["name"], which, n, r, c)
    # the other operands are the dense ones of the table
    for k in ("x", "dy", "w", "bias", "y0", "dx0"):
        if k != name and R.inputs(case)[k] is not None:
            assert inp[k] is R.inputs(case)[k]
    usable = Cs - (z is not None)
    if which in ("fwd", "dgrad"):
        met, dense = _weights_met(case, which, inp)
        if z is not None:
            if which == "fwd":
                dense[:, :, torch.from_numpy(S.eff_channels(case)[0] == z)] = False
            else:
                dense[..., z] = False
        missing = int((dense & ~met).sum())
        assert missing == inp["uncovered"], (case["name"], which, missing, inp["uncovered"])
        assert (missing > 0) == ((case["name"], which) in PARTIAL), (case["name"], which, missing)
        assert missing < int(dense.sum())
    else:
        if which == "wgrad_x":
            reached = S.evaluate(case, "fwd", inp, "ind").sum(-1) > 0                      # a nonzero of act(up(x)) under some tap
        else:
            reached = (inp["dy"] != 0).any(-1)
        if inp["lattice_step"] == 1:
            assert bool(reached.all()), (case["name"], which, int((~reached).sum()))
            assert usable < 4 or (4 * len(inp["heavy"]) <= usable and len(inp["heavy"]) >= 1)
        else:
            assert usable < 4, (case["name"], which, usable)
            assert bool(reached.reshape(-1)[0]) and bool(reached.any())


@pytest.mark.parametrize("case,passes", list(_GEOMETRIES.values()), ids=[c["name"] for c, _ in _GEOMETRIES.values()])
def test_sparse_inputs_and_bars(case, passes):
    for which in S.WHICH:
        if S.PASS_OF[which] not in passes:
            continue
        inp = S.inputs(case, which)
        assert S.inputs(case, which) is inp
        b = S.bounds(case, which, inp)
        reached = ~b["exact"]
        assert bool(reached.any()) and bool((b["n"][reached] >= 1).all()) and bool((b["n"][b["exact"]] == 0).all())
        bias, prior = S.extras(case, which, inp)
        add = sum(v.double() for v in (bias, prior) if v is not None)
        # (a)
        low = S.evaluate(case, which, inp, "ref", dtype=torch.float32)
        for v in (bias, prior):
            if v is not None:
                low = low + v
        ra = float(((low.double() - b["ref"]).abs() / b["bar"].clamp_min(1e-300)).max())
        assert bool(((low.double() - b["ref"]).abs() <= b["bar"]).all()), (case["name"], which, ra)
        assert torch.equal(low[b["exact"]], b["expected"][b["exact"]])
        # (b)
        mutant = S.evaluate(case, which, inp, "ref", replace=S.hi_piece(inp[inp["sparse"]])) + add
        over = float(((mutant - b["ref"]).abs() > b["bar"])[reached].double().mean())
        # (d)
        med = float(b["n"][reached].median())
        print("%-36s %-8s fp32 at %.2f bars, mutant over the bar on %.3f, median n %d, exact elements %d"
              % (case["name"], which, ra, over, med, int(b["exact"].sum())))
        assert over >= 0.5, (case["name"], which, over)
        assert med <= 32, (case["name"], which, med)
        # (c)
        _check_operand(case, which, inp)


def test_the_hi_piece_is_what_the_split_keeps():
    """hi_piece against the definition: the largest magnitude scaled into [2^13, 2^14), 11 significand bits kept, off by at most
    2^-11 relative (half an fp16 ulp) and by more than 2^-14 on most elements"""
    t = S.inputs(R.BY_NAME["growth16_relu"], "fwd")["x"]
    hi = S.hi_piece(t)
    e = np.frexp(float(t.abs().max()))[1]
    scaled = hi.double() * 2.0 ** (14 - e)
    assert 2.0 ** 13 <= float(scaled.abs().max()) < 2.0 ** 14
    nz = t != 0
    assert bool((hi[~nz] == 0).all())
    m = np.frexp(scaled[nz].numpy())[0] * 2.0 ** 11
    assert (m == np.round(m)).all()
    rel = ((hi.double() - t.double()).abs() / t.double().abs())[nz]
    assert float(rel.max()) <= 2.0 ** -11 and float((rel > 2.0 ** -14).double().mean()) > 0.5
