"""Sparse inputs and element-wise error bars for the table of tests/conv_routes.py.  tests/test_conv_sparse_cpu.py shows that the
bars can be met by a correct fp32 implementation and cannot be met by one that loses the low piece of a split operand;
tests/test_conv_sparse_gpu.py holds every non-Winograd route of the table to them.  No GPU and no library is needed to import
this module.

Why.  tests/test_conv_routes_gpu.py measures one relative L2 error per call on dense randn tensors, against 2e-5.  The split
engines (two scaled fp16 pieces, three bf16 pieces) promise 22 to 24 significand bits; a lost `lo` piece costs 2^-12 of the
products it is lost in and stays under 2e-5 of a dense output when it is lost in less than about 0.7 % of a contraction.  With
few products per output element, and one bar per element, it does not.

Inputs: inputs(case, which), which in WHICH.  The weights, the bias and the prior contents are the dense ones of
conv_routes.inputs.  One operand is sparse: x for "fwd" and "wgrad_x", dy for "dgrad" and "wgrad_dy"; the other activation
operand is the dense one (for "dgrad" x is dense: no x sits on the kink of the activation).  The sparse operand:
  - nonzeros are fp32 normals with random sign and a random 24-bit significand, magnitudes log-uniform in [2^-6, 1] times `amax`;
    one planted element has magnitude `amax` exactly, every other one is strictly smaller;
  - one channel (`zero_channel`) is zero everywhere, where the operand has more than one channel;
  - the corners, the mid-points of the four edges, the first and the last pixel of the first and of the last image hold nonzeros;
  - "fwd" / "dgrad": every weight w[tap, effective channel, output channel] that a dense operand would meet is met by at least
    one nonzero product (outside the zero channel): planted one by one, as near to the centre of image 0 as possible, so that
    the many-product outputs are few.  On a few one-image geometries of 2 x 2 or 4 x 4 pixels this alone gives the median
    element more than MEDIAN_N products; covering nonzeros are then dropped until it does not (`uncovered` counts the
    weights left out; PARTIAL in the CPU test names the cases);
  - "wgrad_x": every output pixel has a nonzero of act(up(x)) in its receptive field; "wgrad_dy": every output pixel has a nonzero
    of dy.  These covering nonzeros lie on a lattice and go to a quarter of the channels (`heavy`), so that the elements of
    the other channels keep few products.  Where the operand has fewer than four usable channels there is no such quarter:
    the lattice is thinned to what LIGHT nonzeros per channel can hold (`lattice_step` > 1), because few products per
    element is what gives the bar its teeth;
  - beyond these, elements are nonzero with a probability chosen for about 8 products per output element.

Bars: bounds(case, which, inp) evaluates the oracle three times in fp64 (conv_routes.oracle_pieces and autograd for `ref`; the
same composition on absolute values and on indicators for `A` and `n`):
    ref_i  the reference, bias and prior content (y_accumulate / accumulate) included;
    A_i    the same pass on |act(up(x))|, |w|, |dy| and |act'(x)|: the sum of the magnitudes of the products of element i;
    n_i    the same pass on the indicators of nonzero: the number of nonzero products of element i;
    bar_i = (e0 + n_i 2^-23) A_i + 2^-23 (|ref_i| + |bias| + |prior content|).

Derivation (u = 2^-24, the unit roundoff of fp32).  A product a w is formed from two operands that each hold at least 22
significand bits: fp32 itself (24), three bf16 pieces (24), or two fp16 pieces of the operand scaled by a power of two so that
its largest magnitude lies in [2^13, 2^14) (11 + 11 bits; both pieces are exact multiples of the fp16 grid as long as the
element is within 2^-17 of the largest, which holds for every nonzero here).  So each operand is off by at most 2^-22
relative, the two together by 2 * 2^-22; the split engines drop the lo * lo term, at most 2^-11 * 2^-11 = 2^-22; rounding
act(x) and act'(x) to fp32 adds u each, the products of pieces are exact in the fp32 accumulator.  Sum: under
3 * 2^-22 + 2 u < 2^-20 = e0 per product.  ELU and CELU go through the device's expm1f / expf, accurate to a few ulp, not
half an ulp: e0 = 2^-19 there.  The n_i nonzero products are added in fp32 in some order (MFMA accumulators, K splits, pixel
slabs, pooled upsampling gradients, workspace folds): every add rounds a partial sum that is at most A_i in magnitude by u,
and there are fewer than 2 n_i of them (n_i - 1 adds, and folds of at most as many partial results): n_i 2^-23 A_i.  Adding the
bias, adding the prior content and storing round the result, at most |ref_i| + |bias| + |prior| in magnitude, by u each: the
last term, with a factor of two to spare.  Zero products add exactly nothing, so dense zeros cost no error and:

Exact elements: where A_i = 0 no product reaches the element, and the output must be fp32(bias + prior content) -- one
rounding, the same in every order; for the weight gradient exactly 0.  (+0 and -0 compare equal.)

The mutant of test (b): hi_piece(t) = fp16(t * 2^(14 - e)) * 2^(e - 14), e = frexp(max |t|), what x2h_scale and x2h_store4 keep
as the `hi` piece.  It is off by up to 2^-11 per element (half an fp16 ulp), 2^-12 to 2^-13 typically: 2^7 to 2^8 times e0.
"""
import math

import numpy as np

import conv_routes as R

WHICH = ("fwd", "dgrad", "wgrad_x", "wgrad_dy")
PASS_OF = {"fwd": R.FWD, "dgrad": R.DGRAD, "wgrad_x": R.WGRAD, "wgrad_dy": R.WGRAD}
SPARSE_OF = {"fwd": "x", "dgrad": "dy", "wgrad_x": "x", "wgrad_dy": "dy"}
WHICH_OF_PASS = {R.FWD: ("fwd",), R.DGRAD: ("dgrad",), R.WGRAD: ("wgrad_x", "wgrad_dy")}
TARGET = 8            # nonzero products per output element the random part aims at
LIGHT = 12            # nonzeros per channel a thinned lattice may add
MEDIAN_N = 32         # the median number of products per element above which covering nonzeros are given up
U23 = 2.0 ** -23

_cache = {}


def e0(case):
    return 2.0 ** -19 if R.act_kind(case["pre"]) == 2 else 2.0 ** -20


# ------------------------------------------------------------------------------------------------------------------
# the effective channels, in the oracle's order (oracle/nets_torch.py apply_pre_activation; a list is concatenated before
# an upsampling layer's activation)
# ------------------------------------------------------------------------------------------------------------------
def eff_channels(case):
    """(src, sgn): source channel and sign of every effective channel"""
    C = sum(case["segs"])
    if not R.doubled(case["pre"]):
        return np.arange(C), np.ones(C, np.int64)
    segs = (C,) if case["up"] else case["segs"]
    src, sgn, off = [], [], 0
    for s in segs:
        src += list(range(off, off + s)) * 2
        sgn += [1] * s + [-1] * s
        off += s
    return np.array(src), np.array(sgn)


def _taps_1d(In, O, K, s, pad):
    """per tap k: the outputs o whose tap k reads inside the input: 0 <= o s + k - pad < In"""
    return [[o for o in range(O) if 0 <= o * s + k - pad < In] for k in range(K)]


def _lattice_1d(In, O, K, s, pad):
    """inputs (coordinates of the upsampled grid) such that every output reads at least one of them"""
    out, o = [], 0
    while o < O:
        r = min(In - 1, o * s - pad + K - 1)
        out.append(r)
        o = (r + pad) // s + 1
    return out


def _value_nonzero(case, v, sgn):
    """whether act(sgn * v) != 0"""
    return sgn * v > 0 if R.act_kind(case["pre"]) == 1 else v != 0


# ------------------------------------------------------------------------------------------------------------------
# the three evaluations
# ------------------------------------------------------------------------------------------------------------------
def _conv(NT, a, W, stride):
    """NT.conv2d_nhwc; one output channel gets a zero filter beside it (conv_routes.oracle: torch's CPU backward)"""
    import torch
    if W.shape[3] == 1:
        return NT.conv2d_nhwc(a, torch.cat([W, torch.zeros_like(W)], 3), stride)[..., :1]
    return NT.conv2d_nhwc(a, W, stride)


def _act(pre):
    import torch.nn.functional as F
    return {0: (lambda t: t), 1: F.relu, 2: F.elu}[R.act_kind(pre)]


def _eff(NT, case, x, mode, jac):
    """the effective activations [N, Hin, Win, Ceff] of x in the oracle's channel order: with jac false their magnitudes
    ("abs") or indicators ("ind"); with jac true a function of x whose Jacobian is |act'| ("abs") or the indicator of
    act' != 0 ("ind")."""
    import torch
    xs = list(torch.split(x, list(case["segs"]), dim=3))
    if case["up"]:
        xs = [NT.upsample2(torch.cat(xs, 3))]
    f, kind = _act(case["pre"]), R.act_kind(case["pre"])
    if jac:
        if mode == "ind" and kind != 1:
            f = lambda t: t                      # act' != 0 everywhere: ELU'(t) = exp(t) > 0
        halves = (lambda t: [f(t), -f(-t)]) if R.doubled(case["pre"]) else (lambda t: [f(t)])      # act' >= 0
    else:
        g = (lambda t: f(t).abs()) if mode == "abs" else (lambda t: (f(t) != 0).to(t.dtype))
        halves = (lambda t: [g(t), g(-t)]) if R.doubled(case["pre"]) else (lambda t: [g(t)])
    return torch.cat([h for t in xs for h in halves(t)], 3)


def _forward(NT, case, x, w, mode, jac):
    """the forward map of one evaluation; "ref" is conv_routes.oracle_pieces itself, with a zero bias"""
    import torch
    if mode != "ref":
        return _conv(NT, _eff(NT, case, x, mode, jac), w, case["stride"])
    Cout = w.shape[3]
    if Cout == 1:
        w = torch.cat([w, torch.zeros_like(w)], 3)       # (conv_routes.oracle: torch's CPU backward with one output channel)
    xs = list(torch.split(x, list(case["segs"]), dim=3))
    zero = torch.zeros(w.shape[3], dtype=w.dtype, device=w.device)
    return R.oracle_pieces(NT, xs, w, zero, R.PRE_NAME[case["pre"]], case["stride"], bool(case["up"]))[..., :Cout]


def evaluate(case, which, inp, mode="ref", dtype=None, device="cpu", replace=None):
    """one pass of the oracle on `inp`: "ref" (conv_routes.oracle_pieces; without bias and prior content), "abs" or "ind".
    `replace`: a tensor to take the place of the sparse operand (the mutant of the CPU test)."""
    import torch
    from oracle import nets_torch as NT
    dtype = dtype or torch.float64
    t = lambda v: v.to(device=device, dtype=dtype, copy=True)
    x, w, dy = t(inp["x"]), t(inp["w"]), t(inp["dy"])
    if replace is not None:
        if SPARSE_OF[which] == "x":
            x = t(replace)
        else:
            dy = t(replace)
    if mode == "abs":
        w, dy = w.abs(), dy.abs()
    elif mode == "ind":
        w, dy = (w != 0).to(dtype), (dy != 0).to(dtype)
    p = PASS_OF[which]
    if p == R.FWD:
        with torch.no_grad():
            return _forward(NT, case, x, w, mode, False)
    if p == R.DGRAD:
        x.requires_grad_(True)
        return torch.autograd.grad(_forward(NT, case, x, w, mode, True), x, dy)[0].detach()
    w.requires_grad_(True)
    return torch.autograd.grad(_forward(NT, case, x, w, mode, False), w, dy)[0].detach()


def extras(case, which, inp):
    """(bias, prior content) of the call as float32 tensors broadcastable to the output, or None"""
    p = PASS_OF[which]
    bias = inp["bias"] if (p == R.FWD and case["bias"]) else None
    prior = inp["y0"] if (p == R.FWD and case["y_acc"]) else (inp["dx0"] if (p == R.DGRAD and case["acc"]) else None)
    return bias, prior


def bounds(case, which, inp, device="cpu"):
    """dict of float64 tensors on `device`, shaped like the output: ref, A, n, bar; `exact` (A == 0) and `expected` (float32:
    what an exact element must hold)"""
    import torch
    ref = evaluate(case, which, inp, "ref", device=device)
    A = evaluate(case, which, inp, "abs", device=device)
    n = evaluate(case, which, inp, "ind", device=device).round()
    bias, prior = extras(case, which, inp)
    extra = torch.zeros((), dtype=torch.float64, device=device)
    expected = torch.zeros(ref.shape, dtype=torch.float32, device=device)
    for v in (bias, prior):
        if v is not None:
            v = v.to(device)
            ref = ref + v.double()
            extra = extra + v.double().abs()
            expected = expected + v               # fp32: one rounding where both are present
    bar = (e0(case) + n * U23) * A + U23 * (ref.abs() + extra)
    return dict(ref=ref, A=A, n=n, bar=bar, exact=A == 0, expected=expected)


def hi_piece(t):
    """the `hi` piece of the two-fp16-piece split: scale 2^(14 - e), e = frexp(max |t|), round to fp16"""
    import torch
    e = math.frexp(float(t.abs().max()))[1]
    s = 2.0 ** (14 - e)
    return ((t * s).to(torch.float16).to(torch.float32) / s).to(t.dtype)


# ------------------------------------------------------------------------------------------------------------------
# the sparse operand
# ------------------------------------------------------------------------------------------------------------------
def _density(case, which, d, g):
    s, up4 = d["stride"], 4 if d["upsample"] else 1
    taps, two = d["KH"] * d["KW"], 2 if d["preact"] == R.ACT_CELU else 1
    if which == "fwd":
        dense = taps * d["C"] * two
    elif which == "dgrad":
        dense = taps * d["Cout"] * two * up4 / (s * s)
    elif which == "wgrad_x":
        dense = d["N"] * d["H"] * d["W"] * up4 / (s * s)
    else:
        dense = d["N"] * g["OH"] * g["OW"]
    return min(1.0, TARGET / max(dense, 1.0))


def _near_centre(rows, cols, Hs, Ws):
    """the pixels rows x cols, nearest to the centre of the image first"""
    px = [(r, c) for r in rows for c in cols]
    px.sort(key=lambda p: ((p[0] - (Hs - 1) / 2) ** 2 + (p[1] - (Ws - 1) / 2) ** 2, p))
    return px


def _wgrad_counts(case, a_ind, dy_ind):
    """[KH, KW, Ceff, Cout] counts of (pixel, tap) pairs at which both indicators are nonzero"""
    import torch
    from oracle import nets_torch as NT
    W = torch.zeros(case["KH"], case["KW"], a_ind.shape[3], dy_ind.shape[3], dtype=torch.float64, requires_grad=True)
    y = _conv(NT, a_ind, W, case["stride"])
    return torch.autograd.grad(y, W, dy_ind)[0].detach().round()


def _cover_fwd(case, d, g, val, usable, rng, draw, budget):
    """plant x so that every (tap, effective channel) a dense x would meet is met, nearest to the centre of image 0 first (one
    nonzero there serves every tap that reads the pixel); at most `budget` nonzeros -> (planted, left uncovered)"""
    src, sgn = eff_channels(case)
    s, up = d["stride"], d["upsample"]
    th = _taps_1d(g["Hin"], g["OH"], d["KH"], s, g["pad_t"])
    tw = _taps_1d(g["Win"], g["OW"], d["KW"], s, g["pad_l"])
    relu = R.act_kind(case["pre"]) == 1
    rows = [sorted({(o * s + kh - g["pad_t"]) >> up for o in th[kh]}) for kh in range(d["KH"])]
    cols = [sorted({(o * s + kw - g["pad_l"]) >> up for o in tw[kw]}) for kw in range(d["KW"])]
    cand, missing = {}, []
    for kh in range(d["KH"]):
        for kw in range(d["KW"]):
            px = _near_centre(rows[kh], cols[kw], d["H"], d["W"])
            if not px:
                continue
            cand[kh, kw] = px
            rr, cc = np.array([p[0] for p in px]), np.array([p[1] for p in px])
            for ce in range(len(src)):
                if src[ce] in usable and not _value_nonzero(case, val[:, rr, cc, src[ce]], sgn[ce]).any():
                    missing.append((kh, kw, ce))
    order = rng.permutation(len(missing))
    covered, planted, left = set(), 0, 0
    for i in order:
        kh, kw, ce = missing[i]
        if (kh, kw, ce) in covered:
            continue
        free = [p for p in cand[kh, kw] if val[0, p[0], p[1], src[ce]] == 0]
        if planted >= budget or not free:
            left += 1
            continue
        r, c = free[0]
        val[0, r, c, src[ce]] = draw() * (sgn[ce] if relu else rng.choice((-1.0, 1.0)))
        planted += 1
        both = [ce] if relu else [e for e in range(len(src)) if src[e] == src[ce]]      # ELU(t) and ELU(-t) are both nonzero
        covered.update((a, b, e) for a in range(d["KH"]) if r in rows[a] for b in range(d["KW"]) if c in cols[b] for e in both)
    return planted, left * d["Cout"]


def _cover_dgrad(case, d, g, val, usable, inp_x, rng, draw, budget):
    """plant dy so that every (tap, effective channel, output channel) a dense dy would meet is met: a dy element at output o
    meets w[tap, ceff, cout] where act'(x) != 0 at the pixel o s + tap - pad of effective channel ceff.  Nearest to the centre
    of image 0 first; at most `budget` nonzeros -> (planted, left uncovered)"""
    import torch
    from oracle import nets_torch as NT
    with torch.no_grad():
        jac = _eff(NT, case, inp_x.double(), "ind", False)      # relu-type: act'(t) != 0 exactly where act(t) != 0
    if R.act_kind(case["pre"]) != 1:
        jac = torch.ones_like(jac)                              # otherwise act' != 0 everywhere
    s = d["stride"]
    th = _taps_1d(g["Hin"], g["OH"], d["KH"], s, g["pad_t"])
    tw = _taps_1d(g["Win"], g["OW"], d["KW"], s, g["pad_l"])
    ths, tws = [set(t) for t in th], [set(t) for t in tw]
    dense = _wgrad_counts(case, jac, torch.ones(d["N"], g["OH"], g["OW"], d["Cout"], dtype=torch.float64)) > 0
    cover = _wgrad_counts(case, jac, torch.from_numpy((val != 0).astype(np.float64)))
    missing = ((cover == 0) & dense).numpy()
    missing[..., [c for c in range(d["Cout"]) if c not in usable]] = False
    jn = jac.numpy() != 0
    cand = {}
    for kh in range(d["KH"]):
        for kw in range(d["KW"]):
            px = _near_centre(th[kh], tw[kw], g["OH"], g["OW"])
            oh, ow = np.array([p[0] for p in px], np.int64), np.array([p[1] for p in px], np.int64)
            cand[kh, kw] = (oh, ow, oh * s + kh - g["pad_t"], ow * s + kw - g["pad_l"])
    planted = 0
    keys = sorted({(a, b, c) for a, b, _, c in zip(*np.nonzero(missing))})
    for i in rng.permutation(len(keys)):
        kh, kw, co = keys[i]
        oh, ow, ih, iw = cand[kh, kw]
        while missing[kh, kw, :, co].any() and planted < budget:
            ce = int(np.flatnonzero(missing[kh, kw, :, co])[0])
            hit = np.argwhere(jn[:, ih, iw, ce] & (val[:, oh, ow, co] == 0))          # [N, candidates]
            if not len(hit):
                break
            n, j = hit[0]
            val[n, oh[j], ow[j], co] = draw() * rng.choice((-1.0, 1.0))
            planted += 1
            for a in range(d["KH"]):
                for b in range(d["KW"]):
                    if oh[j] in ths[a] and ow[j] in tws[b]:
                        missing[a, b, :, co] &= ~jn[n, oh[j] * s + a - g["pad_t"], ow[j] * s + b - g["pad_l"], :]
    return planted, int(missing.sum())


def _cover_wgrad(case, which, d, g, val, usable, rng, draw):
    """lattice nonzeros so that every output pixel meets a nonzero; -> lattice step (1: the whole lattice)"""
    s, up = d["stride"], d["upsample"]
    if which == "wgrad_x":
        rows = sorted({r >> up for r in _lattice_1d(g["Hin"], g["OH"], d["KH"], s, g["pad_t"])})
        cols = sorted({c >> up for c in _lattice_1d(g["Win"], g["OW"], d["KW"], s, g["pad_l"])})
    else:
        rows, cols = range(g["OH"]), range(g["OW"])
    pts = [(n, r, c) for n in range(d["N"]) for r in rows for c in cols]
    usable = sorted(usable)
    heavy = usable[:len(usable) // 4]
    step = 1
    if not heavy:
        heavy = usable
        step = max(1, -(-len(pts) // (LIGHT * len(usable))))
        pts = pts[::step]
    positive = which == "wgrad_x" and case["pre"] == R.ACT_RELU
    for i, (n, r, c) in enumerate(pts):
        ch = heavy[i % len(heavy)]
        if val[n, r, c, ch] == 0 or (positive and val[n, r, c, ch] < 0):
            val[n, r, c, ch] = draw() * (1.0 if positive else rng.choice((-1.0, 1.0)))
    return step, heavy if step == 1 else []


def inputs(case, which):
    """conv_routes.inputs(case) with the sparse operand of `which` in place of the dense one, and: `sparse` (its key), `amax`,
    `zero_channel` (or None), `lattice_step`, `heavy` (channels that carry the weight gradient's covering lattice)"""
    import torch
    key = (R.base_name(case), which)
    if key in _cache:
        return _cache[key]
    d = R.desc_fields(case)
    g = R.make_geo(d)
    dense = R.inputs(case)
    name = SPARSE_OF[which]
    shape = tuple(dense[name].shape)
    N, Hs, Ws, Cs = shape
    seed = R.seed_of(R.base_name(case) + which) % (2 ** 32)
    gen = [np.random.RandomState(seed)]
    amax = float(np.float32(2.0 + 2.0 * gen[0].random_sample()))
    below = float(np.nextafter(np.float32(amax), np.float32(0)))

    def draw(size=None):
        """magnitudes log-uniform in [2^-6, 1) amax, rounded to fp32 (a random 24-bit significand), strictly below amax"""
        m = np.minimum(np.asarray(amax * 2.0 ** (-6.0 * gen[0].random_sample(size))).astype(np.float32), np.float32(below))
        return m.astype(np.float64) if size is not None else float(m)

    rng = gen[0]
    zero_channel = int(rng.randint(Cs)) if Cs > 1 else None
    usable = set(range(Cs)) - {zero_channel}
    mask = rng.random_sample(shape) < _density(case, which, d, g)
    base = np.where(mask, draw(shape) * rng.choice((-1.0, 1.0), size=shape), 0.0)
    if zero_channel is not None:
        base[..., zero_channel] = 0.0
    chans = sorted(usable)
    for n in sorted({0, N - 1}):
        for r, c in ((0, 0), (0, Ws - 1), (Hs - 1, 0), (Hs - 1, Ws - 1), (0, Ws // 2), (Hs - 1, Ws // 2), (Hs // 2, 0), (Hs // 2, Ws - 1)):
            if not base[n, r, c].any():
                base[n, r, c, chans[rng.randint(len(chans))]] = draw() * rng.choice((-1.0, 1.0))
    step, heavy, left, budget = 1, [], 0, 1 << 40
    while True:
        # (the covering nonzeros are drawn from a generator of their own, so that a second attempt repeats the first)
        rng = gen[0] = np.random.RandomState((seed + 1) % (2 ** 32))
        val = base.copy()
        if which == "fwd":
            planted, left = _cover_fwd(case, d, g, val, usable, rng, draw, budget)
        elif which == "dgrad":
            planted, left = _cover_dgrad(case, d, g, val, usable, dense["x"], rng, draw, budget)
        else:
            step, heavy = _cover_wgrad(case, which, d, g, val, usable, rng, draw)
            break
        # few products per element come first: where covering every weight leaves the median element with more than
        # MEDIAN_N products (small images with many channels), a quarter of the covering nonzeros go, and again
        n = evaluate(case, which, dict(dense, **{name: torch.from_numpy(val)}), "ind")
        if planted == 0 or float(n[n > 0].median()) <= MEDIAN_N:
            break
        budget = planted * 3 // 4
    nz = np.argwhere(val != 0)
    at = tuple(nz[rng.randint(len(nz))])
    val[at] = math.copysign(amax, val[at])
    out = dict(dense)
    out[name] = torch.from_numpy(val.astype(np.float32))
    assert (out[name].double().numpy() == val).all()
    out.update(sparse=name, amax=amax, zero_channel=zero_channel, lattice_step=step, heavy=heavy, uncovered=left)
    _cache[key] = out
    return out


def sparse_tensor(shape, seed, density):
    """a float32 tensor [..., C] with the values of the sparse operands above and no covering nonzeros: each element nonzero
    with probability `density`, random sign, magnitude log-uniform in [2^-6, 1) amax, one planted element of magnitude amax, the
    first and the last pixel nonzero, channel seed % C zero everywhere -> (tensor, amax)"""
    import torch
    rng = np.random.RandomState(seed % (2 ** 32))
    amax = float(np.float32(2.0 + 2.0 * rng.random_sample()))
    below = np.float32(np.nextafter(np.float32(amax), np.float32(0)))
    mag = np.minimum((amax * 2.0 ** (-6.0 * rng.random_sample(shape))).astype(np.float32), below)
    val = np.where(rng.random_sample(shape) < density, mag * rng.choice((-1.0, 1.0), size=shape).astype(np.float32), np.float32(0))
    flat = val.reshape(-1, shape[-1])
    zero = seed % shape[-1]
    for row in (0, len(flat) - 1):
        flat[row, (zero + 1) % shape[-1]] = mag.reshape(-1, shape[-1])[row, 0]
    flat[:, zero] = 0
    nz = np.flatnonzero(flat)
    at = nz[rng.randint(len(nz))]
    flat.reshape(-1)[at] = math.copysign(amax, flat.reshape(-1)[at])
    return torch.from_numpy(val.astype(np.float32)), amax


def over_bar(got, b, device):
    """(worst |got - ref| / bar over the elements any product reaches, its flat index, the number of exact elements that are not
    what they must be, the flat index of the first) of a result against bounds(); a NaN counts as infinitely wrong"""
    import torch
    flat = lambda t: t.reshape(-1).to(device)
    got = got.reshape(-1).to(device).double()
    assert got.numel() == b["ref"].numel(), (got.numel(), tuple(b["ref"].shape))
    err, bar, exact = (got - flat(b["ref"])).abs(), flat(b["bar"]), flat(b["exact"])
    ratio = torch.where(exact, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    wrong = exact & ~(got == flat(b["expected"]).double())
    first = int(wrong.nonzero()[0]) if bool(wrong.any()) else -1
    return float(ratio.max()), int(ratio.argmax()), int(wrong.sum()), first
