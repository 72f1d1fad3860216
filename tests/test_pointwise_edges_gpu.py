"""GPU: edge shapes and exactness of the memory-bound kernels -- csrc/pointwise.hip, the absmax reduction of
csrc/winograd.hip, the batched copies -- against tests/pointwise_ref.py (fp64 restatements, bit-exact float32 emulations
of the optimisers; tests/test_pointwise_ref_cpu.py shows that each comparison used here fires on a subtly wrong
implementation).  Integer-valued inputs make reductions exact (`==`), planted extrema make the amax records exact, every
kernel writes into a guarded buffer and reads from buffers whose pitch columns and surroundings are NaN.

Worst |err| / (tol * scale) measured on an MI355X, tol = 1e-6 per element against fp64 with the scale named in each test
(the table of DESIGN.md section 4; no tolerance had to be widened):

    kernel                                               float4 / batched    scalar / per layer
    column sums, GLU-backward column sums (integers)     bit-equal           bit-equal
    column sums, random (tol = L 2^-24, scale sum |a|)   0.00057             0.00047
    GLU-backward column sums, random (same bound)        0.0019              -
    absmax and every producer's amax record              == max |t|          == max |t|
    weight norm forward   w / inv_norm / wT              0.21 / 0.10 / -     0.21 / 0.12 / bit-equal
    weight norm backward  dV / dg                        0.052 / 0.11        0.15 / 0.097
    GLU forward                                          0.17                0.18
    GLU backward          da / dl                        0.17 / 0.26         0.17 / 0.25
    tanh forward / backward                              -                   0.14 / 0.15
    feature head forward  f / norm                       0.11 / 0.051        0.10 / 0.049
    feature head backward                                0.56                0.18
    Adam (+ EMA), Adam over gathered gradients, Adamax,
      Nesterov: p, v, mg, shadow over three steps        -                   bit-equal to the float32 emulation
    copy2d_batched, gather3d_batched                     -                   bit-equal

Adamax and Nesterov were NOT bit-equal before this file existed: the compiler had contracted `mom2 * mg + 1e-8f`, `p - lr * q`,
one product of `mom1 * v + om1 * g` (Adamax) and `mom1 * vo - lr * g`, `p - mom1 * vo`, `... + opm * vn` (Nesterov) into fused
multiply-adds (read in the kernels' ISA, not found by re-running); the kernels now carry the same `fp contract(off)` as adam_elem.

Wall time of the file on an MI355X: 6.6 s, measured for 170 of its 174 tests (the slowest, the 8.4 M-element GLU wrap case,
0.8 s); the four two-segment gathered-Adam cases came later and are the size of the 4.2 M-element Adam cases (0.2 s each)."""
import ctypes

import numpy as np
import pytest
import torch

import pointwise_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-6
WORST = {}          # kernel -> worst ratio seen in this run (printed: the table above is filled from it)


def _lib():
    from otgan_amd import _lib as m
    m.lib()
    return m


def _L():
    return _lib().lib()


def _sp():
    return _lib().stream_ptr()


def _dev():
    _lib()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _out(shape, pitch=None, lead=0):
    return R.guarded(shape, pitch=pitch, lead=lead, device=_dev())


def _inp(data, pitch=None, lead=0):
    """`data` (a CPU tensor) inside a device buffer that is NaN everywhere else."""
    g = R.guarded(tuple(data.shape), pitch=pitch, lead=lead, device=_dev(), bits=R.POISON_BITS)
    g.view.copy_(data)
    return g


def _record(fill=0.0, n=1):
    g = _out((n, R.AMAX_RECORD_FLOATS) if n > 1 else (R.AMAX_RECORD_FLOATS,))
    g.view.fill_(fill)
    return g


def _ok(rc, what=""):
    assert rc == 0, (what, rc, _L().otgan_last_error().decode("utf-8", "replace"))


def _refused(rc):
    assert rc == -1, rc          # OTGAN_ERR_INVALID, returned before any launch


def _close(name, got, ref, scale, tol=TOL):
    r = R.assert_close_elementwise(got, ref, scale, tol, name)
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"RATIO {name} {r:.3g}")
    return r


def _same_value(got, ref, what=""):
    """Record against the exact maximum: equal, or both NaN."""
    assert (np.isnan(got) and np.isnan(ref)) or got == ref, (what, got, ref)


def _intact(*gs):
    for i, g in enumerate(gs):
        R.assert_guards_intact(g, f"buffer {i}")


# =============================================================================================== column sums
COLSUM_CASES = [(1, 4, 4, 0), (15, 64, 64, 0), (16, 64, 64, 0), (17, 68, 68, 0),
                (64, 4, 4, 0), (65, 4, 4, 0),             # one row chunk, then two
                (16385, 8, 8, 0),                         # 256 chunks of 65 rows: the last three are empty
                (100, 36, 52, 8),                         # columns 8 .. 43 of a 52-wide NaN-filled buffer
                (33, 3, 3, 0), (70, 66, 67, 0), (40, 8, 8, 1)]      # scalar kernel: C % 4, lda % 4, a misaligned base


def _colsum(a, rows, cols, lda):
    out, scratch = _out((cols,)), _out((256 * cols,))
    _ok(_L().otgan_colsum_f32(a.view.data_ptr(), rows, cols, lda, out.view.data_ptr(), scratch.view.data_ptr(), _sp()), "colsum")
    torch.cuda.synchronize()
    _intact(out, scratch, a)
    return out.view.cpu()


@pytest.mark.parametrize("rows,cols,lda,lead", COLSUM_CASES)
def test_colsum_of_integers_is_exact(rows, cols, lda, lead):
    a = R.int_valued((rows, cols), -8, 8, _gen(rows * 131 + cols))
    a[-1] = (torch.arange(cols) % 8 + 1).float()          # (a last row of zeros would hide a dropped row)
    g = _inp(a, pitch=lda, lead=lead)
    assert (g.view.data_ptr() % 16 != 0) == (lead % 4 != 0)
    got = _colsum(g, rows, cols, lda)
    R.assert_bits_equal(got, R.colsum_exact(a).astype(np.float32), f"colsum {rows}x{cols} lda {lda}")


@pytest.mark.parametrize("rows,cols,vec", [(16385, 8, True), (16385, 3, False)])
def test_colsum_of_random_data(rows, cols, vec):
    """|err| <= L * 2^-24 * sum |a| per column, L the longest sequential addition chain of the launch."""
    a = torch.randn(rows, cols, generator=_gen(7))
    got = _colsum(_inp(a), rows, cols, cols)
    L = R.colsum_chain_length(rows, cols, vec)
    _close("colsum (random)", got, a.double().sum(0), a.double().abs().sum(0), tol=L * 2.0 ** -24)


@pytest.mark.parametrize("rows", [1, 17, 65, 16385])
@pytest.mark.parametrize("C", [4, 36, 68])
def test_glu_backward_column_sums_are_exact(rows, C):
    """dy integer, gates 0 (s = 1/2 exactly), a an even integer: da = dy / 2 and dl = dy * a / 4 are exact, and so are the
    column sums of both halves (tests/test_pointwise_ref_cpu.py: below 2^24 units)."""
    g = _gen(rows * 7 + C)
    x = torch.zeros(rows, 2 * C)
    x[:, :C] = 2 * R.int_valued((rows, C), -4, 4, g)
    dy = R.int_valued((rows, C), -8, 8, g)
    dy[-1] = (torch.arange(C) % 8 + 1).float()
    x[-1, :C] = 2.0
    gx, gdy = _inp(x), _inp(dy)
    dx, rec, cs, scratch = _out((rows, 2 * C)), _record(), _out((2 * C,)), _out((256 * 2 * C,))
    _ok(_L().otgan_glu_bwd_colsum_f32(gx.view.data_ptr(), gdy.view.data_ptr(), rows, C, dx.view.data_ptr(), rec.view.data_ptr(),
                                      cs.view.data_ptr(), scratch.view.data_ptr(), _sp()), "glu bwd colsum")
    torch.cuda.synchronize()
    _intact(dx, rec, cs, scratch, gx, gdy)
    want = torch.cat([dy * 0.5, dy * x[:, :C] * 0.5 * 0.5], 1)
    R.assert_bits_equal(dx.view, want, "dx")
    R.assert_bits_equal(cs.view, want.double().sum(0).float(), "column sums")
    _same_value(R.record_value(rec.view), R.amax_exact(want), "record")


def test_glu_backward_column_sums_of_random_data():
    rows, C = 16385, 36
    g = _gen(11)
    x = torch.cat([torch.randn(rows, C, generator=g) * 3, torch.rand(rows, C, generator=g) * 24 - 12], 1)
    dy = torch.randn(rows, C, generator=g)
    gx, gdy = _inp(x), _inp(dy)
    dx, rec, cs, scratch = _out((rows, 2 * C)), _record(), _out((2 * C,)), _out((256 * 2 * C,))
    _ok(_L().otgan_glu_bwd_colsum_f32(gx.view.data_ptr(), gdy.view.data_ptr(), rows, C, dx.view.data_ptr(), rec.view.data_ptr(),
                                      cs.view.data_ptr(), scratch.view.data_ptr(), _sp()), "glu bwd colsum")
    torch.cuda.synchronize()
    _intact(dx, rec, cs, scratch)
    wrote = dx.view.cpu().double()                          # the sums are of what the kernel wrote
    L = R.colsum_chain_length(rows, C, True)
    _close("glu bwd column sums (random)", cs.view, wrote.sum(0), wrote.abs().sum(0), tol=L * 2.0 ** -24)
    _same_value(R.record_value(rec.view), R.amax_exact(dx.view), "record")
    ref = R.glu_bwd(x, dy)
    s = torch.sigmoid(x[:, C:].double())
    scale = torch.cat([ref[:, :C].abs(), (dy.double() * x[:, :C].double() * s).abs()], 1)
    _close("glu bwd (+ column sums) dx", dx.view, ref, scale)


# =============================================================================================== absmax
ABSMAX_SHAPES = [(1, 4, 4), (1, 1028, 1028), (3, 4, 12), (7, 36, 52),
                 (8197, 256, 256)]        # 524 608 quads: every thread takes the 8-way loop once, 320 threads a tail quad


def _absmax(ptr, rows, C, ld, rec_ptr):
    return _L().otgan_absmax_f32(ptr, rows, C, ld, rec_ptr, _sp())


def _absmax_value(g, rows, C, ld):
    rec = _record(fill=123.0)               # the kernel writes all 16 sub-slots: nothing of the fill may count
    _ok(_absmax(g.view.data_ptr(), rows, C, ld, rec.view.data_ptr()), "absmax")
    torch.cuda.synchronize()
    _intact(rec)
    sub = rec.view.cpu().numpy()[::R.AMAX_SUB_STRIDE]
    assert (sub[1:] == 0).all(), sub
    return R.record_value(rec.view)


@pytest.mark.parametrize("rows,C,ld", ABSMAX_SHAPES)
def test_absmax_finds_a_planted_maximum(rows, C, ld):
    base = torch.rand(rows, C, generator=_gen(rows + C)) * 2 - 1
    g = _inp(base, pitch=ld)
    _same_value(_absmax_value(g, rows, C, ld), R.amax_exact(base), "no plant")
    n4, blocks, stride, last_unrolled, first_tail = R.absmax_geometry(rows, C, ld)
    spots = {0, rows * C - 1, (rows - 1) * C + C - 1}
    if last_unrolled is not None:
        spots |= {4 * last_unrolled + 3, 4 * last_unrolled}
    if first_tail is not None:
        spots |= {4 * first_tail, 4 * first_tail + 3}
    if rows == 8197:
        assert (last_unrolled, first_tail) == (524287, 524288)
    for flat in sorted(spots):
        idx = R.plant(g.view, flat, -7.0)
        _same_value(_absmax_value(g, rows, C, ld), np.float32(7.0), f"maximum at {idx}")
        g.view[idx] = base[idx]
    _same_value(_absmax_value(g, rows, C, ld), R.amax_exact(base), "restored")
    if ld > C:
        # the pitch columns and the floats around the slice hold NaN already; a larger finite value there must not count either
        for off in (g.start + C, g.start + (rows - 1) * ld + C, g.start - 1, g.start + rows * ld):
            g.buf[off] = 1e30
        _same_value(_absmax_value(g, rows, C, ld), R.amax_exact(base), "values outside the slice")


@pytest.mark.parametrize("rows,C,ld", [(7, 36, 52), (1, 1028, 1028), (513, 64, 64)])
def test_absmax_special_values(rows, C, ld):
    g = _inp(torch.zeros(rows, C), pitch=ld)
    R.assert_bits_equal(_absmax_value(g, rows, C, ld), np.float32(0.0), "zeros")
    g.view.fill_(-0.0)
    R.assert_bits_equal(_absmax_value(g, rows, C, ld), np.float32(0.0), "-0.0")
    g.view.copy_(torch.rand(rows, C, generator=_gen(3)) * 2 - 1)
    for spot in (0, rows * C // 2, rows * C - 1):
        idx = R.plant(g.view, spot, float("-inf"))
        assert np.isposinf(_absmax_value(g, rows, C, ld)), idx
        g.view[idx] = float("nan")
        assert np.isnan(_absmax_value(g, rows, C, ld)), idx
        g.view[idx] = 0.5
    R.plant(g.view, 0, float("inf"))
    R.plant(g.view, rows * C - 1, float("nan"))
    assert np.isnan(_absmax_value(g, rows, C, ld))           # NaN wins over infinity


def test_absmax_seventy_calls_in_flight():
    """The per-launch scratch is a ring of 64 slots: 70 launches on one stream, no synchronisation between them, each with
    its own maximum at its own place."""
    n, rows, C = 70, 513, 64                                 # 8208 quads: five blocks per launch
    base = torch.rand(n, rows, C, generator=_gen(5)) * 2 - 1
    want = []
    for k in range(n):
        want.append(np.float32(2.0 + k))
        R.plant(base[k], (k * 4099) % (rows * C), -(2.0 + k))
    g, recs = _inp(base), _record(fill=123.0, n=n)
    for k in range(n):
        _ok(_absmax(g.view[k].data_ptr(), rows, C, C, recs.view[k].data_ptr()), f"absmax {k}")
    torch.cuda.synchronize()
    _intact(recs)
    got = recs.view.cpu().numpy()
    for k in range(n):
        _same_value(R.record_value(got[k]), want[k], f"launch {k}")


def test_absmax_refuses_bad_arguments():
    g = _inp(torch.ones(4, 8), lead=0)
    m = _inp(torch.ones(4, 8), lead=1)
    rec = _record(fill=123.0)
    _refused(_absmax(g.view.data_ptr(), 4, 6, 8, rec.view.data_ptr()))           # C % 4
    _refused(_absmax(g.view.data_ptr(), 2, 8, 4, rec.view.data_ptr()))           # ld < C
    _refused(_absmax(m.view.data_ptr(), 4, 8, 8, rec.view.data_ptr()))           # misaligned x
    _refused(_absmax(g.view.data_ptr(), 4, 8, 8, rec.view.data_ptr() + 4))       # misaligned record
    torch.cuda.synchronize()
    assert bool((rec.view == 123.0).all())
    _intact(rec)


# =============================================================================================== weight norm, per layer
WN_CASES = [(1, 4), (33, 33), (75, 3), (31, 20), (64, 64), (65, 68),
            (4097, 16),         # 65 row chunks: the partial sums live inside w / dV
            (16400, 256)]       # K * Cout just past 4096 * 256 * 4: weightnorm_bwd_kernel's grid wraps


def _wn_inputs(K, Cout, seed, zero_col=True):
    """|V| in [0.5, 1.5]: the scale dV and dg are held to, (sum_k |dw V|) |g| inv, measures the two terms of
    dV = g inv (dw - V dot inv^2) against each other only when V is of order one -- chosen before any run; with |V| << 1
    the rounding of the first term alone exceeds it, whatever the kernel."""
    g = _gen(seed)
    V = (torch.rand(K, Cout, generator=g) + 0.5) * (torch.randint(0, 2, (K, Cout), generator=g) * 2 - 1).float()
    zc = Cout // 2 if zero_col else None
    if zero_col:
        V[:, zc] = 0.0
    gain = torch.rand(Cout, generator=g) + 0.5
    dw = torch.randn(K, Cout, generator=g)
    return V, gain, dw, zc


def _wn_check_fwd(tag, V, gain, w, inv, zc):
    rw, rinv = R.weight_norm_fwd(V, gain)
    _close(tag + " w", w, rw, rw.abs())
    _close(tag + " inv", inv, rinv, rinv.abs())
    if zc is not None:
        assert bool((torch.as_tensor(w)[:, zc] == 0).all())
        want = 1.0 / np.sqrt(np.float64(np.float32(1e-12)))               # rsqrtf(1e-12f)
        assert abs(float(inv[zc]) - want) <= 1e-6 * want


def _wn_check_bwd(tag, V, gain, dw, dV, dg, zc):
    rV, rg = R.weight_norm_bwd(V, gain, dw)
    _, rinv = R.weight_norm_fwd(V, gain)
    col = (dw.double() * V.double()).abs().sum(0) * gain.double().abs() * rinv          # per column: they are differences
    sV, sg = col.expand_as(rV).clone(), col.clone()
    if zc is not None:                                      # the zero column has no second term: dV = g inv dw, dg = 0
        sV[:, zc] = rV[:, zc].abs()
        assert float(torch.as_tensor(dg)[zc]) == 0.0
    _close(tag + " dV", dV, rV, sV)
    _close(tag + " dg", dg, rg, sg)


@pytest.mark.parametrize("K,Cout", WN_CASES)
def test_weightnorm_per_layer(K, Cout):
    V, gain, dw, zc = _wn_inputs(K, Cout, K * 3 + Cout)
    gV, gg, gdw = _inp(V), _inp(gain), _inp(dw)
    w, wT, inv, rec = _out((K, Cout)), _out((Cout, K)), _out((Cout,)), _record()
    _ok(_L().otgan_weightnorm_fwd_amax_f32(gV.view.data_ptr(), gg.view.data_ptr(), K, Cout, w.view.data_ptr(), wT.view.data_ptr(),
                                           inv.view.data_ptr(), rec.view.data_ptr(), _sp()), "weightnorm fwd")
    torch.cuda.synchronize()
    _intact(w, wT, inv, rec, gV, gg)
    wc, invc = w.view.cpu(), inv.view.cpu()
    R.assert_bits_equal(wT.view, wc.t().contiguous(), "wT")        # ragged 32 x 32 tiles at 33, 65, 68, 75, 4097
    _same_value(R.record_value(rec.view), R.amax_exact(wc), "record")
    _wn_check_fwd("weightnorm fwd", V, gain, wc, invc, zc)
    dV, dg, scratch = _out((K, Cout)), _out((Cout,)), _out((Cout,))
    _ok(_L().otgan_weightnorm_bwd_f32(gV.view.data_ptr(), gg.view.data_ptr(), inv.view.data_ptr(), gdw.view.data_ptr(), K, Cout,
                                      dV.view.data_ptr(), dg.view.data_ptr(), scratch.view.data_ptr(), _sp()), "weightnorm bwd")
    torch.cuda.synchronize()
    _intact(dV, dg, scratch, inv, gdw)
    _wn_check_bwd("weightnorm bwd", V, gain, dw, dV.view.cpu(), dg.view.cpu(), zc)


def test_weightnorm_integer_directions():
    """Integer V: the sum of squares is exact in fp32, so inv_norm is rsqrtf of an exact argument -- 4 ulp."""
    K, Cout = 33, 33
    V = R.int_valued((K, Cout), -8, 8, _gen(1))
    V[0] = 1.0
    gV, gg = _inp(V), _inp(torch.ones(Cout))
    w, inv = _out((K, Cout)), _out((Cout,))
    _ok(_L().otgan_weightnorm_fwd_amax_f32(gV.view.data_ptr(), gg.view.data_ptr(), K, Cout, w.view.data_ptr(), None,
                                           inv.view.data_ptr(), None, _sp()), "weightnorm fwd")
    torch.cuda.synchronize()
    _intact(w, inv)
    want = (1.0 / np.sqrt((V.double() ** 2).sum(0).numpy())).astype(np.float32)
    assert int(R.ulp_distance(inv.view, want).max()) <= 4


# =============================================================================================== weight norm, batched
WN_CEFF = [1, 14, 15, 64, 400]          # K = 9 Ceff: fewer rows than the 128 row lanes, about as many, more
WN_LAYER_COUNTS = [1, 16, 17, 33]       # OTGAN_WN_MAX_LAYERS = 16 per launch


@pytest.fixture(scope="module")
def wn_layers():
    """33 layers' inputs (CPU), built once; the fp64 references are computed by the checks from them."""
    out = []
    for k in range(max(WN_LAYER_COUNTS)):
        Ceff = WN_CEFF[k % len(WN_CEFF)]
        V, gain, dw, _ = _wn_inputs(9 * Ceff, 16, 1000 + k, zero_col=False)
        _, rinv = R.weight_norm_fwd(V, gain)
        out.append((Ceff, V, gain, dw, rinv.float()))
    return out


@pytest.mark.parametrize("with_wT", [False, True])
@pytest.mark.parametrize("nl", WN_LAYER_COUNTS)
def test_weightnorm_batched_forward(wn_layers, nl, with_wT):
    from otgan_amd._lib_layers import WnFwdLayer
    arr = (WnFwdLayer * nl)()
    keep = []
    for k in range(nl):
        Ceff, V, gain, _, _ = wn_layers[k]
        K = 9 * Ceff
        gV, gg = _inp(V), _inp(gain)
        w, inv = _out((K, 16)), _out((16,))
        wT = _out((16, K)) if with_wT else None
        a = arr[k]
        a.V, a.g, a.w, a.inv, a.K = gV.view.data_ptr(), gg.view.data_ptr(), w.view.data_ptr(), inv.view.data_ptr(), K
        a.wT = wT.view.data_ptr() if with_wT else None
        keep.append((gV, gg, w, inv, wT))
    _ok(_L().otgan_weightnorm_fwd_batched16_f32(arr, nl, _sp()), "weightnorm fwd batched")
    torch.cuda.synchronize()
    for k, (gV, gg, w, inv, wT) in enumerate(keep):
        _, V, gain, _, _ = wn_layers[k]
        _intact(w, inv, gV, gg)
        wc = w.view.cpu()
        _wn_check_fwd("weightnorm fwd (batched)", V, gain, wc, inv.view.cpu(), None)
        if with_wT:
            _intact(wT)
            R.assert_bits_equal(wT.view, wc.t().contiguous(), f"layer {k} wT")


def _wn_parts(form, Ceff, dw, seed):
    """dw [9 Ceff, 16] cut into the parts of `form`; returns ([(guarded part or None, perm or None, nrows, rstride)])."""
    if form == "one":
        sizes, rstride, perm_first = [Ceff], 16, False
    elif form == "two_perm":
        sizes, rstride, perm_first = [(Ceff + 1) // 2, Ceff // 2], 16, True
    else:
        sizes, rstride, perm_first = [Ceff // 3, Ceff // 3, Ceff - 2 * (Ceff // 3)], int(form.split("_")[1]), False
    dw3 = dw.view(9, Ceff, 16)
    parts, s = [], 0
    for i, n in enumerate(sizes):
        if n == 0:
            parts.append((None, None, 0, 0))
            continue
        piece = dw3[:, s:s + n, :]
        perm = None
        if perm_first and i == 0:
            perm = torch.randperm(n, generator=_gen(seed)).to(torch.int32)
            stored = torch.empty_like(piece)
            stored[:, perm.long(), :] = piece              # the kernel reads row perm[e] for the logical row e
            piece = stored
        parts.append((_inp(piece.reshape(9 * n, 16).contiguous(), pitch=rstride), perm.to(_dev()) if perm is not None else None,
                      n, rstride))
        s += n
    return parts


@pytest.mark.parametrize("form", ["one", "two_perm", "three_16", "three_48"])
@pytest.mark.parametrize("nl", WN_LAYER_COUNTS)
def test_weightnorm_batched_backward(wn_layers, nl, form):
    from otgan_amd._lib_layers import WnBwdLayer
    arr = (WnBwdLayer * nl)()
    keep = []
    for k in range(nl):
        Ceff, V, gain, dw, inv32 = wn_layers[k]
        K = 9 * Ceff
        gV, gg, ginv = _inp(V), _inp(gain), _inp(inv32)
        dV, dg = _out((K, 16)), _out((16,))
        parts = _wn_parts(form, Ceff, dw, 2000 + k)
        a = arr[k]
        a.V, a.g, a.inv, a.dV, a.dg = (t.view.data_ptr() for t in (gV, gg, ginv, dV, dg))
        a.Ceff, a.taps = Ceff, 9
        for i, (part, perm, n, rstride) in enumerate(parts):
            q = a.part[i]
            q.p = part.view.data_ptr() if part is not None else None
            q.perm = perm.data_ptr() if perm is not None else None
            q.nrows, q.rstride = n, rstride
        keep.append((gV, gg, ginv, dV, dg, parts))
    _ok(_L().otgan_weightnorm_bwd_batched16_f32(arr, nl, _sp()), "weightnorm bwd batched")
    torch.cuda.synchronize()
    for k, (gV, gg, ginv, dV, dg, parts) in enumerate(keep):
        _, V, gain, dw, _ = wn_layers[k]
        _intact(dV, dg, gV, gg, ginv, *[p[0] for p in parts if p[0] is not None])
        _wn_check_bwd("weightnorm bwd (batched)", V, gain, dw, dV.view.cpu(), dg.view.cpu(), None)


# =============================================================================================== GLU, tanh, feature head
def _cases(cs_vec, cs_scalar, sizes):
    out = [(n, C, 0) for C in cs_vec + cs_scalar for n in sizes]
    return out + [(sizes[1], 8, 1), (sizes[2], 8, 1)]        # C = 8 on a view one float into its allocation: scalar kernels


GLU_CASES = _cases([4, 36], [1, 3, 6], [1, 5, 257]) + [
    (R.grid_wrap_elements(8) // 64 + 1, 64, 0),              # float4 kernels: just past 4096 * 256 * 8 elements
    (R.grid_wrap_elements(4) // 3 + 1, 3, 0)]                # scalar kernels: just past 4096 * 256 * 4


@pytest.mark.parametrize("rows,C,lead", GLU_CASES)
def test_glu_forward_and_backward(rows, C, lead):
    g = _gen(rows * 5 + C)
    x = torch.cat([torch.randn(rows, C, generator=g) * 3, torch.rand(rows, C, generator=g) * 24 - 12], 1)   # gates in [-12, 12]
    dy = torch.randn(rows, C, generator=g)
    vec = C % 4 == 0 and lead == 0
    assert rows * C <= R.grid_wrap_elements(8 if vec else 4) + 64
    gx, gdy = _inp(x, lead=lead), _inp(dy, lead=lead)
    y, dx = _out((rows, C), lead=lead), _out((rows, 2 * C), lead=lead)
    r1, r2 = (_record(), _record()) if vec else (None, None)
    ptr = lambda r: r.view.data_ptr() if r is not None else None
    _ok(_L().otgan_glu_fwd_amax_f32(gx.view.data_ptr(), rows, C, y.view.data_ptr(), ptr(r1), _sp()), "glu fwd")
    _ok(_L().otgan_glu_bwd_amax_f32(gx.view.data_ptr(), gdy.view.data_ptr(), rows, C, dx.view.data_ptr(), ptr(r2), _sp()), "glu bwd")
    if not vec:          # the scalar kernels keep no record: asking for one is refused before any launch
        rec = _record()
        _refused(_L().otgan_glu_fwd_amax_f32(gx.view.data_ptr(), rows, C, y.view.data_ptr(), rec.view.data_ptr(), _sp()))
        _refused(_L().otgan_glu_bwd_amax_f32(gx.view.data_ptr(), gdy.view.data_ptr(), rows, C, dx.view.data_ptr(), rec.view.data_ptr(), _sp()))
    torch.cuda.synchronize()
    _intact(y, dx, gx, gdy)
    kind = "float4" if vec else "scalar"
    ry = R.glu_fwd(x)
    _close(f"glu fwd ({kind})", y.view, ry, ry.abs())
    rdx = R.glu_bwd(x, dy)
    s = torch.sigmoid(x[:, C:].double())
    _close(f"glu bwd da ({kind})", dx.view[:, :C], rdx[:, :C], rdx[:, :C].abs())
    _close(f"glu bwd dl ({kind})", dx.view[:, C:], rdx[:, C:], (dy.double() * x[:, :C].double() * s).abs())
    if vec:
        _intact(r1, r2)
        _same_value(R.record_value(r1.view), R.amax_exact(y.view), "y record")
        _same_value(R.record_value(r2.view), R.amax_exact(dx.view), "dx record")


@pytest.mark.parametrize("n,lead", [(1, 0), (5, 0), (257, 0), (257, 1), (R.grid_wrap_elements(4) + 257, 0)])
def test_tanh_forward_and_backward(n, lead):
    g = _gen(n)
    x = torch.where(torch.rand(n, generator=g) < 0.5, torch.randn(n, generator=g), torch.rand(n, generator=g) * 40 - 20)
    x[0] = 20.0
    x[-1] = -20.0 if n > 1 else 20.0
    dy = torch.randn(n, generator=g)
    gx, gdy = _inp(x, lead=lead), _inp(dy, lead=lead)
    y, dx = _out((n,), lead=lead), _out((n,), lead=lead)
    _ok(_L().otgan_tanh_fwd_f32(gx.view.data_ptr(), n, y.view.data_ptr(), _sp()), "tanh fwd")
    _ok(_L().otgan_tanh_bwd_f32(y.view.data_ptr(), gdy.view.data_ptr(), n, dx.view.data_ptr(), _sp()), "tanh bwd")
    torch.cuda.synchronize()
    _intact(y, dx, gx, gdy)
    yc, dxc = y.view.cpu(), dx.view.cpu()
    assert float(yc[0]) == 1.0 and float(yc[-1]) == (-1.0 if n > 1 else 1.0)        # saturated: exactly +-1 ...
    assert float(dxc[0]) == 0.0 and float(dxc[-1]) == 0.0                            # ... and the gradient exactly 0
    ry = R.tanh_fwd(x)
    _close("tanh fwd", yc, ry, ry.abs())
    _close("tanh bwd", dxc, R.tanh_bwd(x, dy), dy.double().abs())


HEAD_CASES = [(3, HW, C, 0) for C in (4, 36, 1, 3, 6) for HW in (1, 5, 257)] + [
    (1, 3, 4, 0), (1, 4, 3, 0),          # one sample of 12 floats: fewer than the block's threads, float4 and scalar
    (1, 257, 36, 0), (3, 5, 8, 1), (3, 257, 8, 1)]


@pytest.mark.parametrize("N,HW,C,lead", HEAD_CASES)
def test_feature_head_forward_and_backward(N, HW, C, lead):
    g = _gen(N * 1000 + HW * 10 + C)
    x = torch.randn(N, HW, C, generator=g)
    zeros = HW * C >= 3
    if zeros:
        x[0, 0, 0] = 0.0
        x[-1, -1, -1] = -0.0
    df = torch.randn(N, HW * 2 * C, generator=g)
    gx, gdf = _inp(x, lead=lead), _inp(df, lead=lead)
    f, norm, dx, rec = _out((N, HW * 2 * C), lead=lead), _out((N,)), _out((N, HW, C), lead=lead), _record()
    _ok(_L().otgan_feature_head_fwd_f32(gx.view.data_ptr(), N, HW, C, f.view.data_ptr(), norm.view.data_ptr(), _sp()), "head fwd")
    _ok(_L().otgan_feature_head_bwd_amax_f32(gx.view.data_ptr(), f.view.data_ptr(), norm.view.data_ptr(), gdf.view.data_ptr(), N, HW, C,
                                             dx.view.data_ptr(), rec.view.data_ptr(), _sp()), "head bwd")
    torch.cuda.synchronize()
    _intact(f, norm, dx, rec, gx, gdf)
    kind = "float4" if (C % 4 == 0 and lead == 0) else "scalar"
    rf, rnorm = R.feature_head_fwd(x)
    _close(f"feature head fwd f ({kind})", f.view, rf, rf.abs())
    _close(f"feature head fwd norm ({kind})", norm.view, rnorm, rnorm.abs())
    rdx = R.feature_head_bwd(x, df)
    dot = (rf * df.double()).sum(1)
    active = x.double().abs() / rnorm[:, None, None]                       # the f element of the half that is active
    scale = rdx.abs() + active * (dot.abs() / rnorm)[:, None, None]
    _close(f"feature head bwd ({kind})", dx.view, rdx, scale)
    dxc = dx.view.cpu()
    if zeros:
        assert float(dxc[0, 0, 0]) == 0.0 and float(dxc[-1, -1, -1]) == 0.0  # x == 0 and x == -0.0: neither half is active
    _same_value(R.record_value(rec.view), R.amax_exact(dxc), "dx record")


# =============================================================================================== ops.glu on any contiguous tensor
class _Probe(torch.autograd.Function):
    """Sits where the convolution in front of a GLU would: sees the gradient the GLU's backward hands on."""
    seen = {}

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        from otgan_amd import ops
        _Probe.seen = {"g": g, "colsum": ops.colsum_of(g), "amax": ops.amax_of(g)}
        return g


@pytest.mark.parametrize("which", ["aligned", "x", "dy"])
def test_glu_op_on_a_misaligned_contiguous_view(which):
    """A contiguous view one float into its allocation is a legal argument: ops.glu takes the scalar kernels for it, forward
    and backward, with correct values; the record and column-sum hand-offs ride on the results only where the library wrote
    them (aligned tensors), otherwise the consumers' own reductions run."""
    from otgan_amd import ops
    dev = _dev()
    shape, C = (2, 5, 3, 16), 8
    g = _gen(17)
    xc = torch.cat([torch.randn(shape[:-1] + (C,), generator=g) * 3, torch.rand(shape[:-1] + (C,), generator=g) * 24 - 12], -1)
    dyc = torch.randn(shape[:-1] + (C,), generator=g)

    def place(t, misaligned):
        base = torch.empty(t.numel() + 8, device=dev)
        v = base[1 if misaligned else 4:][:t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and (v.data_ptr() % 16 != 0) == misaligned
        return v
    x = place(xc, which == "x").requires_grad_(True)
    dy = place(dyc, which == "dy")
    y = ops.glu(_Probe.apply(x))
    assert (ops.amax_of(y) is not None) == (which != "x")
    if which != "x":
        _same_value(R.record_value(ops.amax_of(y)), R.amax_exact(y.detach()), "y record")
    ry = R.glu_fwd(xc)
    _close("ops.glu fwd", y.detach(), ry, ry.abs())
    y.backward(dy)
    seen = _Probe.seen
    fused = which == "aligned"
    assert (seen["colsum"] is not None) == fused and (seen["amax"] is not None) == fused
    rdx = R.glu_bwd(xc, dyc)
    s = torch.sigmoid(xc[..., C:].double())
    scale = torch.cat([rdx[..., :C].abs(), (dyc.double() * xc[..., :C].double() * s).abs()], -1)
    _close("ops.glu bwd", seen["g"], rdx, scale)
    if fused:
        wrote = seen["g"].double().reshape(-1, 2 * C).cpu()
        L = R.colsum_chain_length(wrote.shape[0], C, True)
        _close("ops.glu bwd column sums", seen["colsum"], wrote.sum(0), wrote.abs().sum(0), tol=L * 2.0 ** -24)
        _same_value(R.record_value(seen["amax"]), R.amax_exact(seen["g"]), "dx record")
    else:
        # the consumers' fallbacks: a reduction of the tensor itself
        _same_value(R.record_value(ops.absmax_record(seen["g"].contiguous())), R.amax_exact(seen["g"]), "absmax_record")


# =============================================================================================== optimisers and EMA
BIG = R.grid_wrap_elements(4) + 257
MOM2, DECAY = 0.999, 0.999
# (n, mom1, lr, bias corrections from a device tensor); mom1 = 0.9 beside 0.5: 0.5 * v is exact, so only 0.9 would show a
# fused mom1 * v + om1 * g
ADAM_CASES = [(n, m, lr, coef) for n in (1, 255, 257) for m in (0.5, 0.0, 0.9) for lr, coef in ((3e-4, False), (-3e-4, True))] + [
    (BIG, 0.5, 3e-4, False), (BIG, 0.0, -3e-4, True)]


def _opt_state(n, seed):
    g = _gen(seed)
    p = torch.randn(n, generator=g)
    grads = [R.optimiser_gradient(n, g) for _ in range(3)]
    return p, grads


def _bits(tag, step, **pairs):
    for name, (got, want) in pairs.items():
        R.assert_bits_equal(got, want, f"{tag} step {step}: {name}")


@pytest.mark.parametrize("n,mom1,lr,use_coef", ADAM_CASES)
def test_adam_and_ema_are_bit_exact(n, mom1, lr, use_coef):
    from otgan_amd import ops
    p0, grads = _opt_state(n, n + int(mom1 * 10))
    p, v, mg, sh = _out((n,)), (_out((n,)) if mom1 > 0 else None), _out((n,)), _out((n,))
    p.view.copy_(p0)
    sh.view.copy_(p0)
    mg.view.zero_()
    ep, ev, emg, esh = p0.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32), p0.numpy().copy()
    if v is not None:
        v.view.zero_()
    for t in (1, 2, 3):
        gt = _inp(grads[t - 1])
        c1, c2 = ops.adam_coefficients(mom1, MOM2, t)
        coef = torch.tensor([c1, c2], dtype=torch.float32, device=_dev()) if use_coef else None
        ops.adam_step(p.view, gt.view, v.view if v is not None else None, mg.view, lr, mom1, MOM2, 0 if use_coef else t, coef=coef)
        ops.ema_update(sh.view, p.view, DECAY)
        torch.cuda.synchronize()
        ep, ev, emg = R.adam_f32(ep, grads[t - 1], ev, emg, lr, mom1, MOM2, c1, c2)
        esh = R.ema_f32(esh, ep, DECAY)
        _bits("adam", t, p=(p.view, ep), mg=(mg.view, emg), shadow=(sh.view, esh))
        if v is not None:
            _bits("adam", t, v=(v.view, ev))
        _intact(p, mg, sh, gt, *([v] if v is not None else []))


@pytest.mark.parametrize("n,mom1", [(n, m) for n in (1, 255, 257) for m in (0.9, 0.0)] + [(BIG, 0.9)])
def test_adamax_is_bit_exact(n, mom1):
    from otgan_amd import ops
    p0, grads = _opt_state(n, n + 50)
    p, v, mg = _out((n,)), (_out((n,)) if mom1 > 0 else None), _out((n,))
    p.view.copy_(p0)
    mg.view.zero_()
    ep, ev, emg = p0.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    if v is not None:
        v.view.zero_()
    for t in (1, 2, 3):
        gt = _inp(grads[t - 1])
        ops.adamax_step(p.view, gt.view, v.view if v is not None else None, mg.view, 3e-4, mom1, MOM2)
        torch.cuda.synchronize()
        ep, ev, emg = R.adamax_f32(ep, grads[t - 1], ev, emg, 3e-4, mom1, MOM2)
        _bits("adamax", t, p=(p.view, ep), mg=(mg.view, emg))
        if v is not None:
            _bits("adamax", t, v=(v.view, ev))
        _intact(p, mg, gt, *([v] if v is not None else []))


@pytest.mark.parametrize("n", [1, 255, 257, BIG])
def test_nesterov_is_bit_exact(n):
    from otgan_amd import ops
    p0, grads = _opt_state(n, n + 60)
    p, v = _out((n,)), _out((n,))
    p.view.copy_(p0)
    v.view.zero_()
    ep, ev = p0.numpy().copy(), np.zeros(n, np.float32)
    for t in (1, 2, 3):
        gt = _inp(grads[t - 1])
        ops.nesterov_step(p.view, gt.view, v.view, 3e-4, 0.9)
        torch.cuda.synchronize()
        ep, ev = R.nesterov_f32(ep, grads[t - 1], ev, 3e-4, 0.9)
        _bits("nesterov", t, p=(p.view, ep), v=(v.view, ev))
        _intact(p, v, gt)


@pytest.mark.parametrize("use_coef", [False, True])
@pytest.mark.parametrize("mom1", [0.5, 0.0])
@pytest.mark.parametrize("nseg", [5, 32, 2])
def test_adam_gather_is_bit_exact(nseg, mom1, use_coef):
    """Per-variable gradients into a flat buffer whose first segment starts at offset 5: the five floats in front and the
    seven behind belong to somebody else.  Two segments: a long one that wraps the grid beside one of three elements."""
    from otgan_amd import ops
    lens = [BIG, 3] if nseg == 2 else [[1, 255, 257, 1024, 3][k % 5] for k in range(nseg)]
    front, back, total = 5, 7, sum(lens)
    offsets = [front]
    for n in lens:
        offsets.append(offsets[-1] + n)
    size = front + total + back
    g = _gen(nseg * 3 + int(mom1 * 10))
    p0 = torch.randn(size, generator=g)
    p0[:front], p0[front + total:] = 777.0, -777.0
    bufs = {k: _out((size,)) for k in ("p", "v", "mg", "sh")}
    emu = {"p": p0.numpy().copy(), "v": np.full(size, 0.25, np.float32), "mg": np.full(size, 0.5, np.float32), "sh": p0.numpy().copy()}
    for k in bufs:
        bufs[k].view.copy_(torch.from_numpy(emu[k]))
    lr = -3e-4 if use_coef else 3e-4
    body = slice(front, front + total)
    for t in (1, 2, 3):
        grads = [R.optimiser_gradient(n, g) for n in lens]
        gts = [_inp(x) for x in grads]
        c1, c2 = ops.adam_coefficients(mom1, MOM2, t)
        coef = torch.tensor([c1, c2], dtype=torch.float32, device=_dev()) if use_coef else None
        ops.adam_step_gather(bufs["p"].view, [x.view for x in gts], offsets, bufs["v"].view if mom1 > 0 else None, bufs["mg"].view, lr,
                             mom1, MOM2, 0 if use_coef else t, ema_shadow=bufs["sh"].view, ema_decay=DECAY, coef=coef)
        torch.cuda.synchronize()
        ep, ev, emg = R.adam_f32(emu["p"][body], torch.cat(grads), emu["v"][body], emu["mg"][body], lr, mom1, MOM2, c1, c2)
        emu["p"][body], emu["mg"][body] = ep, emg
        if mom1 > 0:
            emu["v"][body] = ev
        emu["sh"][body] = R.ema_f32(emu["sh"][body], ep, DECAY)
        for k in bufs:
            R.assert_bits_equal(bufs[k].view, emu[k], f"adam gather step {t}: {k}")
        _intact(*bufs.values(), *gts)


# =============================================================================================== batched copies
SMALL_COPIES = [(1, 1, 1, 1), (1, 7, 9, 7), (6, 1, 1, 4), (3, 5, 5, 5), (4, 4, 8, 12), (17, 33, 40, 33), (2, 129, 129, 130)]
BIG_COPY = (520, 513, 515, 513)          # 266 760 elements > 256 * 1024: the other segments' workgroups mostly idle


@pytest.mark.parametrize("nseg", [1, 64, 65])
def test_copy2d_batched(nseg):
    from otgan_amd import ops
    g = _gen(nseg)
    dims = [BIG_COPY] + [SMALL_COPIES[k % len(SMALL_COPIES)] for k in range(nseg - 1)]
    data = [torch.randn(r, c, generator=g) for r, c, _, _ in dims]
    srcs = [_inp(d, pitch=sld) for d, (_, _, sld, _) in zip(data, dims)]
    dsts = [_out((r, c), pitch=dld) for r, c, _, dld in dims]
    ops.copy2d_batched([(s.view.data_ptr(), d.view.data_ptr(), r, c, sld, dld) for s, d, (r, c, sld, dld) in zip(srcs, dsts, dims)])
    torch.cuda.synchronize()
    for k, (d, dst, src) in enumerate(zip(data, dsts, srcs)):
        R.assert_bits_equal(dst.view, d, f"segment {k} {dims[k]}")
        _intact(dst, src)


def _arr(ty, vals):
    a = (ty * len(vals))(*vals)
    return a, ctypes.cast(a, ctypes.c_void_p)


def test_copy2d_batched_refusals():
    src, dst = _inp(torch.ones(4, 4)), _out((4, 4))
    dst.view.fill_(5.0)
    sp, dp = src.view.data_ptr(), dst.view.data_ptr()

    def call(n, srcs, dsts, rows, cols, sld, dld):
        keep = [_arr(ctypes.c_void_p, srcs), _arr(ctypes.c_void_p, dsts), _arr(ctypes.c_int, rows), _arr(ctypes.c_int, cols),
                _arr(ctypes.c_long, sld), _arr(ctypes.c_long, dld)]
        return _L().otgan_copy2d_batched_f32(*[k[1] for k in keep], n, _sp())
    _refused(call(0, [sp], [dp], [4], [4], [4], [4]))                                   # no segment
    n = 65                                                                              # one more than the maximum
    _refused(call(n, [sp] * n, [dp] * n, [4] * n, [4] * n, [4] * n, [4] * n))
    _refused(call(1, [sp], [dp], [4], [4], [3], [4]))                                   # src_ld < cols
    _refused(call(1, [sp], [dp], [4], [4], [4], [3]))                                   # dst_ld < cols
    _refused(call(2, [sp, None], [dp, dp], [4, 4], [4, 4], [4, 4], [4, 4]))             # a null segment pointer
    _refused(call(2, [sp, sp], [dp, None], [4, 4], [4, 4], [4, 4], [4, 4]))
    torch.cuda.synchronize()
    assert bool((dst.view == 5.0).all())
    _intact(dst)


@pytest.mark.parametrize("kind", ["permutation", "repeats", "identity"])
@pytest.mark.parametrize("n2", [1, 16, 20])
def test_gather3d_batched(n2, kind):
    from otgan_amd import ops
    g = _gen(n2 * 3 + len(kind))
    nseg, n1, base1 = 32, 6, 2
    if kind == "permutation":
        m = torch.randperm(n1, generator=g)
    elif kind == "repeats":
        m = torch.tensor([3, 0, 3, 3, 5, 0])
    else:
        m = torch.arange(n1)
    map1 = None if kind == "identity" else m.to(torch.int32).to(_dev())
    M1 = base1 + n1 + 1                                   # rows in front of base1 and one behind the mapped range: never read
    # segment 3 sets the grid (with n2 = 20: 264 000 elements, past the 256 x 1024 the capped grid covers in one sweep);
    # segment 7 has 6 * n2 elements: all but the first workgroup of its row never enter the loop
    n0s = [2200 if k == 3 else (1 if k == 7 else k % 5 + 1) for k in range(nseg)]
    used = torch.zeros(M1, dtype=torch.bool)
    used[base1 + m] = True
    segs, keep, peak = [], [], 0.0
    for k, n0 in enumerate(n0s):
        src = torch.randn(n0, M1, n2, generator=g)
        src[:, ~used, :] = 1e30                           # rows the map never names: must reach neither dst nor the record
        if k == 7:
            src[0, base1 + int(m[n1 - 1]), n2 - 1] = -9.5  # the overall maximum sits in the smallest segment
        want = src[:, base1 + m, :]
        gs = _inp(src, pitch=n2 + 3)
        gd = _out((n0, n1, n2), pitch=n2 + 1)
        segs.append((gs.view.data_ptr(), gd.view.data_ptr(), n0, M1 * (n2 + 3), n2 + 3, n1 * (n2 + 1), n2 + 1))
        keep.append((gs, gd, want))
        peak = max(peak, float(want.abs().max()))
    rec = _record()
    ops.gather3d_batched(segs, n1, n2, base1=base1, map1=map1, amax_out=rec.view)
    torch.cuda.synchronize()
    for k, (gs, gd, want) in enumerate(keep):
        R.assert_bits_equal(gd.view, want, f"segment {k}")
        _intact(gd, gs)
    _intact(rec)
    assert peak == 9.5
    _same_value(R.record_value(rec.view), np.float32(peak), "record")


def test_gather3d_batched_refusals():
    src, dst = _inp(torch.ones(2, 3, 4)), _out((2, 3, 4))
    dst.view.fill_(5.0)
    sp, dp = src.view.data_ptr(), dst.view.data_ptr()

    def call(n, srcs, dsts):
        k = len(srcs)
        keep = [_arr(ctypes.c_void_p, srcs), _arr(ctypes.c_void_p, dsts), _arr(ctypes.c_int, [2] * k), _arr(ctypes.c_long, [12] * k),
                _arr(ctypes.c_long, [4] * k), _arr(ctypes.c_long, [12] * k), _arr(ctypes.c_long, [4] * k)]
        p = [q[1] for q in keep]
        return _L().otgan_gather3d_batched_f32(p[0], p[1], p[2], 3, 4, p[3], p[4], p[5], p[6], 0, None, None, n, _sp())
    _refused(call(0, [sp], [dp]))
    _refused(call(33, [sp] * 33, [dp] * 33))
    _refused(call(2, [sp, None], [dp, dp]))
    _refused(call(2, [sp, sp], [dp, None]))
    torch.cuda.synchronize()
    assert bool((dst.view == 5.0).all())
    _intact(dst)


def test_zz_report_worst_ratios():
    """Prints the table of the module docstring (run with -s); asserts nothing beyond what the tests above did."""
    for name in sorted(WORST):
        print(f"WORST {name:45s} {WORST[name]:.3g}")
