"""Precision, recall, density and coverage on the GPU: the fused fp64-MFMA k-NN launch (csrc/knn.hip) against the
brute-force numpy fp64 restatement (tests/pr_ref.py), the host layer (utils/pr.py), the training hook against the device's
own features and against the op-by-op fp64 interpreter (tests/inception_graphs.py), two ranks against one process, and
train.main with --pr_neighbours end to end.

Bars.  A squared distance, per entry of `nearest`: pr_ref.error_bound = 2 (C + 8) 2^-53 (|a| + |b|)^2, derived there; an
order statistic of a row moves by at most the largest bar of the row.  Counts and the four values: EXACT (==), after the
test has shown on the reference alone that every comparison |d2 - threshold| has a margin of more than 1000 bars, so a
mismatch is a kernel error and not a tie.  Order, position, split and role: the same BITS.  The hook against the fp64
interpreter: the network's own error (TOL_NET = 1e-5, tests/test_inception_gpu.py) moves a squared distance and its
threshold by at most 4 TOL_NET (|a| + |b|)^2 together, so a row with a comparison inside that band is "uncertain" and a
value may differ by the uncertain rows of its side / N (density: at most the uncertain pairs / (K N) as well); more than 6
uncertain rows of 96 would hide too much and fail.
Measured on an MI355X: largest error / bar of `nearest` 0.010 ... 0.041 over the shapes (0.0068 at 300 x 257 x 2048); margins
of the count tests 4.6e5 ... 7.8e13 bars, of the four-value tests 1.6e4 (300 x 257 x 2048) ... 5.7e8; the hook on the narrow
graph (0.1771, 0.9583, 0.0972, 0.1771), the fp64 interpreter's values exactly, with 1 generated and 5 real uncertain rows;
two ranks and one process (0.1771, 0.9579, 0.0972, 0.1789) on 96 x 95 rows and (0.1789, 0.9579, 0.0982, 0.1789) on 95 x 95.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pr_ref
import metric_harness as H
from metric_harness import DEV, EVALS    # (96, and 95: the last row of rank 1 falls to the truncation, the shares differ)
from otgan_amd import _lib
from otgan_amd.utils import fid, kid, pr

pytestmark = pytest.mark.gpu
TOL_NET = 1e-5
MARGIN = 1000.0
K = 3


# ---------------------------------------------------------------- inputs and the shared reference
def _sets(seed, ng, nr, C, equal_noise=False):
    """pool_3-like clusters: 8 non-negative centres with a scale per channel (as test_kid_gpu._features), generated rows
    around centres 0 - 5, real rows around centres 2 - 7, per-channel noise 0.5 U(0.2, 1) (one draw for both sides with
    `equal_noise`), absolute values."""
    rng = np.random.default_rng(seed)
    centres = np.abs(rng.standard_normal((8, C))) * rng.uniform(0.05, 3.0, C) + rng.uniform(0.0, 1.0, C)
    sg = 0.5 * rng.uniform(0.2, 1.0, C)
    sr = sg if equal_noise else 0.5 * rng.uniform(0.2, 1.0, C)
    g = np.abs(centres[rng.integers(0, 6, ng)] + rng.standard_normal((ng, C)) * sg)
    r = np.abs(centres[rng.integers(2, 8, nr)] + rng.standard_normal((nr, C)) * sr)
    return g.astype(np.float32), r.astype(np.float32)


# (nq, ny, C, k): the minimum, fewer columns than k, below / at / above one tile and one block in either direction, more
# than one column block per workgroup (65 x 130), a column split with few rows (5 x 1500: 6 splits of 4 blocks), both
# list lengths of the kernel (k <= 4 and k > 4), and the full width with two splits of 4 + 1 blocks (300 x 257 x 2048)
SHAPES = [(1, 2, 4, 1), (3, 3, 4, 3), (7, 9, 40, 3), (16, 17, 40, 3), (17, 16, 40, 3), (33, 30, 100, 3), (63, 64, 40, 1),
          (64, 65, 40, 8), (65, 130, 40, 5), (5, 1500, 40, 3), (70, 600, 40, 8), (300, 257, 2048, 3)]


@functools.lru_cache(maxsize=None)
def _case(nq, ny, C, k):
    """Inputs and reference of one shape, computed once: q, y, the cross distances and bars, the own-set ones of y, and
    thresholds = the reference radii of y with min(K, ny - 1) neighbours."""
    q, y = _sets(nq + 10 * ny + C, nq, ny, C, equal_noise=C == 2048)
    d, bar = pr_ref.dist2(q, y), pr_ref.error_bound(q, y)
    dyy, baryy = pr_ref.dist2(y, y), pr_ref.error_bound(y, y)
    thresh = pr_ref.knn(y, y, min(K, ny - 1), self0=0, d=dyy)[0][:, min(K, ny - 1) - 1]
    return SimpleNamespace(q=q, y=y, d=d, bar=bar, dyy=dyy, baryy=baryy, thresh=thresh)


def _dev(a):
    return torch.as_tensor(a, device=DEV)


def _check_nearest(tag, got, ref, rowbar):
    """Each entry within the largest bar of its row, +inf entries in the same places; returns the largest error / bar."""
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float64, (tag, got.shape, ref.shape)
    assert np.array_equal(np.isinf(got), np.isinf(ref)), (tag, got, ref)
    assert (np.diff(got, axis=1)[np.isfinite(got[:, 1:])] >= 0).all(), tag                 # ascending
    fin = np.isfinite(ref)
    ratio = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)) / rowbar[:, None]
    assert (ratio <= 1.0).all(), (tag, float(ratio.max()))
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------- the kernel against the reference
@pytest.mark.parametrize("nq,ny,C,k", SHAPES)
def test_kernel_against_numpy_fp64(nq, ny, C, k):
    c = _case(nq, ny, C, k)
    # the reference alone: no comparison is a near-tie
    margin = float((np.abs(c.d - c.thresh[None, :]) / c.bar).min())
    assert margin > MARGIN, margin
    qt, yt, tt = _dev(c.q), _dev(c.y), _dev(c.thresh)
    nearest, inside = pr.knn(qt, yt, k, thresh=tt)
    assert nearest.is_cuda and inside.dtype == torch.int32 and inside.shape == (nq,)
    ref_near, ref_in = pr_ref.knn(c.q, c.y, k, thresh=c.thresh, d=c.d)
    worst = _check_nearest("cross", nearest, ref_near, c.bar.max(axis=1))
    assert np.array_equal(inside.cpu().numpy(), ref_in), (inside, ref_in)
    # the own set of y, each row's own column excluded by position
    own, none = pr.knn(yt, yt, k, self0=0)
    assert none is None
    worst_own = _check_nearest("own", own, pr_ref.knn(c.y, c.y, k, self0=0, d=c.dyy)[0], c.baryy.max(axis=1))
    print("knn %d x %d x %d k=%d: margin %.3g bars, largest error / bar %.3g (cross) %.3g (own set)"
          % (nq, ny, C, k, margin, worst, worst_own))
    # the same call gives the same bits
    again = pr.knn(qt, yt, k, thresh=tt)
    assert torch.equal(nearest, again[0]) and torch.equal(inside, again[1])


def test_fewer_columns_than_k_leave_infinities():
    c = _case(3, 3, 4, 3)
    own = pr.knn(_dev(c.y), _dev(c.y), 3, self0=0)[0].cpu().numpy()
    assert np.isinf(own[:, 2]).all() and np.isfinite(own[:, :2]).all()
    nearest, inside = pr.knn(_dev(c.q), _dev(c.y[:0]), 3, thresh=_dev(c.thresh[:0]))      # no column at all
    assert np.isinf(nearest.cpu().numpy()).all() and not inside.any()


def test_a_row_range_of_a_bank_with_its_first_row_as_self0():
    """The multi-rank pattern: the queries are rows lo .. hi of the columns."""
    c = _case(65, 130, 40, 5)
    yt = _dev(c.y)
    whole = pr.knn(yt, yt, 5, self0=0)[0]
    for lo, hi in ((0, 65), (65, 130), (37, 101)):
        part = pr.knn(yt[lo:hi], yt, 5, self0=lo)[0]
        assert torch.equal(part, whole[lo:hi]), (lo, hi)
        _check_nearest("rows %d:%d" % (lo, hi), part, pr_ref.knn(c.y[lo:hi], c.y, 5, self0=lo, d=c.dyy[lo:hi])[0],
                       c.baryy[lo:hi].max(axis=1))


# ---------------------------------------------------------------- the four values are exact
@functools.lru_cache(maxsize=None)
def _pr_case(ng, nr, C):
    g, r = _sets(7 + ng + nr + C, ng, nr, C, equal_noise=C == 2048)
    return g, r, pr_ref.values(g, r, K), pr_ref.margin(g, r, K)


def _bank(rows):
    rows = _dev(rows)
    return kid.FeatureBank(rows.shape[0], rows.shape[1], DEV).append(rows)


@pytest.mark.parametrize("ng,nr,C", [(70, 75, 40), (33, 30, 100), (65, 130, 40), (300, 257, 2048)])
def test_values_equal_the_reference(ng, nr, C):
    g, r, ref, margin = _pr_case(ng, nr, C)
    print("P/R/D/C %d x %d x %d: reference %s, margin %.3g bars" % (ng, nr, C, ref, margin))
    assert margin > MARGIN, margin
    if (ng, C) in ((70, 40), (300, 2048)):           # not vacuous: sets that overlap in part
        assert all(0.05 < v < 0.95 for v in (ref[0], ref[1], ref[3])), ref
    gb, rb = _bank(g), _bank(r)
    got = pr.precision_recall(gb, rb, K)
    assert got == ref and all(type(v) is float for v in got), (got, ref)
    assert tuple(pr.counts(gb, rb, K).tolist()) == pr_ref.counts(g, r, K)
    # the radii of the real rows, computed once and passed in: the same values
    radii = pr.radii(rb.rows, K)
    assert radii.shape == (nr,) and radii.dtype == torch.float64
    assert (np.abs(radii.cpu().numpy() - pr_ref.radii(r, K)) <= pr_ref.error_bound(r, r).max(axis=1)).all()
    assert pr.precision_recall(gb, rb, K, real_radii=radii) == ref


def test_too_few_rows_for_k_are_refused():
    g, r, _, _ = _pr_case(33, 30, 100)
    with pytest.raises(ValueError, match="more than 3 rows"):
        pr.precision_recall(_bank(g[:3]), _bank(r), 3)
    with pytest.raises(ValueError, match="between 1 and 8"):
        pr.precision_recall(_bank(g), _bank(r), 9)


# ---------------------------------------------------------------- order, position, split and role: the same bits
def test_permuted_columns_give_identical_outputs():
    c = _case(65, 130, 40, 5)
    perm = np.random.default_rng(3).permutation(130)
    a = pr.knn(_dev(c.q), _dev(c.y), 5, thresh=_dev(c.thresh))
    b = pr.knn(_dev(c.q), _dev(c.y[perm]), 5, thresh=_dev(c.thresh[perm]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and across the column split: 1500 columns in 6 splits against the same columns in another order
    c = _case(5, 1500, 40, 3)
    perm = np.random.default_rng(4).permutation(1500)
    a = pr.knn(_dev(c.q), _dev(c.y), 3, thresh=_dev(c.thresh))
    b = pr.knn(_dev(c.q), _dev(c.y[perm]), 3, thresh=_dev(c.thresh[perm]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_rows_of_one_call_equal_separate_calls():
    c = _case(300, 257, 2048, 3)
    qt, yt, tt = _dev(c.q), _dev(c.y), _dev(c.thresh)
    whole = pr.knn(qt, yt, 3, thresh=tt)
    for lo, hi in ((0, 5), (60, 70), (299, 300)):          # another tile, block and column split than in the whole call
        part = pr.knn(qt[lo:hi], yt, 3, thresh=tt)
        assert torch.equal(part[0], whole[0][lo:hi]) and torch.equal(part[1], whole[1][lo:hi]), (lo, hi)
    # a shorter list in the kernel (k <= 4) and a longer one (k > 4) agree on what both hold
    assert torch.equal(pr.knn(qt, yt, 5)[0][:, :3], whole[0])


@pytest.mark.parametrize("nq,C", [(8, 40), (70, 100)])
def test_swapped_roles_give_the_same_bits(nq, C):
    """nearest at k = ny = 8 holds every d2 of a row; the transposed calls hold the same pairs the other way round."""
    q, y = _sets(nq, nq, 8, C)
    qt, yt = _dev(q), _dev(y)
    one = pr.knn(qt, yt, 8)[0].cpu().numpy()                                               # [nq, 8]: all pairs
    other = [pr.knn(yt, qt[lo:lo + 8], 8)[0].cpu().numpy() for lo in range(0, nq, 8)]      # [8, 8] each, +inf past nq
    other = np.concatenate([o[np.isfinite(o)] for o in other])
    assert one.size == other.size == nq * 8
    assert np.array_equal(np.sort(one.ravel()).view(np.int64), np.sort(other).view(np.int64))
    # pair by pair, where the kernel leaves no doubt which is which: one query against one column
    for i, j in ((0, 0), (nq - 1, 7), (3, 5)):
        a = pr.knn(qt[i:i + 1], yt[j:j + 1], 1)[0]
        assert torch.equal(a, pr.knn(yt[j:j + 1], qt[i:i + 1], 1)[0]) and float(a) in one[i]


# ---------------------------------------------------------------- self-exclusion by position
def test_repeated_rows_are_neighbours_at_distance_zero():
    c = _case(64, 65, 40, 8)
    y = c.y.copy()
    y[20] = y[64] = y[3]                                   # one row three times, in two column blocks
    yt = _dev(y)
    d = pr_ref.dist2(y, y)
    bar = pr_ref.error_bound(y, y).max(axis=1)
    own = pr.knn(yt, yt, 3, self0=0)[0]
    _check_nearest("repeated rows", own, pr_ref.knn(y, y, 3, self0=0, d=d)[0], bar)
    got = own.cpu().numpy()
    for i in (3, 20, 64):
        assert got[i, 0] == 0.0 and got[i, 1] == 0.0       # exactly: the norms are the diagonal of the same product
        assert abs(got[i, 2] - pr_ref.radii(y, 3)[i]) <= bar[i] and got[i, 2] > 1e6 * bar[i]
    assert (got[[0, 1, 2, 4, 63], 0] > 0).all()
    # without the exclusion every row finds itself first, and the rest moves back by one
    every = pr.knn(yt, yt, 4, self0=-1)[0]
    assert not every[:, 0].any() and torch.equal(every[:, 1:], own)


# ---------------------------------------------------------------- slices, prefilled outputs, bad arguments
def _call(nq, ny, C, q_ptr, ldq, y_ptr, ldy, k, self0, thresh, nearest, inside, ws=None):
    """The C entry point as it is, with a workspace of the queried size unless one is given."""
    L = _lib.lib()
    if ws is None:
        ws = torch.empty(max(L.otgan_knn_workspace_bytes(max(nq, 0), max(ny, 0), min(max(k, 0), 8)) // 8, 1),
                         dtype=torch.float64, device=DEV)
    ptr = lambda t: t.data_ptr() if t is not None else None
    return L.otgan_knn_f64(nq, ny, C, q_ptr, ldq, y_ptr, ldy, k, self0, ptr(thresh), ptr(nearest), ptr(inside),
                           ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr())


def test_reads_column_slices_of_wider_buffers_and_overwrites_its_outputs():
    c = _case(33, 30, 100, 3)
    ldq, offq, ldy, offy = 172, 16, 200, 8
    wideq, widey = np.full((33, ldq), 1e30, np.float32), np.full((30, ldy), 1e30, np.float32)      # poison beside the slices
    wideq[:, offq:offq + 100], widey[:, offy:offy + 100] = c.q, c.y
    wq, wy, tt = _dev(wideq), _dev(widey), _dev(c.thresh)
    nearest = torch.full((33, 3), 1e300, dtype=torch.float64, device=DEV)                          # prefilled: overwritten
    inside = torch.full((33,), 12345, dtype=torch.int32, device=DEV)
    assert _call(33, 30, 100, wq.data_ptr() + 4 * offq, ldq, wy.data_ptr() + 4 * offy, ldy, 3, -1, tt, nearest, inside) == 0
    want = pr.knn(_dev(c.q), _dev(c.y), 3, thresh=tt)
    assert torch.equal(nearest, want[0]) and torch.equal(inside, want[1])
    _check_nearest("slices (C call)", nearest, pr_ref.knn(c.q, c.y, 3, d=c.d)[0], c.bar.max(axis=1))
    # the wrapper passes the row strides of sliced tensors on
    got = pr.knn(wq[:, offq:offq + 100], wy[:, offy:offy + 100], 3, thresh=tt)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a slice the kernel cannot read in 16-byte pieces is copied, not refused
    got = pr.knn(wq[:, offq:offq + 100], _dev(np.pad(widey, ((0, 0), (1, 3))))[:, offy + 1:offy + 101], 3, thresh=tt)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_bad_arguments_leave_the_outputs_untouched():
    x = torch.ones(8, 48, device=DEV)
    th = torch.ones(8, dtype=torch.float64, device=DEV)
    nearest = torch.full((8, 3), 7.0, dtype=torch.float64, device=DEV)
    inside = torch.full((8,), 7, dtype=torch.int32, device=DEV)
    p = x.data_ptr()
    assert _call(8, 8, 6, p, 48, p, 48, 3, 0, th, nearest, inside) != 0              # C not a multiple of 4
    assert _call(8, 8, 0, p, 48, p, 48, 3, 0, th, nearest, inside) != 0              # C = 0
    assert _call(8, 8, 40, p, 36, p, 48, 3, 0, th, nearest, inside) != 0             # ldq < C
    assert _call(8, 8, 40, p, 48, p, 36, 3, 0, th, nearest, inside) != 0             # ldy < C
    assert _call(8, 8, 40, p, 48, p, 50, 3, 0, th, nearest, inside) != 0             # ldy not a multiple of 4
    assert _call(-1, 8, 40, p, 48, p, 48, 3, 0, th, nearest, inside) != 0
    assert _call(8, -1, 40, p, 48, p, 48, 3, 0, th, nearest, inside) != 0
    assert _call(8, 8, 40, p, 48, p, 48, 9, 0, th, nearest, inside) != 0             # k > 8
    assert _call(8, 8, 40, p, 48, p, 48, -1, 0, th, nearest, inside) != 0
    assert _call(8, 8, 40, p, 48, p, 48, 3, -2, th, nearest, inside) != 0            # self0 < -1
    assert _call(8, 8, 40, p, 48, p, 48, 3, 0, th, nearest, None) != 0               # thresh without inside
    assert _call(8, 8, 40, p, 48, p, 48, 3, 0, None, nearest, inside) != 0           # inside without thresh
    assert _call(8, 8, 40, p, 48, p, 48, 3, 0, th, None, inside) != 0                # null nearest with k > 0
    assert _call(8, 8, 40, p + 4, 48, p, 48, 3, 0, th, nearest, inside) != 0         # rows not 16-byte aligned
    assert _call(8, 8, 40, p, 48, p + 8, 48, 3, 0, th, nearest, inside) != 0
    small = torch.empty(1, dtype=torch.float64, device=DEV)
    assert _call(8, 8, 40, p, 48, p, 48, 3, 0, th, nearest, inside, ws=small) == -2  # OTGAN_ERR_WORKSPACE
    assert _call(0, 8, 40, p, 48, p, 48, 3, 0, th, nearest, inside) == 0             # nothing to do: OTGAN_OK, nothing launched
    torch.cuda.synchronize()
    assert torch.equal(nearest, torch.full((8, 3), 7.0, dtype=torch.float64, device=DEV))
    assert torch.equal(inside, torch.full((8,), 7, dtype=torch.int32, device=DEV))
    # ny = 0: +inf and 0, no workspace needed
    assert _call(8, 0, 40, p, 48, p, 48, 3, 0, th, nearest, inside) == 0
    assert torch.isinf(nearest).all() and not inside.any()
    # workspace: the norms of both sides, then per (column split, query row) k doubles and one count, rounded up to 8 bytes
    L = _lib.lib()
    assert L.otgan_knn_workspace_bytes(8, 8, 3) == (16 + 8 * 3) * 8 + 8 * 4                          # one split
    assert L.otgan_knn_workspace_bytes(5, 1500, 3) == (1505 + 6 * 5 * 3) * 8 + 6 * 5 * 4            # 24 column blocks: 6 splits of 4
    assert L.otgan_knn_workspace_bytes(3, 2, 0) == 5 * 8 + 16                                        # 12 bytes of counts, rounded
    assert L.otgan_knn_workspace_bytes(50000, 50000, 3) == (100000 + 2 * 50000 * 3) * 8 + 2 * 50000 * 4   # 782 x 2 workgroups
    assert L.otgan_knn_workspace_bytes(0, 8, 3) == 0 and L.otgan_knn_workspace_bytes(8, 0, 3) == 0


def test_wrapper_rejects_bad_inputs_on_the_host():
    x = torch.ones(8, 40, device=DEV)
    with pytest.raises(_lib.OtganError, match="no CPU fallback"):
        pr.knn(x.cpu(), x, 1)
    with pytest.raises(ValueError):
        pr.knn(x.double(), x, 1)
    with pytest.raises(ValueError):
        pr.knn(x, x[:, :36], 1)                                                      # different channels
    with pytest.raises(ValueError):
        pr.knn(x, x, 9)
    with pytest.raises(ValueError):
        pr.knn(x, x, 1, self0=-2)
    with pytest.raises(ValueError):
        pr.knn(x, x, 1, thresh=torch.ones(7, dtype=torch.float64, device=DEV))       # one threshold per column
    with pytest.raises(ValueError):
        pr.knn(x, x, 1, thresh=torch.ones(8, device=DEV))                            # fp32 thresholds
    assert pr.knn(x[:0], x, 2)[0].shape == (0, 2)


# ---------------------------------------------------------------- the hook on the narrow graph (C = 40)
def _args(eval_samples, k=K, **more):
    return SimpleNamespace(eval_samples=eval_samples, pr_neighbours=k, seed=H.SEED, **more)


def _state(real, k=K):
    return H.state(pr_real=real, pr_real_radii=pr.radii(real.rows, k))


@functools.lru_cache(maxsize=None)
def _device_rows():
    """pool_3 of the two 96-image sets from the device network (numpy): what the hook's banks hold."""
    net = H.net()
    xa, xb = H.sets()
    return H.pool3(net, xa).cpu().numpy(), H.pool3(net, xb).cpu().numpy()


def test_hook_equals_the_reference_on_the_device_features(capsys):
    from otgan_amd.train import inception_hook
    net = H.net()
    xa, xb = H.sets()
    real = kid.real_bank(net, xb, 96)
    state = _state(real)
    model = H.Replay(xa)                        # its samples fail when read on the host
    out = inception_hook(model, _args(96), net, state)
    printed = capsys.readouterr().out
    # the rows the banks hold are the network's pool_3 of the two sets (the batches differ: not bit for bit) ...
    pa, pb = state["kid_gen"].rows.cpu().numpy(), real.rows.cpu().numpy()
    for have, want in zip((pa, pb), _device_rows()):
        assert have.shape == (96, 40) and np.allclose(have, want, rtol=1e-5, atol=1e-6)
    # ... and of those rows the hook returns exactly the reference's values
    ref, margin = pr_ref.values(pa, pb, K), pr_ref.margin(pa, pb, K)
    assert margin > MARGIN, margin
    with capsys.disabled():
        print("hook: P/R/D/C %s on the device's features, margin %.3g bars" % (ref, margin))
    assert out["pr_live"] == ref and out["pr_EMA"] == ref and set(out) == {"live", "EMA", "pr_live", "pr_EMA"}
    assert model.at == {False: 96, True: 96}             # one pass over the samples per evaluated model
    lines = printed.splitlines()
    fmt = "precision was %.4f, recall was %.4f, density was %.4f, coverage was %.4f"
    assert len(lines) == 5
    assert lines[0].startswith("inception score was") and lines[1] == fmt % ref
    assert lines[2].startswith("EMA inception score was") and lines[3] == "EMA " + fmt % ref
    assert lines[4].startswith("max inception score was")

    # 50 of the 96 samples: exactly those rows
    state50 = _state(real)
    out50 = inception_hook(H.Replay(xa), _args(50), net, state50)
    capsys.readouterr()
    pa50 = state50["kid_gen"].rows.cpu().numpy()
    assert pa50.shape == (50, 40) and np.allclose(pa50, _device_rows()[0][:50], rtol=1e-5, atol=1e-6)
    ref50, margin50 = pr_ref.values(pa50, pb, K), pr_ref.margin(pa50, pb, K)
    assert margin50 > MARGIN and ref50 != ref            # (the other 46 rows would have shown)
    assert out50["pr_live"] == ref50 and out50["pr_EMA"] == ref50


def test_hook_prints_after_the_fid_and_kid_lines(capsys):
    from otgan_amd.train import inception_hook
    net = H.net()
    xa, xb = H.sets()
    real = kid.real_bank(net, xb, 96)
    mu, sigma, _ = fid.dataset_stats(net, xb)
    state = _state(real)
    state.update(fid_real=(mu, sigma), kid_real=real)    # KID and P&R share the real bank
    out = inception_hook(H.Replay(xa), _args(96, kid_subsets=8, kid_subset_size=32), net, state)
    lines = capsys.readouterr().out.splitlines()
    names = ("inception score was", "FID was", "KID was", "precision was", "EMA inception score was", "EMA FID was",
             "EMA KID was", "EMA precision was", "max inception score was", "min FID was", "min KID was")
    assert [l.split(",")[0].rsplit(" ", 1)[0] for l in lines] == [n for n in names], lines
    alone = inception_hook(H.Replay(xa), _args(96), net, _state(real))
    capsys.readouterr()
    assert out["pr_live"] == alone["pr_live"] and out["live"] == alone["live"]
    kid_only = inception_hook(H.Replay(xa), SimpleNamespace(eval_samples=96, kid_subsets=8, kid_subset_size=32, seed=H.SEED),
                              net, H.state(kid_real=real))
    capsys.readouterr()
    assert out["kid_live"] == kid_only["kid_live"]       # KID is what it is without --pr_neighbours


def test_hook_with_zero_neighbours_is_the_hook_without_the_flag(capsys):
    from otgan_amd.train import inception_hook
    net = H.net()
    xa, xb = H.sets()
    real = kid.real_bank(net, xb, 96)
    state0, state1 = _state(real), {"max": 0.0, "iter": 0, "epoch": 3}
    out0 = inception_hook(H.Replay(xa), _args(96, k=0), net, state0)
    printed0 = capsys.readouterr().out
    out1 = inception_hook(H.Replay(xa), SimpleNamespace(eval_samples=96), net, state1)
    printed1 = capsys.readouterr().out
    assert set(out0) == {"live", "EMA"} and out0 == out1
    assert printed0 == printed1 and "precision" not in printed0
    del state0["pr_real"], state0["pr_real_radii"]
    assert state0 == state1


def _uncertain(d, thresh, tol):
    """bool [rows, columns]: comparisons d2 <= threshold that the network's own error can flip."""
    return np.abs(d - thresh) <= tol


def test_hook_against_the_fp64_interpreter(capsys):
    from otgan_amd.train import inception_hook
    net = H.net()
    xa, xb = H.sets()
    (p3a, _), (p3b, _) = H.interpreter(0), H.interpreter(1)
    ref = pr_ref.values(p3a, p3b, K)
    d = pr_ref.dist2(p3a, p3b)
    na, nb = np.sqrt((p3a * p3a).sum(axis=1)), np.sqrt((p3b * p3b).sum(axis=1))
    tol = 4.0 * TOL_NET * (na[:, None] + nb[None, :]) ** 2
    rg, rr = pr_ref.radii(p3a, K), pr_ref.radii(p3b, K)
    in_real, in_gen = _uncertain(d, rr[None, :], tol), _uncertain(d, rg[:, None], tol)    # [g, r] both
    # a generated row takes part in precision and density through the real balls; a real row in recall through the
    # generated balls and in coverage through its own ball
    ug, ur = int(in_real.any(axis=1).sum()), int((in_gen.any(axis=0) | in_real.any(axis=0)).sum())
    out = inception_hook(H.Replay(xa), _args(96), net, _state(kid.real_bank(net, xb, 96)))
    capsys.readouterr()
    got = out["pr_live"]
    bars = (ug / 96, ur / 96, min(ug / 96, int(in_real.sum()) / (K * 96)), ur / 96)
    with capsys.disabled():
        print("hook against the fp64 interpreter: device %s, interpreter %s; uncertain rows: %d generated, %d real; bars %s"
              % (got, ref, ug, ur, bars))
    assert max(ug, ur) <= 6, (ug, ur)                                                      # else the bars hide too much
    assert any(0.05 < v < 0.95 for v in ref), ref                                          # not vacuous
    for name, g, r, bar in zip(("precision", "recall", "density", "coverage"), got, ref, bars):
        assert abs(g - r) <= bar + 1e-12, (name, g, r, bar)
    assert out["pr_EMA"] == got


# ---------------------------------------------------------------- two ranks equal one process
def _rank_worker(rank, world, path):
    from otgan_amd.train import inception_hook
    net = H.net()
    xa, xb = H.sets()
    real = kid.real_bank(net, xb, 95, rank, world)               # shares of 48 and 47 rows
    assert real.n == 48 - rank and real.total == 95
    radii = pr.radii(real.rows, K, rank, world)
    assert radii.shape == (95,)
    res = {"real": real.rows.cpu(), "radii": radii.cpu()}
    for ev in EVALS:
        share = -(-ev // world)
        state = H.state(pr_real=real, pr_real_radii=radii)
        out = inception_hook(H.Replay(xa[rank * share:(rank + 1) * share]), _args(ev), net, state, rank, world)
        res[ev] = (out["pr_live"], out["pr_EMA"], state["kid_gen"].rows.cpu())
    return res


def test_two_ranks_return_exactly_what_one_process_returns():
    got = H.two_ranks(_rank_worker)
    real = torch.cat([got[0]["real"], got[1]["real"]])
    assert real.shape[0] == 95 and torch.equal(got[0]["radii"], got[1]["radii"])
    rb = _bank(real)
    assert torch.equal(pr.radii(rb.rows, K).cpu(), got[0]["radii"])          # the gathered radii: one process's bits
    for ev in EVALS:
        assert got[0][ev][:2] == got[1][ev][:2], (ev, got)                   # every rank ends with the same values
        gen = torch.cat([got[0][ev][2], got[1][ev][2]])
        assert gen.shape[0] == ev
        single = pr.precision_recall(_bank(gen), rb, K)                      # one process on the same rows
        ref, margin = pr_ref.values(gen.numpy(), real.numpy(), K), pr_ref.margin(gen.numpy(), real.numpy(), K)
        print("two ranks, %d samples: %s, one process %s, reference %s (margin %.3g bars)" % (ev, got[0][ev][0], single, ref, margin))
        assert got[0][ev][0] == single and got[0][ev][1] == single
        assert margin > MARGIN and single == ref


# ---------------------------------------------------------------- train.main end to end
def test_train_main_with_precision_and_recall(tmp_path, capsys):
    from otgan_amd import train
    common = H.train_args(tmp_path)
    train.main(common + ["--pr_neighbours", "3"])
    out = capsys.readouterr().out
    assert out.count("precision / recall features of the real data: pool_3 of the first 20 training images, kept on the device") == 1
    lines = out.splitlines()
    names = ("inception score was", "precision was", "EMA inception score was", "EMA precision was", "max inception score was")
    first = [n for n, l in enumerate(lines) if l.startswith("inception score was")][0]
    assert all(l.startswith(n) for l, n in zip(lines[first:first + 5], names)), lines[first:first + 5]      # consecutive lines
    vals = [float(w.rstrip(",")) for w in lines[first + 1].split() if w[0].isdigit()]
    assert len(vals) == 4 and all(np.isfinite(v) and v >= 0.0 for v in vals) and max(vals[0], vals[1], vals[3]) <= 1.0
    assert "KID" not in out and "FID" not in out
    # with KID on the same 20 images the bank is shared, and each line follows the KID line
    train.main(common + ["--pr_neighbours", "3", "--kid_subsets", "4", "--kid_subset_size", "8"])
    out = capsys.readouterr().out
    assert "the bank KID keeps" in out
    kinds = H.kinds(out.splitlines(), ("inception score was", "KID was", "precision was", "EMA inception score was",
                                                "EMA KID was", "EMA precision was", "max inception score was", "min KID was"))
    assert kinds == ["inception score was", "KID was", "precision was", "EMA inception score was", "EMA KID was",
                     "EMA precision was", "max inception score was", "min KID was"], out
    # without the flag: nothing of it
    train.main(common)
    out = capsys.readouterr().out
    assert "precision was" not in out and "precision / recall features" not in out and "max inception score was" in out


def test_train_main_precision_and_recall_notices(tmp_path, capsys):
    from otgan_amd import train
    common = H.train_args(tmp_path)
    # more neighbours than the 20 samples have rows: an error before the first step
    with pytest.raises(ValueError):
        train.main(common + ["--pr_neighbours", "30"])
    assert "starting training" in capsys.readouterr().out
    with pytest.raises(ValueError, match="more than 8 rows"):
        train.main(common + ["--pr_neighbours", "8", "--pr_real_samples", "8"])
    out = capsys.readouterr().out
    assert "starting training" in out and "Iteration" not in out
    # with a classifier that is not the 2015 graph: said once, training goes on
    train.main(common[:-2] + ["--pr_neighbours", "3"])
    out = capsys.readouterr().out
    assert out.count("precision and recall need the 2015 Inception graph") == 1 and "precision was" not in out
    assert "Iteration 1" in out
