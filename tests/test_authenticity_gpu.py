"""GPU: otgan_nn_u8 (csrc/pixnn.hip) and utils/authenticity.py against the numpy restatement in authenticity_ref.py.  Every
comparison is exact equality: distances are integers and the ranking is a total order."""
import functools

import numpy as np
import pytest
import torch

import authenticity_ref as R
import metric_harness as H
from metric_harness import DEV
from otgan_amd import _lib, ops
from otgan_amd.utils import authenticity

pytestmark = pytest.mark.gpu

NQS, KS = (1, 63, 65, 130), (1, 3, 8)
NY_SPLIT = 600                 # 5 column blocks of 128 at 4 per split: two splits (asserted below from the workspace size)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _nn(q, y, k, self0=-1):
    index, dist = ops.nn_u8(_dev(q), _dev(y), k, self0)
    assert index.dtype == torch.int32 and dist.dtype == torch.int64
    return index.cpu().numpy(), dist.cpu().numpy()


def _splits(nq, ny, k):
    """column splits, from the documented workspace layout: 8 splits nq k bytes of keys, then the norms"""
    nbytes = _lib.lib().otgan_nn_u8_workspace_bytes(nq, ny, k)
    norms = (4 * (nq + ny) + 7) // 8 * 8
    assert (nbytes - norms) % (8 * nq * k) == 0
    return (nbytes - norms) // (8 * nq * k)


# ---------------------------------------------------------------- the MFMA lane map
def _lane_map_patterns():
    """q . y = 64 i + j (mod 4096) for row i of q and row j of y: a different number for every (i, j), and for (j, i).
    Values 0 and 1 carry i and j (q = (i, 1), y = (64, j)); in values 2 ... 32 q is random and y is 64, in 33 ... 63 the roles
    are swapped, the last value of each range chosen so that the range's sum is a multiple of 64 -- its product, of 4096."""
    rng = np.random.default_rng(11)
    q, y = np.zeros((64, 64), np.int64), np.zeros((64, 64), np.int64)
    i = np.arange(64)
    q[:, 0], q[:, 1], y[:, 0], y[:, 1] = i, 1, 64, i
    q[:, 2:33], y[:, 2:33] = rng.integers(0, 256, (64, 31)), 64
    q[:, 32] = (-q[:, 2:32].sum(1)) % 64 + 64 * rng.integers(0, 3, 64)
    y[:, 33:], q[:, 33:] = rng.integers(0, 256, (64, 31)), 64
    y[:, 63] = (-y[:, 33:63].sum(1)) % 64 + 64 * rng.integers(0, 3, 64)
    return q.astype(np.uint8), y.astype(np.uint8)


def test_lane_map_with_asymmetric_operands():
    """64 x 64 x 64 with a product that names its row and column, so a row / column swap, a permuted tile or a lane that
    fetches another row's bytes changes the table.  The table is recovered in 8-column slices with k = 8."""
    q, y = _lane_map_patterns()
    dots = q.astype(np.int64) @ y.astype(np.int64).T
    assert np.array_equal(dots % 4096, 64 * np.arange(64)[:, None] + np.arange(64)[None, :]) and len(np.unique(dots)) == 4096
    want = R.distances(q, y)
    assert not np.array_equal(want, want.T)
    got = np.full((64, 64), -1, np.int64)
    for j0 in range(0, 64, 8):
        index, dist = _nn(q, y[j0:j0 + 8], 8)
        assert np.array_equal(np.sort(index, axis=1), np.tile(np.arange(8), (64, 1)))
        np.put_along_axis(got[:, j0:j0 + 8], index.astype(np.int64), dist, axis=1)
    assert np.array_equal(got, want)
    # and the products themselves, from d = |q|^2 + |y|^2 - 2 q . y
    norms = (q.astype(np.int64) ** 2).sum(1)[:, None] + (y.astype(np.int64) ** 2).sum(1)[None, :]
    assert np.array_equal((norms - got) // 2, dots)


# ---------------------------------------------------------------- against the reference
@functools.lru_cache(maxsize=None)
def _grid_case(ny, D):
    """130 queries and ny columns inside wider buffers (a column slice at byte 16, a pitch above D), and their table"""
    rng = np.random.default_rng(1000 * ny + D)
    wq = rng.integers(0, 256, (130, D + 32), dtype=np.uint8)
    wy = rng.integers(0, 256, (ny, D + 16), dtype=np.uint8)
    if ny > 4:                                                 # near and equal rows, so that the order is tested at small d
        wy[3, :D] = wq[0, 16:16 + D]
        wy[1, :D] = wq[0, 16:16 + D]
    return wq, wy, R.distances(wq[:, 16:16 + D], wy[:, :D])


@pytest.mark.parametrize("D", [16, 48, 80, 192, 3072])
@pytest.mark.parametrize("ny", [1, 5, 64, 257, NY_SPLIT])
def test_against_reference(ny, D):
    wq, wy, table = _grid_case(ny, D)
    dq, dy = _dev(wq)[:, 16:16 + D], _dev(wy)[:, :D]
    assert dq.stride(0) == D + 32 and dq.data_ptr() % 16 == 0 and dy.stride(0) == D + 16
    if ny == NY_SPLIT:
        assert _splits(130, ny, 3) >= 2
    for nq in NQS:
        for k in KS:
            index, dist = ops.nn_u8(dq[:nq], dy, k)
            want_i, want_d = R.nearest_from_table(table[:nq], k)
            assert np.array_equal(index.cpu().numpy(), want_i) and np.array_equal(dist.cpu().numpy(), want_d), (nq, k)
            if ny < k:
                assert (want_i[:, ny:] == -1).all() and (want_d[:, ny:] == -1).all()
    # the same rows as contiguous tensors, and through the [n, S, S, 3] form where D allows it
    index, dist = ops.nn_u8(dq.contiguous(), dy.contiguous(), 3)
    want_i, want_d = R.nearest_from_table(table, 3)
    assert np.array_equal(index.cpu().numpy(), want_i) and np.array_equal(dist.cpu().numpy(), want_d)
    if D in (48, 192, 3072):
        S = {48: 4, 192: 8, 3072: 32}[D]
        index, dist = ops.nn_u8(dq.contiguous().view(130, S, S, 3), dy.contiguous().view(ny, S, S, 3), 3)
        assert np.array_equal(index.cpu().numpy(), want_i) and np.array_equal(dist.cpu().numpy(), want_d)


def test_empty_sides():
    q = torch.zeros(3, 16, dtype=torch.uint8, device=DEV)
    index, dist = ops.nn_u8(q, q[:0], 2)
    assert bool((index == -1).all()) and bool((dist == -1).all()) and tuple(index.shape) == (3, 2)
    index, dist = ops.nn_u8(q[:0], q, 2)
    assert tuple(index.shape) == (0, 2) and tuple(dist.shape) == (0, 2)


# ---------------------------------------------------------------- extremes
@pytest.mark.parametrize("D", [12288, 49152])
def test_extremes(D):
    """all-0 against all-255: D 255^2, at D = 49152 3 196 108 800 > 2^31; all-0 against all-0: 0"""
    nq, ny = 3, 70
    q = torch.zeros(nq, D, dtype=torch.uint8, device=DEV)
    y = torch.full((ny, D), 255, dtype=torch.uint8, device=DEV)
    far = D * 65025
    if D == 49152:
        assert far == 3196108800 and far > 2 ** 31
    index, dist = ops.nn_u8(q, y, 3)
    assert index.cpu().tolist() == [[0, 1, 2]] * nq and dist.cpu().tolist() == [[far] * 3] * nq
    index, dist = ops.nn_u8(y[:nq], torch.zeros_like(y), 3)
    assert index.cpu().tolist() == [[0, 1, 2]] * nq and dist.cpu().tolist() == [[far] * 3] * nq
    y[41] = 0                                                  # one all-0 row among them: distance 0, first
    y[7, 5] = 254                                              # and one row nearer by 255^2 - 254^2 = 509
    index, dist = ops.nn_u8(q, y, 3)
    assert index.cpu().tolist() == [[41, 7, 0]] * nq and dist.cpu().tolist() == [[0, far - 509, far]] * nq
    index, dist = ops.nn_u8(q, torch.zeros_like(y), 8)
    assert index.cpu().tolist() == [list(range(8))] * nq and bool((dist == 0).all())


# ---------------------------------------------------------------- ties, self exclusion
def test_ties_go_to_the_smaller_column():
    rng = np.random.default_rng(5)
    D = 80
    base = rng.integers(0, 256, (20, D), dtype=np.uint8)
    y = rng.integers(0, 256, (300, D), dtype=np.uint8)
    for at in (290, 131, 17, 128, 127, 255):                   # the same row at known positions, across blocks and waves
        y[at] = base[0]
    y[[250, 60]] = base[1]
    q = base.copy()
    index, dist = _nn(q, y, 8)
    assert index[0, :6].tolist() == [17, 127, 128, 131, 255, 290] and dist[0, :6].tolist() == [0] * 6
    assert index[1, :2].tolist() == [60, 250]
    want = R.nearest(q, y, 8)
    assert np.array_equal(index, want[0]) and np.array_equal(dist, want[1])


def test_self_exclusion_by_position():
    rng = np.random.default_rng(6)
    bank = rng.integers(0, 256, (150, 48), dtype=np.uint8)
    bank[140] = bank[3]                                        # a duplicate is another row: returned at distance 0
    table = R.distances(bank, bank)
    index, dist = _nn(bank, bank, 3, self0=0)
    want = R.nearest_from_table(table, 3, self0=0)
    assert np.array_equal(index, want[0]) and np.array_equal(dist, want[1])
    assert not (index == np.arange(150)[:, None]).any() and (index[3, 0], dist[3, 0]) == (140, 0)
    # a share of the rows against the whole bank, the way a rank calls it
    index, dist = _nn(bank[129:], bank, 3, self0=129)
    assert np.array_equal(index, want[0][129:]) and np.array_equal(dist, want[1][129:])
    # self0 + i >= ny excludes nothing: rows 0 ... 9 against the first 12 columns with self0 = 8 skip columns 8 ... 11 only
    index, dist = _nn(bank[:10], bank[:12], 3, self0=8)
    want = R.nearest_from_table(table[:10, :12], 3, self0=8)
    assert np.array_equal(index, want[0]) and np.array_equal(dist, want[1])
    assert (index[4:, 0] == np.arange(4, 10)).all() and (dist[4:, 0] == 0).all()       # their own rows, not excluded
    assert not (index[:4] == np.arange(8, 12)[:, None]).any()


# ---------------------------------------------------------------- order-free
def test_order_free():
    rng = np.random.default_rng(7)
    nq, ny, D, k = 130, 700, 192, 8
    q = rng.integers(0, 4, (nq, D), dtype=np.uint8) * 60          # few levels: many equal distances ...
    q[:65] = rng.integers(0, 256, (65, D), dtype=np.uint8)        # ... and rows of every level: hardly any
    y = rng.integers(0, 4, (ny, D), dtype=np.uint8) * 60
    table = R.distances(q, y)
    index, dist = _nn(q, y, k)
    want = R.nearest_from_table(table, k)
    assert np.array_equal(index, want[0]) and np.array_equal(dist, want[1])
    again = _nn(q, y, k)
    assert np.array_equal(again[0], index) and np.array_equal(again[1], dist)      # identical bits
    # permuted columns: the rule holds in the permuted numbering, and mapped back the result is the same wherever the rule
    # did not decide -- a row whose k + 1 smallest distances differ maps back exactly; in any row the distances are the same
    # and so is the set of columns nearer than the last one listed
    perm = rng.permutation(ny)
    pi, pd = _nn(q, y[perm], k)
    wantp = R.nearest_from_table(table[:, perm], k)
    assert np.array_equal(pi, wantp[0]) and np.array_equal(pd, wantp[1]) and np.array_equal(pd, dist)
    back = perm[pi]
    free = np.array([len(set(np.sort(table[i])[:k + 1].tolist())) == k + 1 for i in range(nq)])
    assert free.sum() >= 30 and (~free).sum() >= 30
    assert np.array_equal(back[free], index[free])
    for i in range(nq):
        inside = dist[i] < dist[i, -1]
        assert set(back[i][inside].tolist()) == set(index[i][inside].tolist())
    # queries split over two calls
    a, b = _nn(q[:67], y, k), _nn(q[67:], y, k)
    assert np.array_equal(np.concatenate([a[0], b[0]]), index) and np.array_equal(np.concatenate([a[1], b[1]]), dist)
    # columns split over two calls, merged on the host
    (ai, ad), (bi, bd) = _nn(q, y[:333], k), _nn(q, y[333:], k)
    for i in range(nq):
        pairs = sorted(list(zip(ad[i].tolist(), ai[i].tolist())) + list(zip(bd[i].tolist(), (bi[i] + 333).tolist())))[:k]
        assert pairs == list(zip(dist[i].tolist(), index[i].tolist()))


# ---------------------------------------------------------------- raw calls: guards, bad arguments
def test_overwrite_guards():
    rng = np.random.default_rng(8)
    nq, ny, D, k = 70, 300, 48, 5
    q, y = rng.integers(0, 256, (nq, D), dtype=np.uint8), rng.integers(0, 256, (ny, D), dtype=np.uint8)
    want = R.nearest(q, y, k)
    dq, dy = _dev(q), _dev(y)
    L = _lib.lib()
    nbytes = L.otgan_nn_u8_workspace_bytes(nq, ny, k)
    ws = torch.empty(nbytes // 8 + 2, dtype=torch.int64, device=DEV)
    guard_d = torch.full((nq + 2, k), -77, dtype=torch.int64, device=DEV)
    guard_i = torch.full((nq + 2, k), -77, dtype=torch.int32, device=DEV)
    for _ in range(2):              # the second call overwrites the first: nothing accumulates
        _lib.check(L.otgan_nn_u8(nq, ny, D, dq.data_ptr(), D, dy.data_ptr(), D, k, -1, guard_i[1:].data_ptr(),
                                 guard_d[1:].data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()), "nn_u8")
    torch.cuda.synchronize()
    assert np.array_equal(guard_i[1:-1].cpu().numpy(), want[0]) and np.array_equal(guard_d[1:-1].cpu().numpy(), want[1])
    for r in (0, -1):
        assert bool((guard_d[r] == -77).all()) and bool((guard_i[r] == -77).all())


def test_bad_arguments():
    L = _lib.lib()
    nq, ny, D, k = 8, 12, 32, 3
    q = torch.zeros(nq, D, dtype=torch.uint8, device=DEV)
    y = torch.zeros(ny, D, dtype=torch.uint8, device=DEV)
    out_i = torch.full((nq, 8), -77, dtype=torch.int32, device=DEV)
    out_d = torch.full((nq, 8), -77, dtype=torch.int64, device=DEV)
    nbytes = L.otgan_nn_u8_workspace_bytes(nq, ny, 8)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)

    def call(nq=nq, ny=ny, D=D, qp=q.data_ptr(), ldq=D, yp=y.data_ptr(), ldy=D, k=k, self0=-1, ip=out_i.data_ptr(),
             dp=out_d.data_ptr(), wsp=ws.data_ptr(), wsb=nbytes):
        return L.otgan_nn_u8(nq, ny, D, qp, ldq, yp, ldy, k, self0, ip, dp, wsp, wsb, _lib.stream_ptr())
    bad = [dict(k=0), dict(k=9), dict(self0=-2), dict(D=24), dict(D=0), dict(D=49152 + 16, ldq=49168, ldy=49168), dict(ldq=16),
           dict(ldy=16), dict(ldq=40), dict(ldy=40), dict(nq=-1), dict(ny=-1), dict(ny=2 ** 31 - 1), dict(qp=q.data_ptr() + 4),
           dict(yp=y.data_ptr() + 8), dict(yp=None), dict(qp=None), dict(ip=None), dict(dp=None), dict(ip=out_i.data_ptr() + 2),
           dict(dp=out_d.data_ptr() + 4), dict(wsp=ws.data_ptr() + 4)]
    for kw in bad:
        assert call(**kw) == -1, kw                                        # OTGAN_ERR_INVALID
        assert "otgan_nn_u8" in _lib.lib().otgan_last_error().decode(), kw
    for kw in (dict(wsb=8), dict(wsp=None), dict(wsb=L.otgan_nn_u8_workspace_bytes(nq, ny, k) - 8)):
        assert call(**kw) == -2, kw                                        # OTGAN_ERR_WORKSPACE
        assert "workspace" in _lib.lib().otgan_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out_i == -77).all()) and bool((out_d == -77).all())
    assert call() == 0 and call(nq=0, qp=None, ip=None, dp=None) == 0 and call(ny=0, yp=None, wsp=None, wsb=0) == 0
    assert L.otgan_nn_u8_workspace_bytes(nq, ny, 0) == 0 and L.otgan_nn_u8_workspace_bytes(nq, ny, 9) == 0
    # the wrappers raise on the host, before any launch
    for args in ((q, y, 0), (q, y, 9), (q, y, 3, -2), (q, y[:, :16], 3), (q.int(), y, 3), (q[0], y, 3), (q[:, :24], y[:, :24], 3)):
        with pytest.raises(ValueError):
            authenticity.nearest(*args)
    with pytest.raises(_lib.OtganError):
        authenticity.nearest(q.cpu(), y, 3)
    with pytest.raises(_lib.OtganError):
        ops.nn_u8(q, y.cpu(), 3)


# ---------------------------------------------------------------- the score
@functools.lru_cache(maxsize=None)
def _planted():
    """96 bank images of 8 x 8 x 3; 40 queries: 10 exact copies, 10 copies with one pixel changed by 1, 20 fresh"""
    rng = np.random.default_rng(9)
    bank = rng.integers(0, 256, (96, 8, 8, 3), dtype=np.uint8)
    q = rng.integers(0, 256, (40, 8, 8, 3), dtype=np.uint8)
    src = rng.permutation(96)[:20]
    q[:20] = bank[src]
    for i in range(10, 20):
        y, x, c = rng.integers(0, 8), rng.integers(0, 8), rng.integers(0, 3)
        q[i, y, x, c] = q[i, y, x, c] + 1 if q[i, y, x, c] < 255 else 254
    order = rng.permutation(40)
    return bank, q[order]


@functools.lru_cache(maxsize=None)
def _planted_reference(k=3):
    bank, q = _planted()
    r = R.radii(bank)
    index, dist = R.nearest(q, bank, k)
    return r, index, dist, R.score(index[:, 0], dist[:, 0], r), R.sheet(q, bank, index, dist, rows=10)


def test_planted_copies():
    bank, q = _planted()
    r, index, dist, want, want_sheet = _planted_reference()
    assert 0 < want[0] <= 20 and want[1] == 10 and want[2] <= 1  # no copy is authentic, ten distances are 0, ten are 1
    dbank, dq = _dev(bank), _dev(q)
    got_r = authenticity.radii(dbank)
    assert got_r.dtype == torch.int64 and np.array_equal(got_r.cpu().numpy(), r)
    gi, gd = authenticity.nearest(dq, dbank, 3)
    assert np.array_equal(gi.cpu().numpy(), index) and np.array_equal(gd.cpu().numpy(), dist)
    assert authenticity.score(gi[:, 0], gd[:, 0], got_r) == want
    got_sheet = authenticity.sheet(dq, dbank, gi, gd, rows=10)
    assert got_sheet.dtype == np.uint8 and np.array_equal(got_sheet, want_sheet)
    state = {"epoch": 4}
    metric = authenticity.AuthenticityMetric(dbank, got_r, state)
    m = metric.measure(dq, 3)
    assert (m["authentic"], m["copies"], m["median"], m["n"]) == want + (40,)
    assert torch.equal(m["index"], gi) and torch.equal(m["dist"], gd)
    with pytest.raises(ValueError):
        authenticity.nearest(dq, dbank.view(96, -1), 3)          # the two sets in different forms


def _rank_numbers(rank, world, path):
    bank, q = _planted()
    dbank, dq = _dev(bank), _dev(q)
    r = authenticity.radii(dbank, rank, world)
    m = authenticity.AuthenticityMetric(dbank, r, {"epoch": 0}, rank, world).measure(dq, 3)
    return r.cpu(), (m["authentic"], m["copies"], m["median"], m["n"]), m["index"].cpu(), m["dist"].cpu()


def test_two_ranks_return_the_single_process_numbers():
    r, index, dist, want, _ = _planted_reference()
    one = _rank_numbers(0, 1, None)
    assert np.array_equal(one[0].numpy(), r) and one[1] == want + (40,)
    for got in H.two_ranks(_rank_numbers):
        assert torch.equal(got[0], one[0]) and got[1] == one[1] and torch.equal(got[2], one[2]) and torch.equal(got[3], one[3])
