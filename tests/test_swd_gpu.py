"""GPU: the device stages of the sliced Wasserstein distance (csrc/swd.hip through ops.swd_* and utils/swd.py) against the fp64
restatement tests/swd_ref.py.  Every case prints its worst error."""
import functools

import numpy as np
import pytest
import torch

import swd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ND = 130


def _images(seed, n, S):
    return np.random.RandomState(seed).randint(0, 256, (n, S, S, 3)).astype(np.uint8)


def _corner(S, k):
    return ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1))[k]


def _kind(kind, n, S):
    if kind == "random":
        return _images(10 * S + n, n, S)
    if kind == "zeros":
        return np.zeros((n, S, S, 3), np.uint8)
    if kind == "full":
        return np.full((n, S, S, 3), 255, np.uint8)
    img = np.zeros((n, S, S, 3), np.uint8)          # "corner<k>": image i has one 255 pixel, in corner (k + i) % 4, channel i % 3
    for i in range(n):
        y, x = _corner(S, (int(kind[-1]) + i) % 4)
        img[i, y, x, i % 3] = 255
    return img


@pytest.mark.parametrize("kind", ["random", "zeros", "full", "corner0", "corner1", "corner2", "corner3"])
@pytest.mark.parametrize("S", [16, 32, 64])
@pytest.mark.parametrize("n", [1, 3])
def test_pyramid(n, S, kind):
    """Every level of the device pyramid against fp64, 1e-4 absolute: uint8 inputs and dyadic taps make every stage exact in
    fp32 but up() of the 16 x 16 level at S = 64 (30-bit numerators), a handful of roundings at |v| <= 255, ulp 1.5e-5.
    Measured on the MI355X: exactly 0 everywhere except level 1 at S = 64 with random images, worst case 2.12e-5."""
    from otgan_amd import ops
    img = _kind(kind, n, S)
    ref = R.pyramid(img)
    d = torch.from_numpy(img).to(DEV)
    for l, want in enumerate(ref):
        got = ops.swd_pyramid(d, l)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, S >> l, S >> l, 3)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print("pyramid n %d S %d %s level %d: worst %.3g" % (n, S, kind, l, err))
        assert err <= 1e-4


def test_unsupported_size_and_bad_level():
    from otgan_amd import _lib, ops
    for S in (8, 48, 128):
        with pytest.raises(ValueError):
            ops.swd_pyramid(torch.zeros(1, S, S, 3, dtype=torch.uint8, device=DEV), 0)
    # the library itself: OTGAN_ERR_UNSUPPORTED (-4) before any launch
    x = torch.zeros(1, 48, 48, 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1, 48, 48, 3, device=DEV)
    assert _lib.lib().otgan_swd_pyramid_u8(x.data_ptr(), 1, 48, 0, out.data_ptr(), _lib.stream_ptr()) == -4
    with pytest.raises(ValueError):
        ops.swd_pyramid(torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=DEV), 2)


def _positions(seed, n, S, P):
    """random positions whose first patch slots are the four extreme corners of every level"""
    from otgan_amd.utils import swd
    pos = swd.positions(n, S, P, torch.Generator().manual_seed(seed)).numpy().copy()
    for l in range(pos.shape[0]):
        m = (S >> l) - 7
        flat = pos[l].reshape(n * P, 2)
        for k, c in enumerate(((0, 0), (0, m), (m, 0), (m, m))[:n * P]):
            flat[k] = c
    return pos


@functools.lru_cache(maxsize=None)
def _case(S, n, P):
    """One shared reference per (S, n, P): images, positions, directions, fp64 statistics and projections on ND directions."""
    from otgan_amd.utils import swd
    img, pos = _images(S + n + P, n, S), _positions(S + n, n, S, P)
    dirs = swd.directions(1, ND, torch.Generator().manual_seed(P)).numpy()
    pyr = R.pyramid(img)
    stats = [R.channel_stats(R.descriptors(pyr[l], pos[l])) for l in range(len(pyr))]
    return img, pos, dirs, stats, R.projections(img, pos, dirs)


@pytest.mark.parametrize("P", [1, 5, 128])
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("S", [16, 32, 64])
def test_channel_stats(S, n, P):
    """mean and 1 / std of every level and channel against fp64, 1e-6 relative (the outputs are fp32 roundings of fp64 values:
    6e-8; the variance is a difference of fp64 moments).  Measured on the MI355X: mean 5.6e-8, 1 / std 3.4e-8 at worst.  (From the
    fp32 pyramid the mean of level 1 at S = 64, a small difference of large sums, was 3.7e-5 off: the kernel builds its
    pyramid in fp64.)  Presenting the same images in another order gives the same bits: the sums over the images are exact."""
    from otgan_amd import ops
    img, pos, _, stats, _ = _case(S, n, P)
    d_img, d_pos = torch.from_numpy(img).to(DEV), torch.from_numpy(pos).to(DEV)
    mean, inv_std = ops.swd_channel_stats(d_img, d_pos)
    want_mean = np.stack([s[0] for s in stats])
    want_inv = 1.0 / np.stack([s[1] for s in stats])
    assert np.all(want_mean != 0.0)
    e_mean = float((np.abs(mean.cpu().numpy().astype(np.float64) - want_mean) / np.abs(want_mean)).max())
    e_inv = float((np.abs(inv_std.cpu().numpy().astype(np.float64) - want_inv) / want_inv).max())
    print("stats S %d n %d P %d: mean %.3g relative, 1/std %.3g relative" % (S, n, P, e_mean, e_inv))
    assert e_mean <= 1e-6 and e_inv <= 1e-6
    perm = np.random.RandomState(n).permutation(n)
    mean2, inv2 = ops.swd_channel_stats(torch.from_numpy(img[perm]).to(DEV), torch.from_numpy(np.ascontiguousarray(pos[:, perm])).to(DEV))
    assert torch.equal(mean, mean2) and torch.equal(inv_std, inv2)


def test_zero_spread_is_loud():
    from otgan_amd import ops
    from otgan_amd.utils import swd
    g = torch.Generator().manual_seed(0)
    img = torch.full((2, 16, 16, 3), 9, dtype=torch.uint8, device=DEV)
    pos, dirs = swd.positions(2, 16, 3, g).to(DEV), swd.directions(1, 2, g).to(DEV)
    mean, inv_std = ops.swd_channel_stats(img, pos)
    assert torch.equal(mean, torch.full_like(mean, 9.0)) and bool(torch.isinf(inv_std).all())
    assert bool(torch.isnan(ops.swd_project(img, pos, 0, mean, inv_std, dirs)).all())


@pytest.mark.parametrize("P", [1, 5, 128])
@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("S", [16, 32, 64])
def test_projections(S, n, P):
    """proj[j][i P + p] against fp64 for nd in {1, 3, 128, 130}, 1e-4 absolute on values of unit variance by construction: 147
    products whose magnitudes sum to about 45 at 6e-8 each, worst case 2.7e-6; an fp32 emulation measured 2.5e-6.  Measured on
    the MI355X: worst 2.47e-6 over all cases, a fortieth of the bound.  The rows are longer than n P: the guard band stays
    untouched.  Bit-identity: any split of the images into calls, any split of the directions and any co-batching give the
    same bits per element."""
    from otgan_amd import ops
    img, pos, dirs, _, ref = _case(S, n, P)
    d_img, d_pos, d_dirs = torch.from_numpy(img).to(DEV), torch.from_numpy(pos).to(DEV), torch.from_numpy(dirs).to(DEV)
    mean, inv_std = ops.swd_channel_stats(d_img, d_pos)
    L, guard, worst = len(ref), 5, 0.0
    for l in range(L):
        whole = None
        for nd in (1, 3, 128, 130):
            out = torch.full((nd, n * P + guard), 12345.0, device=DEV)
            got = ops.swd_project(d_img, d_pos, l, mean, inv_std, d_dirs[:nd].contiguous(), out=out)
            assert got is out
            assert bool((out[:, n * P:] == 12345.0).all())
            err = float(np.abs(out[:, :n * P].cpu().numpy().astype(np.float64) - ref[l][:nd]).max())
            worst = max(worst, err)
            assert err <= 1e-4, (l, nd, err)
            if whole is not None:
                assert torch.equal(out[:whole.shape[0], :n * P], whole)   # a direction's bits do not depend on nd
            whole = out[:, :n * P].clone()
        # directions split into two calls
        parts = [ops.swd_project(d_img, d_pos, l, mean, inv_std, d_dirs[a:b].contiguous()) for a, b in ((0, 65), (65, 130))]
        assert torch.equal(torch.cat(parts), whole)
        # images split into calls (every cut), each call with its own positions, into one output
        for cut in range(1, n):
            out = torch.full((ND, n * P + guard), 12345.0, device=DEV)
            ops.swd_project(d_img[:cut], d_pos[:, :cut].contiguous(), l, mean, inv_std, d_dirs, out=out)
            ops.swd_project(d_img[cut:], d_pos[:, cut:].contiguous(), l, mean, inv_std, d_dirs, out=out, col0=cut * P)
            assert torch.equal(out[:, :n * P], whole) and bool((out[:, n * P:] == 12345.0).all())
        # co-batching: the last image beside other images and in another place
        if n > 1:
            order = [n - 1] + list(range(n - 1))
            mixed = ops.swd_project(d_img[order].contiguous(), d_pos[:, order].contiguous(), l, mean, inv_std, d_dirs)
            assert torch.equal(mixed[:, :P], whole[:, (n - 1) * P:])
    print("projections S %d n %d P %d: worst %.3g" % (S, n, P, worst))


@pytest.mark.parametrize("m", [1, 255, 4096, 70001])
def test_distance_stage(m):
    """From given fp32 projections, torch.sort + the fp64 row kernel against numpy fp64 on the same values: 1e-9 relative.
    Rows with ties (values on a coarse grid), equal rows and a row against its reverse."""
    from otgan_amd import ops
    rng = np.random.RandomState(m)
    a = rng.randn(6, m).astype(np.float32)
    b = rng.randn(6, m).astype(np.float32)
    a[1], b[1] = np.round(a[1] * 2) / 2, np.round(b[1] * 2) / 2          # many ties
    b[2] = a[2]                                                          # the same multiset: exactly 0
    b[3] = a[3][::-1]
    a[4] = 0.0
    want = np.abs(np.sort(a.astype(np.float64), axis=1) - np.sort(b.astype(np.float64), axis=1)).mean(axis=1)
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = ops.swd_row_l1(torch.sort(da, dim=1)[0], torch.sort(db, dim=1)[0]).cpu().numpy()
    err = float((np.abs(got - want) / np.maximum(want, 1e-300)).max())
    print("distance stage m %d: worst relative %.3g" % (m, err))
    assert got[2] == 0.0 and got[3] == 0.0
    assert err <= 1e-9
    # rows of a wider buffer
    wide_a, wide_b = torch.sort(da, dim=1)[0], torch.sort(db, dim=1)[0]
    pad = torch.zeros(6, m + 3, device=DEV)
    pad[:, :m] = wide_a
    assert torch.equal(ops.swd_row_l1(pad[:, :m], wide_b), torch.from_numpy(got).to(DEV))


@pytest.mark.parametrize("S", [32, 64])
def test_end_to_end(S):
    """utils.swd.distances on two sets of 64 random uint8 images, the second the first plus noise in +-20, against swd_ref.
    Sorting is 1-Lipschitz in the sup norm, so a level's distance moves by at most 1e3 (e_A + e_B) with e the measured worst
    projection error of each side at that level.  Measured on the MI355X: e = 1.6e-6 ... 2.6e-6 per side, bounds of 3.2e-3 ... 4.7e-3, and
    the distances differ by 1.3e-6 ... 3.5e-6 on four of the five levels and by 1.2e-4 on the 16 x 16 level at S = 64.  A set compared with itself gives exactly 0."""
    from otgan_amd import ops
    from otgan_amd.utils import swd
    n, P = 64, 16
    rng = np.random.RandomState(S)
    A = rng.randint(0, 256, (n, S, S, 3)).astype(np.uint8)
    B = np.clip(A.astype(np.int64) + rng.randint(-20, 21, A.shape), 0, 255).astype(np.uint8)
    g = torch.Generator().manual_seed(S)
    pos_a, pos_b, dirs = swd.positions(n, S, P, g), swd.positions(n, S, P, g), swd.directions(2, 8, g)
    dA, dB = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    real = swd.SwdReal(dA, pos_a, dirs, pos_gen=pos_b)
    table = swd.distances(dB, real)
    assert table.dtype == torch.float64 and tuple(table.shape) == (swd.levels(S), 16)
    got = table.mean(dim=1).cpu().numpy()
    ref_a, ref_b = R.projections(A, pos_a.numpy(), dirs.numpy()), R.projections(B, pos_b.numpy(), dirs.numpy())
    want = np.array([1e3 * R.row_distance(a, b).mean() for a, b in zip(ref_a, ref_b)])
    for l in range(len(want)):
        e = []
        for img, pos, ref in ((dA, pos_a, ref_a), (dB, pos_b, ref_b)):
            mean, inv_std = ops.swd_channel_stats(img, pos.to(DEV))
            proj = ops.swd_project(img, pos.to(DEV), l, mean, inv_std, dirs.to(DEV))
            e.append(float(np.abs(proj.cpu().numpy().astype(np.float64) - ref[l]).max()))
        bound = 1e3 * (e[0] + e[1])
        print("end to end S %d level %d: device %.6f reference %.6f, |difference| %.3g, bound 1e3 (%.3g + %.3g) = %.3g"
              % (S, l, got[l], want[l], abs(got[l] - want[l]), e[0], e[1], bound))
        assert abs(got[l] - want[l]) <= bound
    # a split of the directions gives the columns of the whole table
    halves = [swd.distances(dB, real, dir_range=r) for r in ((0, 5), (5, 16))]
    assert torch.equal(torch.cat(halves, dim=1), table)
    # chunked sorts: one direction at a time
    one_by_one = torch.cat([rows for _, rows in swd.sorted_projections(dA, pos_a.to(DEV), dirs.to(DEV), 0, chunk=1)])
    assert torch.equal(one_by_one, real.sorted[0])
    # a real side that keeps a part of the directions
    small = swd.SwdReal(dA, pos_a, dirs, pos_gen=pos_a, dir_range=(3, 9))
    assert torch.equal(small.sorted[0], real.sorted[0][3:9])
    same = swd.distances(dA, small)
    assert tuple(same.shape) == (swd.levels(S), 6) and bool((same == 0.0).all())
