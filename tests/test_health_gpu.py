"""The two kernels behind --health_every on the GPU (csrc/health.hip through ops.tensor_health / ops.plan_marginals) against the
numpy restatement tests/health_ref.py.

Bars.  tensor_health: the maxima, both counts and all 256 buckets are EXACT; the two sums within (n + 1) 2^-53 of the
math.fsum of the same fp64 terms -- the worst case of an fp64 sum of n non-negative terms in any order (the terms themselves
are the restatement's: x^2 is exact, d = x - ref and d * d are one IEEE operation each on both sides).  A segment's 6 + 256
numbers are the same BITS alone and among other segments, at the four alignments of x and ref, and from call to call.
plan_marginals: each number within (n + m + 4) 2^-53 max(1, n / m) of numpy fp64 on the same fp32 plan (a row sum of m and a
column sum of n terms of a plan whose rows sum to 1, then a mean).  The staged chain cost_log_kernels -> sinkhorn_plans ->
plan_marginals against the fp64 oracle's column error: within n 1e-4, the plan bound of tests/test_matching_gpu.py times n
for a column sum."""
import functools

import numpy as np
import pytest
import torch

import health_ref as R
from otgan_amd import ops
from otgan_amd.utils import matching
from oracle import matching_np as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK, CAP = ops.HEALTH_CHUNK, ops.HEALTH_MAX_SEGMENTS
LENGTHS = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7)
SPECIAL = np.array([-0.0, 1e-40, np.inf, np.nan, np.finfo(np.float32).max, 0.0, -np.inf, -3e-45], np.float32)


@functools.lru_cache(maxsize=None)
def _values():
    """(x, ref) of the longest length: ordinary normals over 40 binades with the special values at the front (behind one
    ordinary element), at the back and sprinkled through, at different places in x and ref.  Never written to."""
    rng = np.random.default_rng(0)
    n = max(LENGTHS)
    out = []
    for shift in (0, 5):
        v = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
        v[1 + shift:1 + shift + len(SPECIAL)] = SPECIAL
        at = rng.choice(np.arange(16, n), n // 37, replace=False)
        v[at] = SPECIAL[np.arange(len(at)) % len(SPECIAL)]
        for i, n_ in enumerate(LENGTHS):              # ... and at the last element of every length (the scalar tail)
            if n_ > 16:
                v[n_ - 1] = SPECIAL[(i + shift) % len(SPECIAL)]
        out.append(v)
    for v in out:
        v.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _want(n, with_ref):
    x, ref = _values()
    return R.tensor_health(x[:n], ref[:n] if with_ref else None)


def _at_offset(v, k):
    """v on the device, its first element k floats past a 16-byte boundary"""
    buf = torch.zeros(v.size + 4, dtype=torch.float32, device=DEV)
    view = buf[k:k + v.size]
    view.copy_(torch.from_numpy(np.array(v)))
    assert v.size == 0 or view.data_ptr() % 16 == 4 * k
    return view


def _segments(lengths, kx, kr, with_ref):
    x, ref = _values()
    xs = [_at_offset(x[:n], kx) for n in lengths]
    rs = [_at_offset(ref[:n], kr) for n in lengths] if with_ref else None
    return xs, rs


def _run(xs, rs):
    out, hist = ops.tensor_health(xs, rs)
    return out.cpu().numpy(), hist.cpu().numpy()


def _check(n, out, hist, with_ref):
    want, whist = _want(n, with_ref)
    assert np.array_equal(hist, whist), n
    assert hist.sum() + out[4] + out[5] == n
    for k in (1, 3, 4, 5):
        assert out[k] == want[k], (n, k, out[k], want[k])
    for k in (0, 2):
        err, bar = abs(out[k] - want[k]), R.sum_bound(n, want[k])
        print("n", n, "slot", k, "err", err, "bar", bar)
        assert err <= bar, (n, k, out[k], want[k])


def _bits(out, hist):
    return out.view(np.int64).tolist() + hist.tolist()


def test_the_values_hold_every_class():
    x, ref = _values()
    for v in (x, ref):
        assert np.isnan(v).any() and np.isinf(v).any() and (v == 0).any() and (np.abs(v[v != 0]) < 1e-38).any()
    assert (np.isfinite(x) & ~np.isfinite(ref)).any()


@pytest.mark.parametrize("kx", [0, 1, 2, 3])
@pytest.mark.parametrize("with_ref", [False, True], ids=["no-ref", "ref"])
def test_tensor_health_against_reference(kx, with_ref):
    xs, rs = _segments(LENGTHS, kx, (kx + 1) % 4, with_ref)       # x and ref at different alignments
    out, hist = _run(xs, rs)
    assert out.shape == (len(LENGTHS), 6) and hist.shape == (len(LENGTHS), 256) and hist.dtype == np.int64
    for i, n in enumerate(LENGTHS):
        _check(n, out[i], hist[i], with_ref)
    if not with_ref:
        assert (out[:, 2:4] == 0).all()


def test_null_entries_inside_ref():
    xs, rs = _segments(LENGTHS, 2, 0, True)
    rs = [r if i % 3 else None for i, r in enumerate(rs)]
    out, hist = _run(xs, rs)
    for i, n in enumerate(LENGTHS):
        _check(n, out[i], hist[i], i % 3 != 0)


def test_same_bits_alone_among_others_aligned_or_not_and_again():
    xs, rs = _segments(LENGTHS, 0, 0, True)
    together = _run(xs, rs)
    again = _run(xs, rs)
    assert _bits(*together) == _bits(*again)
    for kx in range(4):
        for kr in {kx, (kx + 3) % 4}:
            xs, rs = _segments(LENGTHS, kx, kr, True)
            for i, n in enumerate(LENGTHS):
                out, hist = _run([xs[i]], [rs[i]])
                assert _bits(out[0], hist[0]) == _bits(together[0][i], together[1][i]), (n, kx, kr)
    # in another order and beside other neighbours
    order = list(range(len(LENGTHS)))[::-1]
    out, hist = _run([xs[i] for i in order], [rs[i] for i in order])
    assert _bits(out[::-1].copy(), hist[::-1].copy()) == _bits(*together)


@pytest.mark.parametrize("nseg", [1, CAP, CAP + 1, 2 * CAP + 3])
def test_any_number_of_segments(nseg):
    some = (CHUNK + 1, 0, 5, 1025, 3 * CHUNK + 7, 256, 1)
    lengths = [some[i % len(some)] for i in range(nseg)]
    xs, rs = _segments(some, 1, 2, True)
    pick = lambda lst: [lst[i % len(some)] for i in range(nseg)]
    out, hist = _run(pick(xs), pick(rs))
    alone = [_run([x], [r]) for x, r in zip(xs, rs)]
    for i, n in enumerate(lengths):
        _check(n, out[i], hist[i], True)
        a = alone[i % len(some)]
        assert _bits(out[i], hist[i]) == _bits(a[0][0], a[1][0]), i


def test_host_checks():
    from otgan_amd import _lib
    x = torch.ones(8, device=DEV)
    with pytest.raises(ValueError):
        ops.tensor_health([x], [x, x])
    with pytest.raises(ValueError):
        ops.tensor_health([x], [x[:4]])
    with pytest.raises(ValueError):
        ops.tensor_health([x.double()])
    with pytest.raises(_lib.OtganError):
        ops.tensor_health([x], [x.cpu()])
    with pytest.raises(ValueError):
        ops.plan_marginals(x)
    # a tensor that is not contiguous is read through a copy: the same numbers
    y = torch.arange(24, dtype=torch.float32, device=DEV).reshape(4, 6)
    a, b = _run([y.t()], None), _run([y], None)
    assert _bits(*a) == _bits(*b)


# ---------------------------------------------------------------- plan_marginals
@functools.lru_cache(maxsize=None)
def _plans(P, n, m):
    rng = np.random.default_rng(P * 1000003 + n * 1009 + m)
    p = rng.random((P, n, m), dtype=np.float32) + np.float32(1e-3)
    p /= p.sum(2, keepdims=True, dtype=np.float32)                # rows sum to 1 like a plan's, to fp32 rounding
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("P,n,m,pad", [(1, 1, 1, 0), (6, 24, 24, 0), (3, 128, 128, 0), (1, 129, 257, 0), (2, 1000, 40, 0),
                                       (1, 33, 1024, 0), (3, 128, 128, 3), (1, 129, 257, 3)])
def test_plan_marginals(P, n, m, pad):
    p = _plans(P, n, m)
    buf = torch.full((P, n, m + pad), 7.0, dtype=torch.float32, device=DEV)       # the padding must not be read
    buf[:, :, :m] = torch.from_numpy(np.array(p))
    plan = buf[:, :, :m]
    assert plan.stride(1) == m + pad
    got = ops.plan_marginals(plan)
    again = ops.plan_marginals(plan)
    assert got.dtype == torch.float64 and tuple(got.shape) == (P, 4)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    got = got.cpu().numpy()
    bar = R.marginals_bound(n, m)
    for q in range(P):
        want = R.plan_marginals(p[q])
        print("P n m", P, n, m, "err", np.abs(got[q] - want).max(), "bar", bar)
        assert (np.abs(got[q] - want) <= bar).all(), (q, got[q], want)
    if P > 1:                                                     # a problem's numbers do not depend on its neighbours
        one = ops.plan_marginals(plan[1])
        assert torch.equal(one.view(torch.int64)[0].cpu(), torch.from_numpy(got[1].view(np.int64)))


@pytest.mark.parametrize("iters,shown", [(3, 1.309e-1), (10, 7.07e-4), (100, 4e-16)])
def test_staged_chain_against_the_oracle(iters, shown):
    n, D, lam = 24, 16, 10.0
    rng = np.random.default_rng(0)
    unit = lambda: (lambda z: (z / np.linalg.norm(z, axis=1, keepdims=True)).astype(np.float32))(rng.standard_normal((n, D)))
    x, y = unit(), unit()
    plan = M.sinkhorn_plan(M.cosine_cost(x.astype(np.float64), y.astype(np.float64)), lam, iters)[0]
    want = np.abs(plan.sum(0) - 1.0).max()
    assert abs(want - shown) <= 1e-3 * shown + 1e-15            # the oracle's own figure, as recorded
    K = matching.cost_log_kernels([torch.from_numpy(x).to(DEV)], [torch.from_numpy(y).to(DEV)], lam)
    got = ops.plan_marginals(matching.sinkhorn_plans(K, lam, iters)).cpu().numpy()[0]
    print("L", iters, "column error", got[2], "oracle", want, "row error", got[0])
    assert abs(got[2] - want) <= n * 1e-4
    # rows sum to 1 (the plan is the row softmax of the last sweep) to the 5e-6 tests/test_matching_gpu.py holds row sums to
    assert got[0] <= 5e-6 and got[1] <= got[0] and got[3] <= got[2]
