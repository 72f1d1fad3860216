"""numpy fp64 restatement of precision, recall, density and coverage (otgan_amd/utils/pr.py, csrc/knn.hip), brute force:
every squared distance is ((a - b)^2).sum() -- NOT the expanded form the kernel uses --, the radius of a row is the K-th
smallest distance to the other rows of its set BY POSITION, and the four values are quotients of integer counts.  Shared
by tests/test_pr_cpu.py and tests/test_pr_gpu.py."""
import numpy as np


def dist2(A, B):
    """fp64 [na, nb]: ((a - b)^2).sum() of every pair, a row of A at a time."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for i, a in enumerate(A):
        out[i] = ((a - B) ** 2).sum(axis=1)
    return out


def error_bound(A, B):
    """fp64 [na, nb]: 2 (C + 8) 2^-53 (|a| + |b|)^2 per pair, the bar between the kernel's d2 = max(0, (a.a + b.b) - 2 a.b)
    and dist2.  Derivation, u = 2^-53: products of fp32 values are exact in fp64; a dot product of C exact products,
    added in any order, is off by at most C u sum |a_i b_i| <= C u |a| |b| (Cauchy-Schwarz), and the two norms by
    C u |a|^2 and C u |b|^2: together C u (|a|^2 + |b|^2 + 2 |a| |b|) = C u (|a| + |b|)^2, the doubling of a.b being exact.
    The addition of the norms and the subtraction round once each, at most u (|a| + |b|)^2 apiece; the clamp at 0 only
    moves a value towards the true one, which is >= 0.  8 covers those two roundings and the second-order terms.  The
    factor 2 covers this reference: C subtractions, squarings and additions whose errors sum to at most
    (C + 3) u |a - b|^2 <= (C + 3) u (|a| + |b|)^2.  The K-th smallest of a row moves by at most the largest bar of the row."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    na, nb = np.sqrt((A * A).sum(axis=1)), np.sqrt((B * B).sum(axis=1))
    return 2.0 * (A.shape[1] + 8.0) * 2.0 ** -53 * (na[:, None] + nb[None, :]) ** 2


def counted(nq, ny, self0):
    """bool [nq, ny]: the columns row i takes -- all but column self0 + i (self0 = -1: all)."""
    m = np.ones((nq, ny), bool)
    if self0 >= 0:
        for i in range(nq):
            if 0 <= self0 + i < ny:
                m[i, self0 + i] = False
    return m


def knn(q, y, k, self0=-1, thresh=None, d=None):
    """(nearest fp64 [nq, k] ascending with +inf where fewer than k columns count, inside int64 [nq] or None)."""
    d = dist2(q, y) if d is None else d
    m = counted(d.shape[0], d.shape[1], self0)
    near = np.sort(np.where(m, d, np.inf), axis=1)[:, :k]
    if near.shape[1] < k:
        near = np.concatenate([near, np.full((d.shape[0], k - near.shape[1]), np.inf)], axis=1)
    inside = None if thresh is None else (m & (d <= np.asarray(thresh)[None, :])).sum(axis=1)
    return near, inside


def radii(S, k):
    """fp64 [n]: the k-th smallest distance of every row to the other rows of S."""
    return knn(S, S, k, self0=0)[0][:, k - 1]


def counts(G, R, k):
    """The six integers of utils.pr.counts: generated rows inside some real ball, real rows inside some generated ball,
    the real balls around the generated rows summed, real rows whose nearest generated row is inside their own ball, Ng, Nr."""
    d = dist2(G, R)
    rg, rr = radii(G, k), radii(R, k)
    in_real = (d <= rr[None, :]).sum(axis=1)
    in_gen = (d.T <= rg[None, :]).sum(axis=1)
    return (int((in_real > 0).sum()), int((in_gen > 0).sum()), int(in_real.sum()), int((d.min(axis=0) <= rr).sum()),
            d.shape[0], d.shape[1])


def values(G, R, k):
    """(precision, recall, density, coverage): quotients of the integer counts, as Python floats."""
    p, r, dn, c, ng, nr = counts(G, R, k)
    return p / ng, r / nr, dn / (k * ng), c / nr


def margin(G, R, k, bound=None):
    """The smallest |d2 - threshold| / bar over every comparison the four values make: d2(g, r) against the radius of r,
    d2(r, g) against the radius of g.  `bound`: the bar per pair [Ng, Nr], error_bound by default.  A radius is itself
    off by at most the largest bar of its row, which the caller's factor has to cover."""
    d = dist2(G, R)
    bar = error_bound(G, R) if bound is None else bound
    rg, rr = radii(G, k), radii(R, k)
    return float(min((np.abs(d - rr[None, :]) / bar).min(), (np.abs(d - rg[:, None]) / bar).min()))
