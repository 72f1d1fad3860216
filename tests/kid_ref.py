"""numpy fp64 restatement of the Kernel Inception Distance (otgan_amd/utils/kid.py, csrc/kid.hip), brute force: the three
Gram matrices of a subset are formed in full, pushed through the cubic kernel element by element and summed; the diagonal
is dropped by POSITION.  Shared by tests/test_kid_cpu.py and tests/test_kid_gpu.py."""
import numpy as np


def _kernel(a, b, C):
    return (a.astype(np.float64) @ b.astype(np.float64).T / C + 1.0) ** 3


def kernel_sums(X, Y, with_diagonal=False):
    """(s0, s1, s2) of the rows X [m, C], Y [m, C]: s0 = sum_{i != j} k(X_i, X_j), s1 the same for Y, s2 = sum_{i, j}
    k(X_i, Y_j), k(a, b) = (a . b / C + 1)^3.  `with_diagonal`: s0 and s1 over all i, j (what a kernel that forgot the
    mask would return)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    C = X.shape[1]
    kxx, kyy, kxy = _kernel(X, X, C), _kernel(Y, Y, C), _kernel(X, Y, C)
    if not with_diagonal:
        kxx, kyy = kxx.copy(), kyy.copy()
        np.fill_diagonal(kxx, 0.0)
        np.fill_diagonal(kyy, 0.0)
    return np.array([kxx.sum(), kyy.sum(), kxy.sum()])


def abs_sums(X, Y):
    """The same three sums over the absolute-valued rows with (|X_i| . |Y_j| / C + 1)^3: the scale of the error bound."""
    return kernel_sums(np.abs(np.asarray(X, np.float64)), np.abs(np.asarray(Y, np.float64)))


def error_bound(X, Y):
    """Per output: 2 (3 C + P + 8) 2^-53 sum (|X_i| . |Y_j| / C + 1)^3 over the counted pairs.  Products of fp32 values are
    exact in fp64; a dot product takes at most C additions and the cube triples its relative error; P summed terms add at
    most P u in any order; 8 covers the division, the + 1 and the two multiplies of the cube; the factor 2 covers the
    rounding of this reference."""
    m, C = np.asarray(X).shape
    P = np.array([m * (m - 1), m * (m - 1), m * m], np.float64)
    return 2.0 * (3.0 * C + P + 8.0) * 2.0 ** -53 * abs_sums(X, Y)


def mmd2(sums, m):
    return sums[0] / (m * (m - 1)) + sums[1] / (m * (m - 1)) - 2.0 * sums[2] / (m * m)


def scale(sums, m):
    """s0 / (m (m - 1)) + s1 / (m (m - 1)) + 2 s2 / m^2: the size of the terms whose difference MMD^2 is."""
    return sums[0] / (m * (m - 1)) + sums[1] / (m * (m - 1)) + 2.0 * sums[2] / (m * m)


def subset_sums(x, xi, y, yi, with_diagonal=False):
    """[nsub, 3]: kernel_sums of the rows x[xi[s]], y[yi[s]] of every subset s."""
    return np.array([kernel_sums(np.asarray(x)[a], np.asarray(y)[b], with_diagonal) for a, b in zip(xi, yi)]).reshape(len(xi), 3)


def kid_values(x, xi, y, yi):
    """MMD^2 of every subset and its scale: ([nsub], [nsub])."""
    m = np.asarray(xi).shape[1]
    s = subset_sums(x, xi, y, yi)
    return np.array([mmd2(r, m) for r in s]), np.array([scale(r, m) for r in s])
