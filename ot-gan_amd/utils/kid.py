"""Kernel Inception Distance beside the Inception score and FID, from fused fp64 kernel sums on the device.

KID (Binkowski et al., "Demystifying MMD GANs") is the unbiased estimate of the squared maximum mean discrepancy between
generated and real `pool_3` features under the cubic kernel k(a, b) = (a . b / C + 1)^3, C = the number of channels,
averaged over subsets.  Unlike FID its expectation does not depend on the sample count, so runs evaluated with different
`--eval_samples` compare.  For one subset of m generated rows X and m real rows Y:

    s0 = sum_{i != j} k(X_i, X_j),   s1 = sum_{i != j} k(Y_i, Y_j),   s2 = sum_{i, j} k(X_i, Y_j)
    MMD^2 = s0 / (m (m - 1)) + s1 / (m (m - 1)) - 2 s2 / m^2                  (may be negative; not clipped)

and KID = mean over the subsets, reported with their (population) standard deviation.  The three sums of ALL of a rank's
subsets come from one launch of csrc/kid.hip (`otgan_kid_sums_f64`: exact products on the fp64 MFMA, the map and the cube
in registers, no m x m matrix written, deterministic); both feature banks stay on the device, so generated samples
never reach the host.

Subsets: subset b draws its rows with numpy.random.default_rng([seed, side, b]).choice(n, m, replace=False), side 0 = the
generated bank, 1 = the real bank -- a draw depends only on (seed, side, b, n, m).

Ranks: every rank holds its own share of both banks (its surviving generated rows; its contiguous share of the real
images) and subset b is computed by rank b % world FROM THAT RANK'S ROWS; the per-subset values are summed into one
vector (one non-zero contributor per entry: exact) and every rank takes mean and std of the same vector.  The value
therefore depends on the world size: unlike FID, two ranks do not reproduce one process bit for bit -- they draw their
subsets from different pools of rows.  Each is an unbiased estimate of the same quantity.
"""
import numpy as np

from .. import _lib
from .features import FeatureBank, HookMetric, kernel_rows, real_bank, share    # (FeatureBank, real_bank: also this module's names)


def subset_indices(n, m, count, seed, side, first=0, step=1):
    """int32 [k, m]: the row numbers of subsets b = first, first + step, ... < count of a bank of n rows, m distinct rows
    each.  Rows [first::step] of the full table (first = 0, step = 1)."""
    n, m = int(n), int(m)
    if m > n:
        raise ValueError("a subset of %d distinct rows cannot be drawn from %d rows" % (m, n))
    if m < 1 or count < 0 or first < 0 or step < 1:
        raise ValueError("subset_indices: m %d >= 1, count %d >= 0, first %d >= 0, step %d >= 1" % (m, count, first, step))
    rows = [np.random.default_rng([int(seed), int(side), b]).choice(n, m, replace=False) for b in range(first, count, step)]
    return np.asarray(rows, np.int32).reshape(len(rows), m)


def mmd2_from_sums(sums, m):
    """The unbiased MMD^2 of each row (s0, s1, s2) of `sums` [..., 3] (numpy or torch): may be negative, returned as is."""
    m = int(m)
    if m < 2:
        raise ValueError("the unbiased estimator needs m >= 2, got %d" % m)
    return sums[..., 0] / (m * (m - 1)) + sums[..., 1] / (m * (m - 1)) - 2.0 * sums[..., 2] / (m * m)


def effective_subset_size(subset_size, eval_samples, real_samples, world=1):
    """The subset size KID can use: `subset_size`, cut to the smallest rank's surviving generated rows (the hook's `mine`)
    and to the smallest rank's share of the `real_samples` real rows.  Fewer than 2 is a ValueError."""
    gen, real = (min(hi - lo for lo, hi in (share(n, r, world) for r in range(world))) for n in (eval_samples, real_samples))
    m = min(int(subset_size), gen, real)
    if m < 2:
        raise ValueError("KID needs subsets of at least 2 rows: --kid_subset_size %d, %d generated rows and %d real rows on "
                         "the smallest rank (of %d)" % (subset_size, gen, real, world))
    return m


def _index_table(idx, rows, name):
    import torch
    t = torch.as_tensor(idx)
    if t.dtype != torch.int32 or t.dim() != 2:
        raise ValueError("%s must be int32 [nsub, m], got %s %s" % (name, t.dtype, tuple(t.shape)))
    host = t.cpu()
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= rows):
        raise IndexError("%s holds row numbers outside 0 ... %d" % (name, rows - 1))
    return t


def kid_sums(x, xi, y, yi):
    """fp64 CUDA [nsub, 3]: (s0, s1, s2) of every subset.  x, y: fp32 CUDA [rows, C] (a column slice of a wider buffer
    passes its row stride on); xi, yi: int32 [nsub, m] row numbers (numpy or torch), checked here on the host."""
    import torch
    x, y = kernel_rows(x, "x", "kid_sums"), kernel_rows(y, "y", "kid_sums")
    if x.shape[1] != y.shape[1] or x.device != y.device:
        raise ValueError("x %s and y %s must have the same channels and device" % (tuple(x.shape), tuple(y.shape)))
    xi, yi = _index_table(xi, x.shape[0], "xi"), _index_table(yi, y.shape[0], "yi")
    if xi.shape != yi.shape:
        raise ValueError("xi %s and yi %s must have the same shape" % (tuple(xi.shape), tuple(yi.shape)))
    nsub, m = xi.shape
    if m < 2:
        raise ValueError("subsets need at least 2 rows, got m = %d" % m)
    out = torch.empty(nsub, 3, dtype=torch.float64, device=x.device)
    if nsub == 0:
        return out
    xi, yi = xi.to(x.device).contiguous(), yi.to(x.device).contiguous()
    L = _lib.lib()
    for lo in range(0, nsub, 65535):             # (the subsets are a grid dimension)
        k = min(65535, nsub - lo)
        nbytes = L.otgan_kid_workspace_bytes(k, m)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(L.otgan_kid_sums_f64(k, m, x.shape[1], x.data_ptr(), x.stride(0), xi[lo:lo + k].data_ptr(),
                                            y.data_ptr(), y.stride(0), yi[lo:lo + k].data_ptr(), out[lo:lo + k].data_ptr(),
                                            ws.data_ptr(), nbytes, _lib.stream_ptr()), "kid_sums")
    return out


def kid_values(gen_bank, real_bank, subsets, m, seed, rank=0, world=1):
    """numpy fp64 [subsets]: MMD^2 of every subset, the same on every rank.  Subset b comes from rank b % world's own rows
    of both banks (one `kid_sums` launch per rank); one SUM all-reduce of the vector, each entry with one contributor."""
    import torch
    from .. import parallel
    vals = torch.zeros(int(subsets), dtype=torch.float64, device=gen_bank.device)
    xi = subset_indices(gen_bank.n, m, subsets, seed, 0, rank, world)
    yi = subset_indices(real_bank.n, m, subsets, seed, 1, rank, world)
    if xi.shape[0]:
        vals[rank::world] = mmd2_from_sums(kid_sums(gen_bank.rows, xi, real_bank.rows, yi), m)
    return parallel.allreduce_sum_([vals])[0].cpu().numpy()


def kid(gen_bank, real_bank, subsets, m, seed, rank=0, world=1):
    """(mean, std) of the subsets' MMD^2 (population std, numpy.std); see the module text for the role of the ranks."""
    v = kid_values(gen_bank, real_bank, subsets, m, seed, rank, world)
    return float(np.mean(v)), float(np.std(v))


class KidMetric(HookMetric):
    """real = the real data's FeatureBank.  (mean, std) over the subsets of the bank the hook filled: one fused kernel-sum
    launch per rank, one small all-reduce."""
    key, uses_bank, closing = "kid", True, 'min KID was %.6f, iter was %d'

    def __init__(self, *a):
        super().__init__(*a)
        if "kid_m" not in self.state:
            self.state["kid_m"] = effective_subset_size(self.args.kid_subset_size, self.args.eval_samples, self.real.total, self.world)

    def finish(self, tag, bank):
        k = kid(bank, self.real, self.args.kid_subsets, self.state["kid_m"], getattr(self.args, "seed", 1), self.rank, self.world)
        if self.rank == 0:
            print('%sKID was %.6f, std was %.6f' % (tag, k[0], k[1]))
        self.keep_minimum(k[0])
        return k
