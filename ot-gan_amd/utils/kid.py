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
    share = -(-int(eval_samples) // world)
    gen = min(min(max(int(eval_samples) - r * share, 0), share) for r in range(world))
    per = -(-int(real_samples) // world)
    real = min(min((r + 1) * per, int(real_samples)) - min(r * per, int(real_samples)) for r in range(world))
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


def _rows(x, name):
    import torch
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.OtganError("kid_sums takes CUDA (MI355X) feature tensors; there is no CPU fallback")
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] % 4 or x.shape[1] == 0:
        raise ValueError("%s must be float32 [rows, C] with C a positive multiple of 4, got %s %s" % (name, x.dtype, tuple(x.shape)))
    # the kernel reads 16-byte pieces of a row: a slice it cannot read that way is copied
    if x.stride(1) != 1 or x.stride(0) < x.shape[1] or x.stride(0) % 4 or x.data_ptr() % 16:
        x = x.contiguous()
    return x


def kid_sums(x, xi, y, yi):
    """fp64 CUDA [nsub, 3]: (s0, s1, s2) of every subset.  x, y: fp32 CUDA [rows, C] (a column slice of a wider buffer
    passes its row stride on); xi, yi: int32 [nsub, m] row numbers (numpy or torch), checked here on the host."""
    import torch
    x, y = _rows(x, "x"), _rows(y, "y")
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


class FeatureBank:
    """A preallocated fp32 [rows, C] device buffer that `append` fills with pool_3 rows; it never leaves the device.
    `total`: the rows of the same bank over all ranks (the bank itself holds this rank's)."""

    def __init__(self, rows, C, device="cuda", total=None):
        import torch
        self.C, self.device = int(C), torch.device(device)
        if self.device.type != "cuda":
            raise _lib.OtganError("FeatureBank lives on a CUDA (MI355X) device; there is no CPU fallback")
        self.buf = torch.empty(int(rows), self.C, dtype=torch.float32, device=self.device)
        self.n = 0
        self.total = int(rows) if total is None else int(total)

    def append(self, x):
        import torch
        if not (torch.is_tensor(x) and x.is_cuda):
            raise _lib.OtganError("FeatureBank.append takes CUDA (MI355X) tensors; there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.C or x.dtype != torch.float32:
            raise ValueError("features must be float32 [n, %d], got %s %s" % (self.C, x.dtype, tuple(x.shape)))
        if self.n + x.shape[0] > self.buf.shape[0]:
            raise ValueError("%d more rows do not fit a bank of %d holding %d" % (x.shape[0], self.buf.shape[0], self.n))
        self.buf[self.n:self.n + x.shape[0]].copy_(x)
        self.n += x.shape[0]
        return self

    def clear(self):
        self.n = 0
        return self

    @property
    def rows(self):
        """the filled part, fp32 [n, C]"""
        return self.buf[:self.n]


def real_bank(classifier, images, n, rank=0, world=1):
    """pool_3 of the first n of `images` -- numpy [N, H, W, 3] in [-1, 1] or a `utils.data.DeviceDataset`, read as
    `fid.dataset_stats` reads them -- as a FeatureBank: rank r holds the contiguous share
    [r * ceil(n / world), (r + 1) * ceil(n / world))."""
    import torch
    n = min(int(n), images.shape[0])
    per = -(-n // world)
    lo, hi = min(rank * per, n), min((rank + 1) * per, n)
    bank = FeatureBank(hi - lo, classifier.plan.pool3_channels, classifier.device, total=n)
    bs = classifier.batch_size
    for i in range(lo, hi, bs):
        if hasattr(images, "rows"):
            x = images.rows(i, min(i + bs, hi))
        else:
            x = torch.from_numpy(np.ascontiguousarray(images[i:min(i + bs, hi)], np.float32)).to(classifier.device)
        bank.append(classifier.run(x, 127.5, 127.5)[0])
    return bank


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
