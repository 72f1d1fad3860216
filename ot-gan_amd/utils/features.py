"""What the metrics on `pool_3` features (utils/fid.py, utils/kid.py, utils/pr.py) share: the split of rows over the
ranks, the one loop that classifies a rank's share of the real images, the device feature bank, the row check of the
fused kernels and the ragged all-gather."""
import numpy as np

from .. import _lib


def share(n, rank=0, world=1):
    """(lo, hi): rank r's contiguous share [r * ceil(n / world), (r + 1) * ceil(n / world)) of n rows, cut to n."""
    n = int(n)
    per = -(-n // world)
    return min(rank * per, n), min((rank + 1) * per, n)


def pool3_batches(classifier, images, lo, hi):
    """pool_3 (fp32 CUDA [<= batch_size, C]) of images lo ... hi - 1 in the classifier's batches.  `images`: numpy
    [N, H, W, 3] in [-1, 1], the form of train.py's `trainx`, or a `utils.data.DeviceDataset`, read through its `rows`
    (the same floats, converted on the device)."""
    import torch
    bs = classifier.batch_size
    for i in range(lo, hi, bs):
        if hasattr(images, "rows"):
            x = images.rows(i, min(i + bs, hi))
        else:
            x = torch.from_numpy(np.ascontiguousarray(images[i:min(i + bs, hi)], np.float32)).to(classifier.device)
        yield classifier.run(x, 127.5, 127.5)[0]


def kernel_rows(x, name, caller):
    """x as the fused kernels of `caller` read it: fp32 CUDA [rows, C] in 16-byte pieces of a row (a column slice of a
    wider buffer passes its row stride on; a slice that cannot be read that way is copied)."""
    import torch
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.OtganError("%s takes CUDA (MI355X) feature tensors; there is no CPU fallback" % caller)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] % 4 or x.shape[1] == 0:
        raise ValueError("%s must be float32 [rows, C] with C a positive multiple of 4, got %s %s" % (name, x.dtype, tuple(x.shape)))
    if x.stride(1) != 1 or x.stride(0) < x.shape[1] or x.stride(0) % 4 or x.data_ptr() % 16:
        x = x.contiguous()
    return x


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
    """pool_3 of the first n of `images` (pool3_batches) as a FeatureBank: rank r holds its `share` of them."""
    n = min(int(n), images.shape[0])
    lo, hi = share(n, rank, world)
    bank = FeatureBank(hi - lo, classifier.plan.pool3_channels, classifier.device, total=n)
    for rows in pool3_batches(classifier, images, lo, hi):
        bank.append(rows)
    return bank


class HookMetric:
    """One metric beside the Inception score, as train.inception_hook drives it for every evaluated model: `begin`, `take`
    the pool_3 rows of every batch that survive the cut to eval_samples, `finish` (all ranks: the collectives, the value,
    rank 0's line, the running minimum; `bank` holds the same rows for the metrics with `uses_bank`), and after the last
    model `close` (rank 0's closing line: the running minimum that `keep_minimum` keeps in state[key + "_min" / "_iter"],
    for the metrics that have a `closing` format).  Subclasses: fid.FidMetric, kid.KidMetric, pr.PrMetric."""
    key, uses_bank, closing = None, False, None

    def __init__(self, real, args, classifier, state, rank, world):
        self.real, self.args, self.classifier, self.state, self.rank, self.world = real, args, classifier, state, rank, world
        if self.closing:
            state.setdefault(self.key + "_min", float("inf"))
            state.setdefault(self.key + "_iter", 0)

    def begin(self):
        pass

    def take(self, rows):
        pass

    def keep_minimum(self, value):
        if value < self.state[self.key + "_min"]:
            self.state[self.key + "_min"], self.state[self.key + "_iter"] = value, self.state["epoch"]

    def close(self):
        if self.closing and self.rank == 0:
            print(self.closing % (self.state[self.key + "_min"], self.state[self.key + "_iter"]))


def gather_rows(x, rank=0, world=1):
    """(all ranks' rows of x in rank order, this rank's first row among them).  The shares may differ: each is padded
    to the largest for the one all-gather and cut again."""
    import torch
    from .. import parallel
    if world == 1:
        return x, 0
    counts = parallel.all_gather_rows(torch.tensor([x.shape[0]], dtype=torch.int64, device=x.device)).tolist()
    big = max(counts)
    if x.shape[0] < big:
        x = torch.cat([x, x.new_zeros((big - x.shape[0],) + tuple(x.shape[1:]))])
    allx = parallel.all_gather_rows(x)
    if min(counts) < big:
        allx = torch.cat([allx[r * big:r * big + n] for r, n in enumerate(counts)])
    return allx, sum(counts[:rank])
