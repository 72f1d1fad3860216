"""Frechet Inception Distance beside the Inception score, from additive fp64 feature moments.

FID is defined on `pool_3:0` of the 2015 Inception graph -- the tensor `InceptionNet.run` already produces for the
score -- and needs only its mean and covariance.  Each rank keeps two fp64 moments on the device,
sum = sum_k x_k and outer = sum_k x_k x_k^T (csrc/moments.hip, `otgan_moments_update_f64`: exact products on the fp64
MFMA, deterministic), and the ranks SUM-reduce them once: 8 (C + C^2 + 1) bytes = 33.6 MB at C = 2048 whatever the
number of samples, against 410 MB for gathering 50 000 x 2048 features.  Everything after the reduction runs on the
host in fp64:

    mu = sum / n,   sigma = (outer - n mu mu^T) / (n - 1)            (np.cov's divisor, as the circulated stats files)
    d^2 = |mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr sqrt(sigma1 sigma2)

with tr sqrt(sigma1 sigma2) = sum sqrt(eig(R sigma2 R)), R = sigma1^(1/2) from `eigh` (eigenvalues clipped at 0): the
eigenvalues of sigma1 sigma2 are those of the symmetric positive semi-definite R sigma2 R, so the value stays real
and stable for rank-deficient covariances (fewer samples than channels, dead ReLU channels) where `sqrtm` needs an
epsilon fallback.

Stats files: `.npz` with `mu` [C] and `sigma` [C, C] in float64 -- the key names of the circulated `fid_stats_*.npz`
files, which therefore load as they are -- plus the sample count `n`.

    python -m otgan_amd.utils.fid --data_dir D --inception_model M --out stats.npz     # CIFAR-10 training set statistics
"""
import numpy as np

from .. import _lib
from . import features


class MomentAccumulator:
    """fp64 device buffers `sum` [C], `outer` [C, C] and a row count; batches of fp32 features stream through
    `update`."""

    def __init__(self, C, device="cuda"):
        import torch
        self.C, self.device = int(C), torch.device(device)
        if self.device.type != "cuda":
            raise _lib.OtganError("MomentAccumulator runs on CUDA (MI355X) tensors; there is no CPU fallback")
        self.sum = torch.zeros(self.C, dtype=torch.float64, device=self.device)
        self.outer = torch.zeros(self.C, self.C, dtype=torch.float64, device=self.device)
        self.n = 0

    def update(self, x):
        """x: fp32 CUDA [n, C]; rows may be a column slice of a wider buffer (the row stride goes to the kernel)."""
        import torch
        if not (torch.is_tensor(x) and x.is_cuda):
            raise _lib.OtganError("MomentAccumulator.update takes CUDA (MI355X) tensors; there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.C or x.dtype != torch.float32:
            raise ValueError("features must be float32 [n, %d], got %s %s" % (self.C, x.dtype, tuple(x.shape)))
        n = x.shape[0]
        if n == 0:
            return self
        if x.stride(1) != 1 or x.stride(0) < self.C:
            x = x.contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().otgan_moments_update_f64(n, self.C, x.stride(0), x.data_ptr(), self.sum.data_ptr(),
                                                           self.outer.data_ptr(), _lib.stream_ptr()), "moments_update")
        self.n += n
        return self

    def all_reduce(self):
        """SUM over the ranks of count, sum and outer: one collective (parallel.allreduce_sum_)."""
        import torch
        from .. import parallel
        cnt = torch.tensor([float(self.n)], dtype=torch.float64, device=self.device)
        s, o, cnt = parallel.allreduce_sum_([self.sum, self.outer, cnt])
        self.sum, self.outer, self.n = s, o, int(round(float(cnt)))
        return self

    def moments(self):
        """-> host numpy (n, sum [C], outer [C, C])"""
        return self.n, self.sum.cpu().numpy(), self.outer.cpu().numpy()


def stats_from_moments(n, sum, outer):
    """(mu, sigma) of n rows from their moments; sigma with the n - 1 divisor of np.cov."""
    n = int(n)
    if n < 2:
        raise ValueError("a covariance needs at least 2 rows, got n = %d" % n)
    s = np.asarray(sum, np.float64)
    mu = s / n
    sigma = (np.asarray(outer, np.float64) - n * np.outer(mu, mu)) / (n - 1)
    return mu, sigma


def _psd_sqrt(a):
    w, v = np.linalg.eigh(a)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 sum sqrt(max(eig(R sigma2 R), 0)), R = sigma1^(1/2); host, fp64."""
    mu1, mu2 = np.asarray(mu1, np.float64).reshape(-1), np.asarray(mu2, np.float64).reshape(-1)
    s1, s2 = np.asarray(sigma1, np.float64), np.asarray(sigma2, np.float64)
    C = mu1.shape[0]
    if mu2.shape != (C,) or s1.shape != (C, C) or s2.shape != (C, C):
        raise ValueError("shapes: mu %s / %s, sigma %s / %s" % (mu1.shape, mu2.shape, s1.shape, s2.shape))
    # A channel whose variance is exactly zero on either side (a dead ReLU channel: its row and column of that sigma
    # are zero) adds nothing to tr sqrt(sigma1 sigma2): R sigma2 R = R_K sigma2[K, K] R_K on the other channels K, and
    # the same with the sides exchanged.  Taking those channels out is exact, and it matters: left in, each is a null
    # direction whose computed eigenvalue is rounding noise of size eps |R sigma2 R|, and the square root turns noise
    # of 1e-18 into 1e-9 -- measured as the spread of d^2 over summation orders of the same moments.
    keep = (np.diagonal(s1) != 0.0) & (np.diagonal(s2) != 0.0)
    k1, k2 = s1[np.ix_(keep, keep)], s2[np.ix_(keep, keep)]
    ev = np.zeros(0)
    if keep.any():
        r = _psd_sqrt((k1 + k1.T) * 0.5)
        m = r @ ((k2 + k2.T) * 0.5) @ r
        ev = np.linalg.eigvalsh((m + m.T) * 0.5)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.clip(ev, 0.0, None)).sum())


def save_stats(path, mu, sigma, n):
    """`.npz` with mu [C], sigma [C, C] (float64) and n, written to exactly `path`."""
    with open(path, "wb") as f:
        np.savez(f, mu=np.asarray(mu, np.float64), sigma=np.asarray(sigma, np.float64), n=np.int64(n))


def load_stats(path, C):
    """-> (mu, sigma, n) of a stats file for a classifier whose pool_3 has C channels (n = 0 when the file, like the
    circulated ones, does not record it)."""
    with np.load(path) as f:
        mu, sigma = np.asarray(f["mu"], np.float64).reshape(-1), np.asarray(f["sigma"], np.float64)
        n = int(f["n"]) if "n" in f.files else 0
    if mu.shape[0] != C or sigma.shape != (mu.shape[0], mu.shape[0]):
        raise ValueError("%s holds statistics of %d features (sigma %s), the classifier's pool_3 has %d channels"
                         % (path, mu.shape[0], "x".join(str(d) for d in sigma.shape), C))
    return mu, sigma, n


def dataset_stats(classifier, images, rank=0, world=1):
    """(mu, sigma, n) of pool_3 over `images` (features.pool3_batches: numpy or a `utils.data.DeviceDataset`).  Rank r
    classifies its `features.share` of them on its device; one all-reduce; every rank returns the same values."""
    acc = MomentAccumulator(classifier.plan.pool3_channels, classifier.device)
    for rows in features.pool3_batches(classifier, images, *features.share(images.shape[0], rank, world)):
        acc.update(rows)
    n, s, o = acc.all_reduce().moments()
    mu, sigma = stats_from_moments(n, s, o)
    return mu, sigma, n


class FidMetric(features.HookMetric):
    """real = (mu, sigma) of the real data.  pool_3 of exactly the eval_samples samples the score covers goes into fp64
    moments on the device, one SUM all-reduce per evaluated model replaces a feature gather, rank 0 finalises on the host
    and broadcasts the scalar."""
    key, closing = "fid", 'min FID was %.4f, iter was %d'

    def begin(self):
        self.acc = MomentAccumulator(self.classifier.plan.pool3_channels, self.classifier.device)

    def take(self, rows):
        self.acc.update(rows)

    def finish(self, tag, bank):
        import torch
        from .. import parallel
        self.acc.all_reduce()
        d = torch.zeros(1, dtype=torch.float64, device=self.classifier.device)
        if self.rank == 0:
            d[0] = frechet_distance(*stats_from_moments(*self.acc.moments()), self.real[0], self.real[1])
            print('%sFID was %.4f' % (tag, float(d)))
        d = float(parallel.broadcast_(d))
        self.keep_minimum(d)
        return d


def main(argv=None):
    import argparse
    import torch
    from ..train import load_cifar
    from .inception import load_classifier
    ap = argparse.ArgumentParser(description="pool_3 statistics of the CIFAR-10 training set for train.py --fid_stats")
    ap.add_argument("--data_dir", required=True)
    ap.add_argument("--inception_model", required=True, help="the 2015 Inception graph (.pb, its .tgz or the directory)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=0, help="first N images only (0 = all)")
    a = ap.parse_args(argv)
    clf = load_classifier(a.inception_model, torch.device("cuda", torch.cuda.current_device()))
    if not hasattr(clf, "plan"):
        raise SystemExit("FID needs the 2015 Inception graph, not a TorchScript classifier")
    x = load_cifar(a.data_dir)
    mu, sigma, n = dataset_stats(clf, x[:a.samples] if a.samples else x)
    save_stats(a.out, mu, sigma, n)
    print("wrote pool_3 statistics of %d images (%d channels) to %s" % (n, mu.shape[0], a.out))


if __name__ == "__main__":
    main()
