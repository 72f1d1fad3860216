"""Is the generator copying the training set?  Exact nearest neighbours in pixel space and the authenticity score of Alaa et
al. 2022 ("How Faithful is your Synthetic Data?"), the one question Inception score, FID, KID, precision and SWD do not ask.

With d(a, b) = sum over the pixels of (a - b)^2 on the raw uint8 values (tests/authenticity_ref.py restates all of it in numpy):

    nearest(q, y, k)  = per query the k training rows at the smallest d, by distance ascending, equal distances by the smaller
                        row first (csrc/pixnn.hip, `otgan_nn_u8`: int8 MFMAs, exact int32 products, the distance matrix never
                        written)
    r_j               = d(y_j, its nearest OTHER training row), leave-one-out by position (`radii`)
    authentic(x)      = d(x, y_n) > r_n for n = the nearest training row of x: a sample that sits closer to a training image
                        than that image's own nearest neighbour is a copy of it, not a sample of the distribution
    authenticity      = the fraction of authentic samples;   exact copies = samples with d = 0
    median distance   = the LOWER median of the nearest distances, element (n - 1) // 2 of the sorted values: an integer

Every number is an exact integer and every ranking a total order, so counts, median and sheet are functions of the two image
sets alone: no tolerance, and two ranks return exactly what one process returns.  Held-out images score near 1/2 on data
without duplicates (a fresh draw is nearer to y_n than y_n's own neighbour about half the time); a generator far BELOW its
held-out baseline memorises.  Distances are shown as sqrt(d / D), the rms difference in 8-bit levels.  CUDA tensors only:
there is no CPU fallback.
"""
import numpy as np

from .. import _lib

MAX_K = 8


def check_neighbours(k):
    """1 <= k <= 8; ValueError otherwise."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("%d neighbours: between 1 and %d" % (k, MAX_K))
    return k


def nearest(q, y, k, self0=-1):
    """(index int32 CUDA [nq, k], dist int64 CUDA [nq, k]) of ops.nn_u8: q, y uint8 CUDA [n, D] or [n, S, S, 3].  Row
    self0 + i of y is skipped for row i of q (self0 = -1: none); (-1, -1) where fewer than k rows were counted."""
    import torch
    from .. import ops
    for t in (q, y):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.OtganError("authenticity.nearest takes CUDA (MI355X) uint8 images; there is no CPU fallback")
    if q.dtype != torch.uint8 or y.dtype != torch.uint8:
        raise ValueError("authenticity.nearest takes uint8 images, found %s and %s" % (q.dtype, y.dtype))
    if tuple(q.shape[1:]) != tuple(y.shape[1:]):
        raise ValueError("the two sets differ: rows of %s against %s" % (tuple(q.shape[1:]), tuple(y.shape[1:])))
    k, self0 = check_neighbours(k), int(self0)
    if self0 < -1:
        raise ValueError("authenticity.nearest: self0 %d >= -1" % self0)
    return ops.nn_u8(q, y, k, self0)


def radii(bank, rank=0, world=1):
    """int64 CUDA [n], the same on every rank: r_j = the squared distance of bank row j to its nearest OTHER bank row (by
    position: a duplicate gives 0); -1 for a bank of one row.  A rank computes its contiguous share of the rows against the
    whole bank and the vector is gathered."""
    from . import features
    lo, hi = features.share(bank.shape[0], rank, world)
    mine = nearest(bank[lo:hi], bank, 1, self0=lo)[1][:, 0].contiguous()
    return features.gather_rows(mine, rank, world)[0] if world > 1 else mine


def flags(index1, dist1, radii):
    """bool [n]: authentic = dist1 > radii[index1] (index1, dist1: the first neighbour's column of `nearest`)."""
    return dist1 > radii[index1.long()]


def lower_median(dist1):
    """Element (n - 1) // 2 of the sorted values as a Python int."""
    import torch
    n = dist1.shape[0]
    if n == 0:
        raise ValueError("the median of no distance")
    return int(torch.sort(dist1)[0][(n - 1) // 2])


def score(index1, dist1, radii):
    """(authentic samples, exact copies, lower median of dist1) as Python ints; index1 / dist1: int [n], the nearest bank row
    of each query and its squared distance; radii: int64 [bank rows]."""
    return int(flags(index1, dist1, radii).sum()), int((dist1 == 0).sum()), lower_median(dist1)


def rms(d, D):
    """sqrt(d / D): a squared distance over D values as the rms difference in 8-bit levels."""
    return float(np.sqrt(float(d) / float(D)))


def sheet(generated, bank, index, dist, rows=10):
    """uint8 [R (S + 1) + 1, (K + 1) (S + 1) + 1, 3], R = min(rows, n): the R samples with the smallest nearest distance
    (equal distances by the smaller sample first), one per line, each followed by its K = index.shape[1] nearest training
    images in rank order; white one-pixel separators as train.save_tile_png; an empty slot (index -1) stays white.  generated,
    bank: uint8 [n, S, S, 3] (torch on any device, or numpy); index, dist: [n, K]."""
    to_np = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    index, dist = to_np(index), to_np(dist)
    n, K = index.shape
    S = generated.shape[1]
    order = np.argsort(dist[:, 0], kind="stable")[:max(min(int(rows), n), 0)]
    out = np.full((len(order) * (S + 1) + 1, (K + 1) * (S + 1) + 1, 3), 255, np.uint8)
    for r, i in enumerate(order):
        cells = [to_np(generated[int(i)])] + [to_np(bank[int(j)]) if j >= 0 else None for j in index[i]]
        for c, im in enumerate(cells):
            if im is not None:
                out[1 + r * (S + 1):1 + r * (S + 1) + S, 1 + c * (S + 1):1 + c * (S + 1) + S] = im
    return out


def save_png(array, path):
    """Through PIL when present, skipped silently otherwise (as train.save_tile_png)."""
    try:
        from PIL import Image
    except ImportError:
        return
    Image.fromarray(array).save(path)


class AuthenticityMetric:
    """What train.authenticity_hook keeps and says.  `measure(images, k)` takes a whole query set (uint8 CUDA, the same on
    every rank), searches this rank's share of the queries (features.share) against the bank, sums the two counts in one
    all-reduce and gathers neighbours and distances: every rank gets {"authentic", "copies", "n", "median", "index", "dist"}.
    `evaluate` prints the line on rank 0 and keeps the running minimum in state["authenticity_min" / "authenticity_iter"];
    `held`: the held-out baseline as a `measure` result, or None."""
    key = "authenticity"

    def __init__(self, bank, radii, state, rank=0, world=1, held=None):
        self.bank, self.radii, self.state, self.rank, self.world, self.held = bank, radii, state, rank, world, held
        self.D = int(np.prod(bank.shape[1:]))
        state.setdefault("authenticity_min", float("inf"))
        state.setdefault("authenticity_iter", 0)

    def measure(self, images, k=1):
        import torch
        from .. import parallel
        from . import features
        n = images.shape[0]
        lo, hi = features.share(n, self.rank, self.world)
        index, dist = nearest(images[lo:hi], self.bank, k)
        i1, d1 = index[:, 0], dist[:, 0]
        c = torch.stack([flags(i1, d1, self.radii).sum(), (d1 == 0).sum()]).to(torch.int64)
        c = parallel.allreduce_sum_([c])[0]
        if self.world > 1:
            index = features.gather_rows(index, self.rank, self.world)[0]
            dist = features.gather_rows(dist, self.rank, self.world)[0]
        authentic, copies = (int(v) for v in c.tolist())
        return {"authentic": authentic, "copies": copies, "n": n, "median": lower_median(dist[:, 0]), "index": index, "dist": dist}

    def line(self, m, tag=""):
        held = self.held
        return ('%sauthenticity was %.4f%s, median nearest distance was %.2f%s, exact copies %d, %d generated against %d training images'
                % (tag, m["authentic"] / m["n"], ' (held-out %.4f)' % (held["authentic"] / held["n"]) if held else '',
                   rms(m["median"], self.D), ' (held-out %.2f)' % rms(held["median"], self.D) if held else '',
                   m["copies"], m["n"], self.bank.shape[0]))

    def evaluate(self, images, tag="", k=1):
        m = self.measure(images, k)
        if self.rank == 0:
            print(self.line(m, tag))
        a = m["authentic"] / m["n"]
        if a < self.state["authenticity_min"]:
            self.state["authenticity_min"], self.state["authenticity_iter"] = a, self.state.get("epoch", 0)
        return m

    def close(self):
        if self.rank == 0:
            print('min authenticity was %.4f, iter was %d' % (self.state["authenticity_min"], self.state["authenticity_iter"]))
