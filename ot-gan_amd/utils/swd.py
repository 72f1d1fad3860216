"""The sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, "Progressive Growing of GANs", section 5):
the one sample-quality metric that needs nothing but the two image sets -- no Inception graph.  One number per pyramid level,
so large-scale structure (the 16 x 16 level) is told from texture (the finest level).

Definition (include/otgan_layers.h states the device stages; tests/swd_ref.py restates all of it in fp64).  Both sets are uint8
[n, S, S, 3], S in {16, 32, 64}; generated samples are quantised as clip(rint(127.5 (x + 1)), 0, 255), half to even (`quantise`).
Each image becomes a Laplacian pyramid of L = log2(S / 16) + 1 levels (5 x 5 binomial filter, mirror border, the 16 x 16 level
stays Gaussian); per level and image P patches of 7 x 7 x 3 at given positions are flattened in [channel, dy, dx] order and
each channel is normalised by the mean and population std over all of that set's descriptor elements of the level; both sets'
n P descriptors are projected on R K unit directions, each projection is sorted, and the distance of the level is the mean
over directions of mean |sort A - sort B|, x 1e3.  The paper's sizes: n = 16384, P = 128, K = 128, R = 4.

Positions and directions are inputs, drawn on the host from a private seeded generator (`positions`, `directions`), never in a
kernel.  The descriptor matrix (1.2 GB per level and set at the paper's sizes) is never written: ops.swd_channel_stats and
ops.swd_project gather the patches from the pyramid in LDS.  The per-direction sorts are torch.sort (rocPRIM), the one framework
call on this path; directions go through in chunks whose projections, sorted values and int64 indices stay under CHUNK_BYTES.
Every stage is deterministic and a direction's distance does not depend on which directions share a call, so the [L, R K] table
is the same however the directions are split over ranks.  CUDA tensors only: there is no CPU fallback.
"""
import numpy as np

from .. import _lib

PATCH = 7
DESC = 3 * PATCH * PATCH
CHUNK_BYTES = 3 * 10 ** 9        # projections (4 B) + sorted values (4 B) + sort indices (8 B) of one chunk of directions
SAMPLE_BATCH = 500               # generated images per generator pass of the hook; part of the definition of sample i's latent
SEED_OFFSET = 0x5357             # the hook's private device seeds: (--seed + SEED_OFFSET) * 65536 + batch number


def levels(S):
    """log2(S / 16) + 1 for S in {16, 32, 64}; a ValueError otherwise."""
    if S not in (16, 32, 64):
        raise ValueError("the sliced Wasserstein pyramid is defined for images of 16, 32 and 64 pixels a side, not %s" % (S,))
    return {16: 1, 32: 2, 64: 3}[S]


def quantise(x):
    """Images in [-1, 1] -> uint8 by clip(rint(127.5 (x + 1)), 0, 255), rounding half to even, in the precision of x.  A torch
    tensor (any device) or a numpy array; the result is of the same kind."""
    try:
        import torch
    except ImportError:
        torch = None
    if torch is not None and torch.is_tensor(x):
        return torch.round(127.5 * (x + 1.0)).clamp_(0.0, 255.0).to(torch.uint8)
    x = np.asarray(x)
    return np.clip(np.rint(127.5 * (x + 1.0)), 0.0, 255.0).astype(np.uint8)


def positions(n, S, P, generator):
    """Top-left corners (y, x) of P patches per image and level, uniform on 0 ... S_l - 7: int32 [L, n, P, 2] on the host, drawn
    from `generator` (a CPU torch.Generator) level by level."""
    import torch
    L = levels(S)
    if n < 0 or P < 1:
        raise ValueError("positions of %d images x %d patches" % (n, P))
    return torch.stack([torch.randint(0, (S >> l) - PATCH + 1, (n, P, 2), generator=generator, dtype=torch.int64).to(torch.int32)
                        for l in range(L)])


def directions(R, K, generator):
    """R K directions, each a normal draw of 147 values scaled to unit length (in fp64, stored as fp32): [R K, 147] on the host."""
    import torch
    if R < 1 or K < 1:
        raise ValueError("%d repeats x %d directions" % (R, K))
    d = torch.randn(R * K, DESC, generator=generator, dtype=torch.float64)
    return (d / d.norm(dim=1, keepdim=True)).to(torch.float32)


def _cuda_images(images, who):
    import torch
    if not (torch.is_tensor(images) and images.is_cuda):
        raise _lib.OtganError("%s takes CUDA (MI355X) uint8 images; there is no CPU fallback" % who)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != images.shape[2] or images.shape[3] != 3:
        raise ValueError("%s takes uint8 [n, S, S, 3] images, found %s %s" % (who, images.dtype, tuple(images.shape)))
    levels(images.shape[1])
    if images.shape[0] == 0:
        raise ValueError("%s: no images" % who)
    return images.contiguous()


def chunk_directions(n, P, budget=CHUNK_BYTES):
    """directions per chunk: 16 bytes per projection (fp32 projections, fp32 sorted values, int64 indices) under `budget`"""
    return max(1, int(budget // (16 * n * P)))


def sorted_projections(images, pos, dirs, level, stats=None, chunk=None):
    """Yields (j0, sorted fp32 [c, n P]) for consecutive chunks of the rows of `dirs`: the projections of level `level` of
    `images` at `pos`, each row sorted ascending.  `stats` = (mean, inv_std) of ops.swd_channel_stats (computed when None)."""
    import torch
    from .. import ops
    mean, inv_std = ops.swd_channel_stats(images, pos) if stats is None else stats
    n, P = images.shape[0], pos.shape[2]
    chunk = chunk or chunk_directions(n, P)
    for j0 in range(0, dirs.shape[0], chunk):
        proj = ops.swd_project(images, pos, level, mean, inv_std, dirs[j0:j0 + chunk])
        yield j0, torch.sort(proj, dim=1)[0]


class SwdReal:
    """The real side, computed once per run: the sorted projections of every level of `images` (uint8 CUDA [n, S, S, 3]) at
    positions `pos` on the directions `dirs[lo:hi]`, (lo, hi) = dir_range (all of them when None), kept on the device as L
    tensors fp32 [hi - lo, n P].  Size: L (hi - lo) n P 4 bytes -- with all R K = 512 directions 8.6 GB at the paper's sizes and
    32 x 32 (L = 2), 12.9 GB at 64 x 64; a rank of `world` keeps its share of the directions, 1 / world of that, and
    --swd_samples lowers it in proportion.  `pos_gen`: the positions that `distances` uses for the other side by default."""

    def __init__(self, images, pos, dirs, pos_gen=None, dir_range=None):
        import torch
        images = _cuda_images(images, "SwdReal")
        dev = images.device
        self.n, self.S, self.L = images.shape[0], images.shape[1], levels(images.shape[1])
        self.P = pos.shape[2]
        self.dirs = dirs.to(dev, torch.float32).contiguous()
        self.lo, self.hi = (0, self.dirs.shape[0]) if dir_range is None else (int(dir_range[0]), int(dir_range[1]))
        if not 0 <= self.lo <= self.hi <= self.dirs.shape[0]:
            raise ValueError("directions %d ... %d of %d" % (self.lo, self.hi, self.dirs.shape[0]))
        self.pos_gen = None if pos_gen is None else pos_gen.to(dev)
        pos = pos.to(dev)
        stats = None
        self.sorted = []
        for l in range(self.L):
            kept = torch.empty(self.hi - self.lo, self.n * self.P, dtype=torch.float32, device=dev)
            if self.hi > self.lo:
                if stats is None:
                    from .. import ops
                    stats = ops.swd_channel_stats(images, pos)
                for j0, rows in sorted_projections(images, pos, self.dirs[self.lo:self.hi], l, stats):
                    kept[j0:j0 + rows.shape[0]].copy_(rows)
            self.sorted.append(kept)

    @property
    def nbytes(self):
        return sum(t.numel() * 4 for t in self.sorted)


def distances(images, real, dir_range=None, pos=None):
    """fp64 CUDA [L, hi - lo]: per level and direction, mean |sort A - sort B| x 1e3 between `images` (uint8 CUDA [n, S, S, 3], the
    n and S of `real`) at positions `pos` (real.pos_gen when None) and the real side, for the directions (lo, hi) = dir_range
    inside the range `real` keeps (all of that range when None).  A column depends on its direction alone, so any split of the
    directions gives the columns of the whole table, bit for bit.  [L, R K] when `real` keeps every direction."""
    import torch
    from .. import ops
    images = _cuda_images(images, "swd.distances")
    lo, hi = (real.lo, real.hi) if dir_range is None else (int(dir_range[0]), int(dir_range[1]))
    if not real.lo <= lo <= hi <= real.hi:
        raise ValueError("directions %d ... %d: the real side keeps %d ... %d" % (lo, hi, real.lo, real.hi))
    if tuple(images.shape) != (real.n, real.S, real.S, 3):
        raise ValueError("the two sets differ: %s against %d real images of side %d" % (tuple(images.shape), real.n, real.S))
    pos = real.pos_gen if pos is None else pos
    if pos is None:
        raise ValueError("swd.distances needs the positions of the generated side (pos, or SwdReal(pos_gen=...))")
    pos = pos.to(images.device)
    if pos.shape[2] != real.P:
        raise ValueError("%d patches per image against the real side's %d" % (pos.shape[2], real.P))
    out = torch.empty(real.L, hi - lo, dtype=torch.float64, device=images.device)
    if hi == lo:
        return out
    stats = ops.swd_channel_stats(images, pos)
    for l in range(real.L):
        for j0, rows in sorted_projections(images, pos, real.dirs[lo:hi], l, stats):
            there = real.sorted[l][lo - real.lo + j0:lo - real.lo + j0 + rows.shape[0]]
            out[l, j0:j0 + rows.shape[0]] = ops.swd_row_l1(rows, there) * 1e3
    return out


def summary(table):
    """([L] per-level distances, their average) as Python floats from the [L, R K] table: the mean over the directions in fp64,
    one fixed order."""
    per = table.double().mean(dim=1).tolist()
    return per, sum(per) / len(per)


class SwdMetric:
    """What train.swd_hook keeps and says: `evaluate(images)` takes the whole generated set (uint8 CUDA, the same on every
    rank), computes this rank's contiguous share of the directions, gathers the [L, R K] table and returns (per level, average);
    rank 0 prints the line.  `close` prints the running minimum of the average, kept in state["swd_min" / "swd_iter"]."""
    key = "swd"

    def __init__(self, real, args, state, rank=0, world=1):
        self.real, self.args, self.state, self.rank, self.world = real, args, state, rank, world
        state.setdefault("swd_min", float("inf"))
        state.setdefault("swd_iter", 0)

    def evaluate(self, images, tag=""):
        import torch
        from . import features
        table = distances(images, self.real)                      # [L, this rank's directions]
        if self.world > 1:
            table = features.gather_rows(table.t().contiguous(), self.rank, self.world)[0].t().contiguous()
        per, avg = summary(table)
        if self.rank == 0:
            S = self.real.S
            print('%ssliced Wasserstein distance x 1e3 was %s, average %.4f'
                  % (tag, ', '.join('%dx%d: %.4f' % (S >> l, S >> l, v) for l, v in enumerate(per)), avg))
        if avg < self.state["swd_min"]:
            self.state["swd_min"], self.state["swd_iter"] = avg, self.state["epoch"]
        return per, avg

    def close(self):
        if self.rank == 0:
            print('min average SWD was %.4f, iter was %d' % (self.state["swd_min"], self.state["swd_iter"]))


def sample_images(model, n, seed, ema=False, rank=0, world=1):
    """n generated images as uint8 CUDA [n, S, S, 3], the same on every rank and for every world size, without moving the
    training run: image i belongs to batch i // SAMPLE_BATCH, whose latents come from the device generator seeded with
    (seed + SEED_OFFSET) * 65536 + batch number; a rank draws a contiguous share of the batches and the uint8 images are
    all-gathered.  The device generator's state is saved before and put back after: the run's own stream continues where it was."""
    import torch
    from . import features
    dev = model.device
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    nb = -(-n // SAMPLE_BATCH)
    lo, hi = features.share(nb, rank, world)
    saved = gen.get_state()
    out = []
    try:
        for b in range(lo, hi):
            gen.manual_seed((int(seed) + SEED_OFFSET) * 65536 + b)
            out.append(quantise(model.sample(min(SAMPLE_BATCH, n - b * SAMPLE_BATCH), ema=ema).float()))
    finally:
        gen.set_state(saved)
    S = model.args.image_size
    mine = torch.cat(out) if out else torch.empty(0, S, S, 3, dtype=torch.uint8, device=dev)
    return features.gather_rows(mine, rank, world)[0] if world > 1 else mine
