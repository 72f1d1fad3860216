"""fp64 restatement of the sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, "Progressive Growing
of GANs", section 5), as include/otgan_layers.h states it for csrc/swd.hip and utils/swd.py.  numpy only; written for
clarity, not speed: the tests use a few dozen small images."""
import numpy as np

PATCH = 7
G1 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
G = np.outer(G1, G1) / 256.0


def levels(S):
    if S not in (16, 32, 64):
        raise ValueError("S = %d: the pyramid is defined for 16, 32 and 64" % S)
    return {16: 1, 32: 2, 64: 3}[S]


def _mirror(i, n):
    """mirror without repeating the edge pixel: -1 -> 1, n -> n - 2 (scipy.ndimage mode='mirror')"""
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def convolve(x, k):
    """x [..., H, W, C] convolved with the symmetric 5 x 5 kernel k over H and W, mirror border."""
    H, W = x.shape[-3], x.shape[-2]
    out = np.zeros_like(x)
    for dy in range(5):
        ys = _mirror(np.arange(H) + dy - 2, H)
        for dx in range(5):
            xs = _mirror(np.arange(W) + dx - 2, W)
            out += k[dy, dx] * x[..., ys, :, :][..., :, xs, :]
    return out


def down(x):
    return convolve(x, G)[..., ::2, ::2, :]


def up(x):
    z = np.zeros(x.shape[:-3] + (2 * x.shape[-3], 2 * x.shape[-2], x.shape[-1]))
    z[..., ::2, ::2, :] = x
    return convolve(z, 4.0 * G)


def pyramid(img):
    """img uint8 [n, S, S, 3] -> list of L float64 arrays [n, S_l, S_l, 3]: Laplacian levels, the last one Gaussian."""
    img = np.asarray(img)
    L = levels(img.shape[1])
    pyr = [img.astype(np.float64)]
    for i in range(1, L):
        pyr.append(down(pyr[i - 1]))
        pyr[i - 1] = pyr[i - 1] - up(pyr[i])
    return pyr


def descriptors(level, pos):
    """level [n, s, s, 3], pos int [n, P, 2] (y, x) -> [n, P, 3, 7, 7] (channel, dy, dx)."""
    n, P = pos.shape[:2]
    out = np.empty((n, P, 3, PATCH, PATCH))
    for i in range(n):
        for p in range(P):
            y, x = pos[i, p]
            out[i, p] = level[i, y:y + PATCH, x:x + PATCH, :].transpose(2, 0, 1)
    return out


def channel_stats(desc):
    """(mean [3], std [3]) over all elements of each channel, population std."""
    return desc.mean(axis=(0, 1, 3, 4)), desc.std(axis=(0, 1, 3, 4))


def normalised(desc):
    mean, std = channel_stats(desc)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (desc - mean[None, None, :, None, None]) / std[None, None, :, None, None]
    return d.reshape(desc.shape[0] * desc.shape[1], 3 * PATCH * PATCH)


def projections(img, pos, dirs):
    """img uint8 [n, S, S, 3], pos [L, n, P, 2], dirs [nd, 147] -> list of L arrays [nd, n P]."""
    pyr = pyramid(img)
    return [np.asarray(dirs, np.float64) @ normalised(descriptors(pyr[l], np.asarray(pos)[l])).T for l in range(len(pyr))]


def row_distance(pa, pb):
    """mean |sort(pa) - sort(pb)| per row"""
    return np.abs(np.sort(pa, axis=1) - np.sort(pb, axis=1)).mean(axis=1)


def distance(A, B, pos_a, pos_b, dirs):
    """-> [L] the sliced Wasserstein distance x 1e3 of every level (the mean over the directions)."""
    pa, pb = projections(A, pos_a, dirs), projections(B, pos_b, dirs)
    return np.array([1e3 * row_distance(a, b).mean() for a, b in zip(pa, pb)])
