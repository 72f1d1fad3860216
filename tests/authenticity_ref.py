"""numpy restatement of utils/authenticity.py and of otgan_nn_u8: int64 brute-force distances, the k smallest with the tie
rule, self exclusion by position, radii, the score and the sheet layout.  Nothing here is shared with the code under test."""
import numpy as np


def distances(q, y):
    """int64 [nq, ny]: sum_d (q_id - y_jd)^2 over the raw uint8 values, row by row (no Gram identity)."""
    q = np.asarray(q).reshape(len(q), -1).astype(np.int64)
    y = np.asarray(y).reshape(len(y), -1).astype(np.int64)
    out = np.empty((len(q), len(y)), np.int64)
    for i in range(len(q)):
        diff = y - q[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


def nearest_from_table(d, k, self0=-1):
    """(index int32 [nq, k], dist int64 [nq, k]) from the table d: per row the k smallest over the columns j != self0 + i,
    by (distance, column) ascending; (-1, -1) where fewer were counted."""
    nq, ny = d.shape
    index = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        order = [j for j in np.lexsort((np.arange(ny), d[i])) if not (self0 >= 0 and j == self0 + i)][:k]   # by (d, j)
        for t, j in enumerate(order):
            index[i, t], dist[i, t] = j, d[i, j]
    return index, dist


def nearest(q, y, k, self0=-1):
    return nearest_from_table(distances(q, y), k, self0)


def radii(bank):
    """int64 [n]: the squared distance of every bank row to its nearest OTHER bank row (by position)."""
    return nearest(bank, bank, 1, self0=0)[1][:, 0]


def score(index1, dist1, r):
    """(authentic, exact copies, lower median): authentic = dist1 > r[index1]."""
    index1, dist1, r = np.asarray(index1), np.asarray(dist1, np.int64), np.asarray(r, np.int64)
    authentic = sum(1 for i in range(len(dist1)) if dist1[i] > r[index1[i]])
    copies = sum(1 for v in dist1 if v == 0)
    return authentic, copies, int(sorted(int(v) for v in dist1)[(len(dist1) - 1) // 2])


def sheet(generated, bank, index, dist, rows=10):
    """The `rows` samples with the smallest nearest distance (ties: the smaller sample), one per line, each followed by its
    nearest bank images; cells of S x S pixels in a white grid of one-pixel lines."""
    generated, bank, index, dist = (np.asarray(v) for v in (generated, bank, index, dist))
    n, K = index.shape
    S = generated.shape[1]
    order = sorted(range(n), key=lambda i: (int(dist[i, 0]), i))[:rows]
    out = np.full((len(order) * (S + 1) + 1, (K + 1) * (S + 1) + 1, 3), 255, np.uint8)
    for r, i in enumerate(order):
        y0 = 1 + r * (S + 1)
        out[y0:y0 + S, 1:1 + S] = generated[i]
        for t in range(K):
            if index[i, t] >= 0:
                x0 = 1 + (t + 1) * (S + 1)
                out[y0:y0 + S, x0:x0 + S] = bank[index[i, t]]
    return out
