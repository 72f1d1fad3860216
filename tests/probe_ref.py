"""numpy fp64 restatement of utils/probe.py and csrc/topk.hip, written for clarity (tests/test_probe_cpu.py,
tests/test_probe_gpu.py)."""
import numpy as np


def topk(q, y, k, self0=-1):
    """(index int32 [nq, k], score fp64 [nq, k]): the k largest q_i . y_j over j != self0 + i, by score descending, equal
    scores by the smaller column first; -1 and -inf where fewer were counted."""
    q, y = np.asarray(q, np.float64), np.asarray(y, np.float64)
    return topk_from_dots(q @ y.T if y.shape[0] else np.zeros((q.shape[0], 0)), k, self0)


def topk_from_dots(dots, k, self0=-1):
    """`topk` of a given [nq, ny] matrix of inner products (a test with duplicated columns makes their entries equal first:
    a BLAS need not return the same bits for the same pair at two places)."""
    nq, ny = dots.shape
    index = np.full((nq, k), -1, np.int32)
    score = np.full((nq, k), -np.inf)
    for i in range(nq):
        cols = np.array([j for j in range(ny) if self0 < 0 or j != self0 + i], np.int64)
        d = dots[i, cols]
        order = np.lexsort((cols, -d))[:k]          # last key first: -dot ascending, then the column ascending
        index[i, :len(order)] = cols[order]
        score[i, :len(order)] = d[order]
    return index, score


def bar(q, y):
    """[nq, ny]: 2 (C + 8) 2^-53 |q| |y|^T, the bound on the fp64 summation error of a dot product of exact products in
    any order (the one used for otgan_knn_f64), with the reference's own error inside the factor 2."""
    q, y = np.asarray(q, np.float64), np.asarray(y, np.float64)
    return 2.0 * (q.shape[1] + 8) * 2.0 ** -53 * (np.abs(q) @ np.abs(y).T)


def vote(neigh_labels):
    """The predicted class per row: the most frequent label among the slots >= 0, a tie to the tied class whose first
    member ranks highest, -1 for a row without a neighbour."""
    out = []
    for row in np.asarray(neigh_labels):
        best, best_votes = -1, 0
        for lab in row:                      # in rank order: a later class must have MORE votes to take over
            if lab < 0:
                continue
            votes = sum(1 for other in row if other == lab)
            if votes > best_votes:
                best, best_votes = int(lab), votes
        out.append(best)
    return np.array(out, np.int64)


def accuracy(bank, bank_labels, queries, query_labels, k, leave_one_out=False):
    """(correct at k, correct at 1, queries)"""
    bank_labels = np.asarray(bank_labels, np.int64)
    if leave_one_out:
        queries, query_labels, self0 = bank, bank_labels, 0
    else:
        self0 = -1
    query_labels = np.asarray(query_labels, np.int64)
    index = topk(queries, bank, k, self0)[0]
    neigh = np.where(index >= 0, bank_labels[np.maximum(index, 0)], -1) if len(bank_labels) else np.full(index.shape, -1)
    at_k = int((vote(neigh) == query_labels).sum())
    at_1 = int((vote(neigh[:, :1]) == query_labels).sum())
    return at_k, at_1, int(len(query_labels))
