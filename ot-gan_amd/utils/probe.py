"""k-nearest-neighbour classification of labelled rows in a feature map's own cosine geometry: the training-free score
of "is the critic learning a useful embedding?".

The critic's features are unit-norm, so the largest inner products are the nearest rows.  With K neighbours:

    neighbours(x) = the K bank rows with the largest q . y, ranked by score descending, equal scores by the smaller
                    bank row first (csrc/topk.hip, `otgan_topk_dot_f64`: exact products on the fp64 MFMA, the
                    Gram matrix never written, (score, row) lists folded in registers)
    predict(x)    = the most frequent label among them; a tie goes to the tied class whose first member ranks
                    highest; a row with no neighbour predicts -1, which is never correct
    accuracy at K = mean over the queries of [predict == label];   accuracy at 1 = the same with the first neighbour

The ranking is a total order and a score is the same bits in whichever call, tile or operand role it is computed, so
the neighbours -- and the counts -- are a function of the feature rows alone.  Ranks: every rank holds its share of
the bank and of the queries; its own queries run against all ranks' bank rows, gathered on the device in rank order,
and the integer counts are summed in one all-reduce: two ranks return exactly what one process returns.
"""
from .. import _lib
from .features import gather_rows, kernel_rows    # (gather_rows: also this module's name)

MAX_K = 8


def check_neighbours(k, bank_rows=None):
    """1 <= k <= 8, and (when given) a bank of MORE than k rows.  ValueError otherwise."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("%d neighbours: between 1 and %d" % (k, MAX_K))
    if bank_rows is not None and int(bank_rows) <= k:
        raise ValueError("a k-NN vote over %d neighbours needs a bank of more than %d rows: it has %d" % (k, k, int(bank_rows)))
    return k


def topk(q, y, k, self0=-1):
    """(index int32 CUDA [nq, k], score fp64 CUDA [nq, k]): per row of q the rows of y with the k largest inner products,
    by score descending, equal scores by the smaller row first; -1 and -inf where fewer were counted.  Column self0 + i
    is skipped for row i (self0 = -1: none).  q, y: fp32 CUDA [rows, C] (a column slice of a wider buffer passes its row
    stride on)."""
    import torch
    q, y = kernel_rows(q, "q", "topk"), kernel_rows(y, "y", "topk")
    if q.shape[1] != y.shape[1] or q.device != y.device:
        raise ValueError("q %s and y %s must have the same channels and device" % (tuple(q.shape), tuple(y.shape)))
    k, self0 = check_neighbours(k), int(self0)
    if self0 < -1:
        raise ValueError("topk: self0 %d >= -1" % self0)
    nq, ny = q.shape[0], y.shape[0]
    index = torch.empty(nq, k, dtype=torch.int32, device=q.device)
    score = torch.empty(nq, k, dtype=torch.float64, device=q.device)
    if nq == 0:
        return index, score
    L = _lib.lib()
    nbytes = L.otgan_topk_dot_workspace_bytes(nq, ny, k)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(L.otgan_topk_dot_f64(nq, ny, q.shape[1], q.data_ptr(), q.stride(0), y.data_ptr() if ny else None,
                                        y.stride(0) if ny else q.shape[1], k, self0, index.data_ptr(), score.data_ptr(),
                                        ws.data_ptr(), nbytes, _lib.stream_ptr()), "topk")
    return index, score


def vote(neigh_labels):
    """int64 [nq]: the predicted class per row of `neigh_labels`, int64 [nq, k] -- the labels (>= 0) of the ranked
    neighbours, -1 for an empty slot.  The most frequent label among the non-empty slots wins; a tie goes to the tied class
    whose first member ranks highest; a row with no neighbour predicts -1.  Torch ops on the tensor's device: nq * k
    integers."""
    import torch
    lab = neigh_labels
    if not (torch.is_tensor(lab) and lab.dim() == 2 and lab.dtype == torch.int64):
        raise ValueError("vote takes int64 [rows, k] labels")
    if lab.shape[1] == 0:
        return torch.full((lab.shape[0],), -1, dtype=torch.int64, device=lab.device)
    ok = lab >= 0
    # votes[i][t] = members of slot t's class in row i; the first slot (by rank) with the most votes wins: argmax returns
    # the first maximum only by convention of the backend, so the rank is folded into the key instead
    votes = ((lab[:, :, None] == lab[:, None, :]) & ok[:, None, :]).sum(2) * ok
    k = lab.shape[1]
    key = votes * k + (k - 1 - torch.arange(k, device=lab.device))
    best = key.argmax(1)                                   # keys of a row with votes are distinct in every non-empty slot
    pred = lab.gather(1, best[:, None])[:, 0]
    return torch.where(ok.any(1), pred, torch.full_like(pred, -1))


def counts(bank, bank_labels, queries, query_labels, k, rank=0, world=1, leave_one_out=False):
    """int64 CUDA [3], the same on every rank: (queries the K-vote gets right, queries the first neighbour gets right,
    queries) over all ranks.  See `accuracy`."""
    import torch
    from .. import parallel
    k = check_neighbours(k)
    bank_labels = torch.as_tensor(bank_labels, dtype=torch.int64).to(bank.device)
    if bank_labels.shape != (bank.shape[0],):
        raise ValueError("%d bank rows, labels %s" % (bank.shape[0], tuple(bank_labels.shape)))
    all_bank, first = gather_rows(bank, rank, world)
    all_labels = gather_rows(bank_labels, rank, world)[0]
    if leave_one_out:
        q, ql, self0 = bank, bank_labels, first
    else:
        q, ql, self0 = queries, torch.as_tensor(query_labels, dtype=torch.int64).to(bank.device), -1
        if ql.shape != (q.shape[0],):
            raise ValueError("%d query rows, labels %s" % (q.shape[0], tuple(ql.shape)))
    index = topk(q, all_bank, k, self0)[0].to(torch.int64)
    neigh = torch.where(index >= 0, all_labels[index.clamp(min=0)], torch.full_like(index, -1)) if all_labels.numel() \
        else torch.full_like(index, -1)
    c = torch.stack([(vote(neigh) == ql).sum(), (vote(neigh[:, :1]) == ql).sum(),
                     torch.tensor(q.shape[0], device=bank.device)]).to(torch.int64)
    return parallel.allreduce_sum_([c])[0]


def accuracy(bank, bank_labels, queries, query_labels, k, rank=0, world=1, leave_one_out=False):
    """(correct at K, correct at 1, queries) as Python ints, summed over the ranks in one all-reduce: the two accuracies are
    the quotients.  bank, queries: this rank's share of the fp32 CUDA feature rows; the labels: int64 per row, >= 0.  The
    bank is gathered on the device (features.gather_rows), the queries stay sharded.  Given the same feature rows, two
    ranks return exactly what one process returns.  leave_one_out=True: the bank against itself, every row skipping its
    own column (`queries` and `query_labels` are not read) -- for data with labels but no held-out split."""
    return tuple(int(v) for v in counts(bank, bank_labels, queries, query_labels, k, rank, world, leave_one_out).tolist())
