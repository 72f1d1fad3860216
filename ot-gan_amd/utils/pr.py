"""Precision, recall, density and coverage beside the Inception score, FID and KID, from fused k-NN passes on the device.

The three scalars above mix sample quality with diversity; these four separate them.  With G the generated and R the real
`pool_3` rows, K = --pr_neighbours and rho_K(x; S) the K-th smallest squared distance from x to the OTHER rows of its own
set S (excluded by position: a second row with the same values is a neighbour at distance 0):

    precision = mean over g of [ some r has d2(g, r) <= rho_K(r; R) ]        (Kynkaanniemi et al. 2019, "Improved precision
    recall    = mean over r of [ some g has d2(r, g) <= rho_K(g; G) ]         and recall metric ...", K = 3 as evaluated on
                                                                              the 2015 graph's pool_3 by guided-diffusion)
    density   = sum over g of #{ r : d2(g, r) <= rho_K(r; R) } / (K Ng)      (Naeem et al. 2020, "Reliable fidelity and
    coverage  = mean over r of [ min over g of d2(r, g) <= rho_K(r; R) ]      diversity metrics ...")

All comparisons are on SQUARED distances d2(a, b) = max(0, (a.a + b.b) - 2 a.b); no square root is taken.  The dot
products come from csrc/knn.hip (`otgan_knn_f64`: exact products on the fp64 MFMA, no distance matrix written, the k
smallest and the threshold counts per row folded in registers); both feature banks stay on the device.  A model costs
three passes (G x G for its radii, G x R for precision and density, R x G for recall and coverage); the radii of the real
rows (R x R) are computed once per run.

Ranks: every rank holds its share of both banks; its own rows are the queries and the columns are all ranks' rows,
gathered on the device in rank order, `self0` = the rank's first global row.  The integer counts are summed with one
all-reduce and divided afterwards, so the four values are exactly quotients of integers.  d2 of a pair is the same bits
in whichever call, tile or operand role it is computed, a K-th smallest value and a count do not depend on the order of
the columns -- so, UNLIKE KID, two ranks return exactly the values one process returns.
"""
from .. import _lib
from .features import HookMetric, gather_rows, kernel_rows    # (gather_rows: also this module's name)

MAX_K = 8


def check_neighbours(k, gen_rows, real_rows):
    """The rule of --pr_neighbours: 1 <= k <= 8, and the smaller bank (over all ranks) has MORE than k rows -- a row needs
    k neighbours besides itself.  ValueError otherwise."""
    k, gen_rows, real_rows = int(k), int(gen_rows), int(real_rows)
    if not 1 <= k <= MAX_K:
        raise ValueError("--pr_neighbours %d: between 1 and %d (the papers use 3)" % (k, MAX_K))
    if min(gen_rows, real_rows) <= k:
        raise ValueError("precision and recall with --pr_neighbours %d need more than %d rows per side: %d generated rows, "
                         "%d real rows" % (k, k, gen_rows, real_rows))
    return k


def knn(q, y, k, self0=-1, thresh=None):
    """(nearest fp64 CUDA [nq, k], inside int32 CUDA [nq] or None): per row of q the k smallest d2 to the rows of y,
    ascending (+inf where fewer were counted), and -- with thresh, fp64 [ny] -- the number of columns j with
    d2 <= thresh[j].  Column self0 + i is skipped for row i (self0 = -1: none).  q, y: fp32 CUDA [rows, C] (a column
    slice of a wider buffer passes its row stride on)."""
    import torch
    q, y = kernel_rows(q, "q", "knn"), kernel_rows(y, "y", "knn")
    if q.shape[1] != y.shape[1] or q.device != y.device:
        raise ValueError("q %s and y %s must have the same channels and device" % (tuple(q.shape), tuple(y.shape)))
    k, self0 = int(k), int(self0)
    if not 0 <= k <= MAX_K or self0 < -1:
        raise ValueError("knn: k %d in 0 ... %d, self0 %d >= -1" % (k, MAX_K, self0))
    nq, ny = q.shape[0], y.shape[0]
    if thresh is not None:
        if not (torch.is_tensor(thresh) and thresh.dtype == torch.float64 and thresh.shape == (ny,) and thresh.device == y.device):
            raise ValueError("thresh must be float64 [%d] on the device of y" % ny)
        thresh = thresh.contiguous()
    nearest = torch.empty(nq, k, dtype=torch.float64, device=q.device)
    inside = torch.empty(nq, dtype=torch.int32, device=q.device) if thresh is not None else None
    if nq == 0:
        return nearest, inside
    L = _lib.lib()
    nbytes = L.otgan_knn_workspace_bytes(nq, ny, k)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(L.otgan_knn_f64(nq, ny, q.shape[1], q.data_ptr(), q.stride(0), y.data_ptr() if ny else None, y.stride(0) if ny else q.shape[1],
                                   k, self0, thresh.data_ptr() if thresh is not None else None,
                                   nearest.data_ptr() if k else None, inside.data_ptr() if inside is not None else None,
                                   ws.data_ptr(), nbytes, _lib.stream_ptr()), "knn")
    return nearest, inside


def radii(bank_rows, k, rank=0, world=1, gathered=None):
    """fp64 CUDA [rows of all ranks]: rho_k of every row of the bank -- this rank's rows against all ranks' rows
    (`gathered` = gather_rows(bank_rows, rank, world) if the caller has it), its own column excluded, then gathered."""
    k = int(k)
    if k < 1:
        raise ValueError("radii: k %d >= 1" % k)
    allx, first = gathered if gathered is not None else gather_rows(bank_rows, rank, world)
    mine = knn(bank_rows, allx, k, self0=first)[0][:, k - 1].contiguous()
    return gather_rows(mine, rank, world)[0]


def counts(gen_bank, real_bank, k, real_radii=None, rank=0, world=1):
    """int64 CUDA [6], the same on every rank: (generated rows inside some real ball, real rows inside some generated
    ball, the real balls around the generated rows summed, real rows whose nearest generated row is inside their own
    ball, generated rows, real rows) over all ranks."""
    import torch
    from .. import parallel
    k = int(k)
    g, r = gen_bank.rows, real_bank.rows
    g_all, g0 = gather_rows(g, rank, world)
    r_all, r0 = gather_rows(r, rank, world)
    if real_radii is None:
        real_radii = radii(r, k, rank, world, (r_all, r0))
    gen_radii = radii(g, k, rank, world, (g_all, g0))
    in_real = knn(g, r_all, 0, thresh=real_radii)[1]
    nearest, in_gen = knn(r, g_all, 1, thresh=gen_radii)
    covered = nearest[:, 0] <= real_radii[r0:r0 + r.shape[0]]
    c = torch.stack([(in_real > 0).sum(), (in_gen > 0).sum(), in_real.sum(dtype=torch.int64), covered.sum(),
                     torch.tensor(g.shape[0], device=g.device), torch.tensor(r.shape[0], device=g.device)]).to(torch.int64)
    return parallel.allreduce_sum_([c])[0]


def values_from_counts(c, k):
    """(precision, recall, density, coverage) as Python floats: quotients of the integer counts of `counts`."""
    p, r, d, cov, ng, nr = (int(v) for v in c)
    return p / ng, r / nr, d / (int(k) * ng), cov / nr


def precision_recall(gen_bank, real_bank, k, real_radii=None, rank=0, world=1):
    """(precision, recall, density, coverage) of the generated bank against the real bank, the same on every rank and for
    every world size.  `real_radii`: radii(real_bank.rows, k, rank, world), computed once per run."""
    check_neighbours(k, gen_bank.total, real_bank.total)
    return values_from_counts(counts(gen_bank, real_bank, k, real_radii, rank, world).tolist(), k)


class PrMetric(HookMetric):
    """real = the real data's FeatureBank, its radii in state["pr_real_radii"].  The four values of the bank the hook
    filled: three fused k-NN passes, the same values for every world size."""
    key, uses_bank = "pr", True

    def finish(self, tag, bank):
        v = precision_recall(bank, self.real, self.args.pr_neighbours, self.state["pr_real_radii"], self.rank, self.world)
        if self.rank == 0:
            print('%sprecision was %.4f, recall was %.4f, density was %.4f, coverage was %.4f' % ((tag,) + v))
        return v
