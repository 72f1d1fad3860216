"""GPU: training-mode matching (otgan_matching_two_batch_grad_f32 / _rows_grad_): the injected gradients
`features_a_a - features_a_b` (reference train.py:111) and `features_b_b - features_b_a` (train.py:125-126) and the
closed-form distance, against the fp64 oracle (oracle/matching_np.py, pinned to the reference-generated fixtures) and
against the reference-generated golden vectors themselves.  Tolerances: differences `conftest.REL_DIFF_INJECTED` relative L2
(3 x what tests/test_matching_engine_accuracy_gpu.py measures for the shipped engines; 2e-3 until round 4), loss 1e-4 relative
-- the north-star figure."""
import numpy as np
import pytest
import torch

from conftest import REL_DIFF_INJECTED
from oracle import matching_np as M

pytestmark = pytest.mark.gpu
REL_DIFF = REL_DIFF_INJECTED
REL_LOSS = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from otgan_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)


def test_grad_vs_golden(dev, list_case):
    """the five reference-generated fixtures: grad = two_aa - two_ab, two_bb - two_ba of the reference's own outputs"""
    from otgan_amd.utils import matching
    g = list_case
    fa = _t(np.concatenate(list(g["fa"])), dev)
    fb = _t(np.concatenate(list(g["fb"])), dev)
    ga, gb, ent, dist = matching.matched_feature_grads(fa, fb, float(g["lam"]), int(g["iters"]))
    ra = np.concatenate(list(g["two_aa"])) - np.concatenate(list(g["two_ab"]))
    rb = np.concatenate(list(g["two_bb"])) - np.concatenate(list(g["two_ba"]))
    assert _rel(ga.cpu().numpy(), ra) < REL_DIFF
    assert _rel(gb.cpu().numpy(), rb) < REL_DIFF
    assert float(ent) == pytest.approx(float(g["two_entropy"]), rel=2e-4)
    ref = float(g["two_distance"])
    atol = 2e-6 if g["name"] == "survey" else 1e-7         # (see tests/test_matching_gpu.py::_loss_ok)
    assert abs(float(dist) - ref) <= REL_LOSS * abs(ref) + atol
    # generator steps: no data-side gradient; the generated-side one is the same bits
    ga2, gb2, _, dist2 = matching.matched_feature_grads(fa, fb, float(g["lam"]), int(g["iters"]), need_b=False)
    assert gb2 is None and torch.equal(ga2, ga) and float(dist2) == float(dist)


def _clustered(seed, rows, D):
    rng = np.random.RandomState(seed)
    ca, cb = rng.randn(32, D), rng.randn(32, D)
    fa = M.clustered_features(rng, rows, D, ca).astype(np.float32)
    fb = M.clustered_features(rng, rows, D, cb).astype(np.float32)
    return fa, fb


@pytest.mark.parametrize("N,D,iters", [(128, 32768, 100),     # configs[1]: the exact-fp32 engine, three-term blocks
                                       (256, 7296, 200),      # configs[3] width: the split-precision engine
                                       (256, 131072, 100)],   # configs[4]: 64x64 critic width
                         ids=["N128_D32768", "N256_D7296", "N256_D131072"])
def test_grad_full_size_vs_oracle(dev, N, D, iters):
    from otgan_amd.utils import matching
    lam = 500.0
    fa, fb = _clustered(3, 2 * N, D)
    A, B = _t(fa, dev), _t(fb, dev)
    ga, gb, ent, dist = matching.matched_feature_grads(A, B, lam, iters)
    f64 = lambda z: z.astype(np.float64)
    fa1, fa2, fb1, fb2 = f64(fa[:N]), f64(fa[N:]), f64(fb[:N]), f64(fb[N:])
    plans, costs, ent_ref = M.two_batch_plans(fa1, fa2, fb1, fb2, lam, iters)
    dref = M.closed_form_from(plans, costs, N)
    ra, rb = [], []
    for half in (0, 1):
        aa, bb, ab, ba = M.matched_rows(plans, fa1, fa2, fb1, fb2, half, 0, N)
        ra.append(aa - ab)
        rb.append(bb - ba)
    assert _rel(ga.cpu().numpy(), np.concatenate(ra)) < REL_DIFF
    assert _rel(gb.cpu().numpy(), np.concatenate(rb)) < REL_DIFF
    assert float(ent) == pytest.approx(float(ent_ref), rel=2e-4)
    assert abs(float(dist) - dref) <= REL_LOSS * abs(dref) + 1e-7, (float(dist), dref)
    # the same differences from the four matched arrays of the inference-mode entry point
    out = matching.get_matched_features([A[:N], A[N:]], [B[:N], B[N:]], lam, iters)
    da = (torch.cat(out[0]) - torch.cat(out[2])).cpu().numpy()
    assert _rel(ga.cpu().numpy(), da) < 1e-4


def test_rows_grad_rank_of_8(dev):
    """the rank-level call of the 8-GPU configurations (N = 1024, 256 rows per rank, D = 7296, 200 iterations), with
    and without precomputed log-kernels, ranks 0, 3, 4, 7 against the oracle's rows"""
    from otgan_amd import trainer
    from otgan_amd.utils import matching
    S, Bs, D, lam, iters, WORLD = 16, 128, 7296, 500.0, 200, 8
    N, nb = S * Bs // 2, 256
    fa_h, fb_h = _clustered(11, 2 * N, D)
    fa_d, fb_d = _t(fa_h, dev), _t(fb_h, dev)
    fa, fb = list(torch.chunk(fa_d, S, 0)), list(torch.chunk(fb_d, S, 0))
    slices = [trainer.rank_log_kernel_slices(r, WORLD, fa_d[r * nb:(r + 1) * nb], fb_d[r * nb:(r + 1) * nb], fa, fb, lam)
              for r in range(WORLD)]
    K = trainer.assemble_log_kernels(torch.stack(slices, 0), WORLD)
    f64 = lambda z: z.astype(np.float64)
    fa1, fa2, fb1, fb2 = f64(fa_h[:N]), f64(fa_h[N:]), f64(fb_h[:N]), f64(fb_h[N:])
    plans, costs, ent_ref = M.two_batch_plans(fa1, fa2, fb1, fb2, lam, iters)
    dref = M.closed_form_from(plans, costs, N)
    for r, pre in ((0, K), (3, None), (4, K), (7, K)):
        ga, gb, ent, dist = matching.matched_feature_grads(fa_d, fb_d, lam, iters, rows=(r * nb, nb), log_kernels=pre)
        half, r0 = divmod(r * nb, N)
        aa, bb, ab, ba = M.matched_rows(plans, fa1, fa2, fb1, fb2, half, r0, r0 + nb)
        assert _rel(ga.cpu().numpy(), aa - ab) < REL_DIFF, r
        assert _rel(gb.cpu().numpy(), bb - ba) < REL_DIFF, r
        assert float(ent) == pytest.approx(float(ent_ref), rel=2e-4)
        assert abs(float(dist) - dref) <= REL_LOSS * abs(dref) + 1e-7, (r, float(dist), dref)
    ga2, gb2, _, _ = matching.matched_feature_grads(fa_d, fb_d, lam, iters, need_b=False, rows=(7 * nb, nb), log_kernels=K)
    assert gb2 is None and torch.equal(ga2, ga)


def test_single_batch_grad_vs_golden(dev, list_case):
    """--single_batch, training mode: grad = single_aa - single_ab, single_bb - single_ba of the reference's own outputs"""
    from otgan_amd.utils import matching
    g = list_case
    fa = _t(np.concatenate(list(g["fa"])), dev)
    fb = _t(np.concatenate(list(g["fb"])), dev)
    ga, gb, ent, dist = matching.matched_feature_grads_single_batch(fa, fb, float(g["lam"]), int(g["iters"]))
    ra = np.concatenate(list(g["single_aa"])) - np.concatenate(list(g["single_ab"]))
    rb = np.concatenate(list(g["single_bb"])) - np.concatenate(list(g["single_ba"]))
    assert _rel(ga.cpu().numpy(), ra) < REL_DIFF
    assert _rel(gb.cpu().numpy(), rb) < REL_DIFF
    assert float(ent) == pytest.approx(float(g["single_entropy"]), rel=2e-4)
    ref = float(g["single_distance"])
    atol = 2e-6 if g["name"] == "survey" else 1e-7
    assert abs(float(dist) - ref) <= REL_LOSS * abs(ref) + atol
    ga2, gb2, _, dist2 = matching.matched_feature_grads_single_batch(fa, fb, float(g["lam"]), int(g["iters"]), need_b=False)
    assert gb2 is None and torch.equal(ga2, ga) and float(dist2) == float(dist)


@pytest.mark.parametrize("lam", [0.02, 0.09, 5.0])
def test_single_batch_closed_form_distance_at_small_lambda(dev, lam):
    """the closed-form single-batch distance holds <M, C + 999 I> in its statistics; the reference's calc_distance
    (matching.py:139-153) is a dot product with the real features, i.e. without the 999.  For lambda * 999 below ~90 the
    diagonal plan entries are not exactly 0 and 999 trace(M) has to be added back: the training-mode entry must agree with
    the oracle (and with the inference-mode entry, which forms the dot products) at small lambda too."""
    from otgan_amd.utils import matching
    S, Bs, D, iters = 4, 16, 96, 30
    fa_h, fb_h = _clustered(17, S * Bs, D)
    fa_d, fb_d = _t(fa_h, dev), _t(fb_h, dev)
    fa64 = list(np.split(fa_h.astype(np.float64), S))
    fb64 = list(np.split(fb_h.astype(np.float64), S))
    ref = M.get_matched_features_single_batch(fa64, fb64, lam, iters)
    dref = float(M.calc_distance(fa64, fb64, ref))
    ga, gb, ent, dist = matching.matched_feature_grads_single_batch(fa_d, fb_d, lam, iters)
    assert abs(float(dist) - dref) <= REL_LOSS * abs(dref) + 1e-7, (lam, float(dist), dref)
    ra = np.concatenate(ref[0]) - np.concatenate(ref[2])
    assert _rel(ga.cpu().numpy(), ra) < REL_DIFF
    out = matching.get_matched_features_single_batch(list(torch.chunk(fa_d, S, 0)), list(torch.chunk(fb_d, S, 0)), lam, iters)
    d2 = float(matching.calc_distance(list(torch.chunk(fa_d, S, 0)), list(torch.chunk(fb_d, S, 0)), out))
    assert abs(d2 - dref) <= REL_LOSS * abs(dref) + 1e-7, (lam, d2, dref)


def test_single_batch_rows_grad_rank_of_8(dev):
    """--single_batch in the global scope, row-sharded like the reference (matching.py:99-104): eight ranks x 128 rows
    (n = 1024, D = 7296, 100 iterations), every rank's three cost row slices assembled into the [3, n, n] log-kernels, the
    rows of ranks 0, 3, 4, 7 -- with the assembled kernels and with the library's own -- against the fp64 oracle; the
    all-rows call on the same inputs must give the same rows"""
    from otgan_amd import trainer
    from otgan_amd.utils import matching
    WORLD, nb, D, lam, iters = 8, 128, 7296, 500.0, 100
    n = WORLD * nb
    fa_h, fb_h = _clustered(13, n, D)
    fa_d, fb_d = _t(fa_h, dev), _t(fb_h, dev)
    slices = [trainer.rank_single_log_kernel_slices(fa_d[r * nb:(r + 1) * nb], fb_d[r * nb:(r + 1) * nb], fa_d, fb_d, lam)
              for r in range(WORLD)]
    K = trainer.assemble_single_log_kernels(torch.stack(slices, 0), lam)
    assert tuple(K.shape) == (3, n, n)
    ref = M.get_matched_features_single_batch(list(np.split(fa_h.astype(np.float64), WORLD)),
                                              list(np.split(fb_h.astype(np.float64), WORLD)), lam, iters)
    dref = float(M.calc_distance(list(np.split(fa_h.astype(np.float64), WORLD)), list(np.split(fb_h.astype(np.float64), WORLD)), ref))
    ra = np.concatenate(ref[0]) - np.concatenate(ref[2])
    rb = np.concatenate(ref[1]) - np.concatenate(ref[3])
    full_a, full_b, ent_f, dist_f = matching.matched_feature_grads_single_batch(fa_d, fb_d, lam, iters)
    assert _rel(full_a.cpu().numpy(), ra) < REL_DIFF and _rel(full_b.cpu().numpy(), rb) < REL_DIFF
    assert abs(float(dist_f) - dref) <= REL_LOSS * abs(dref) + 1e-7, (float(dist_f), dref)
    for r, pre in ((0, K), (3, None), (4, K), (7, K)):
        ga, gb, ent, dist = matching.matched_feature_grads_single_batch(fa_d, fb_d, lam, iters, rows=(r * nb, nb), log_kernels=pre)
        sl = slice(r * nb, (r + 1) * nb)
        assert _rel(ga.cpu().numpy(), ra[sl]) < REL_DIFF, r
        assert _rel(gb.cpu().numpy(), rb[sl]) < REL_DIFF, r
        assert _rel(ga.cpu().numpy(), full_a[sl].cpu().numpy()) < 1e-5, r
        assert float(ent) == pytest.approx(float(ref[4]), rel=2e-4)
        assert abs(float(dist) - dref) <= REL_LOSS * abs(dref) + 1e-7, (r, float(dist), dref)
    ga2, gb2, _, _ = matching.matched_feature_grads_single_batch(fa_d, fb_d, lam, iters, need_b=False, rows=(7 * nb, nb), log_kernels=K)
    assert gb2 is None and torch.equal(ga2, ga)


def test_grad_abi_errors(dev):
    from otgan_amd import _lib
    from otgan_amd.utils import matching
    fa = torch.rand(64, 32, device=dev)
    with pytest.raises(_lib.OtganError):
        matching.matched_feature_grads(fa, fa, 10.0, 5, rows=(24, 16))        # straddles the two mini-batches
    with pytest.raises(_lib.OtganError):
        matching.matched_feature_grads(fa.cpu(), fa.cpu(), 10.0, 5)
    with pytest.raises(ValueError):
        matching.matched_feature_grads(fa[:63], fa[:63], 10.0, 5)


@pytest.mark.parametrize("N,D", [(32, 64),      # the fp32 engines, the one-workgroup Sinkhorn kernel
                                 (256, 64)],    # the split-precision engine, the panel kernel
                         ids=["N32", "N256"])
def test_grad_entry_points_copy_their_statistics_out(dev, N, D):
    """The four training-mode entry points with `stats != NULL` (every Python caller passes None): the [P, 4] fp64 statistics
    {row-entropy sum, <M, C>, sum(M), failure} they copy out must be the ones their own results were formed from.
      distance = the closed form evaluated here in fp64 -- two-batch (2 T0 + 2 T1 - T2 - T3 - T4 - T5) / (4 N), single-batch
                 (T1 + T0 - 2 T2) / (2 n), T = stats[:, 2] - stats[:, 1] -- to 16 * 2^-53 * sum |c_p T_p| / denom: the device
                 compiler's fused multiply-adds over a handful of fp64 operations, nothing else.  The single-batch kernel adds
                 999 trace(M_aa), 999 trace(M_bb), exactly 0 at lambda = 500 (exp(-499 500 + potentials) underflows): asserted
                 on the plans of the staged entry points (otgan_cost_matrix_f32 with 999 on the diagonal, then
                 otgan_sinkhorn_plan_f32) -- get_matched_features_single_batch returns matched features and statistics, from
                 which no diagonal can be read.
      entropy  = float32(mean_p(stats[p, 0] / n)) to one fp32 ulp.
      a rows call returns the statistics of the full call on the same input to 1e-12 relative (sums by fp64 atomics)."""
    from otgan_amd import _lib
    from otgan_amd.utils import matching
    L = _lib.lib()
    lam, iters = 500.0, 10
    rng = np.random.RandomState(23)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    fa, fb = _t(unit(rng.randn(2 * N, D)), dev), _t(unit(rng.randn(2 * N, D)), dev)
    s = _lib.stream_ptr()

    def call(single, rows):
        n, P = (N, 3) if single else (N, 6)
        a, b = (fa[:N].contiguous(), fb[:N].contiguous()) if single else (fa, fb)
        cnt = rows[1] if rows else a.shape[0]
        ga, gb = torch.empty((cnt, D), device=dev), torch.empty((cnt, D), device=dev)
        ent = torch.empty((), dtype=torch.float32, device=dev)
        dist = torch.empty((), dtype=torch.float64, device=dev)
        stats = torch.full((P, 4), float("nan"), dtype=torch.float64, device=dev)
        need = (L.otgan_matching_single_batch_grad_workspace_bytes if single else L.otgan_matching_grad_workspace_bytes)(n, D)
        ws = torch.empty(int(need), dtype=torch.uint8, device=dev)
        head = (a.data_ptr(), b.data_ptr(), n, D, D, lam, iters)
        tail = (ga.data_ptr(), gb.data_ptr(), D, ent.data_ptr(), dist.data_ptr(), stats.data_ptr(), ws.data_ptr(), int(need), s)
        name = "otgan_matching_%s_batch_%sgrad_f32" % ("single" if single else "two", "rows_" if rows else "")
        mid = (int(rows[0]), int(rows[1]), None) if rows else ()
        _lib.check(getattr(L, name)(*head, *mid, *tail), name)
        st = stats.cpu().numpy()
        T = st[:, 2] - st[:, 1]
        c = np.array([1.0, 1.0, -2.0] if single else [2.0, 2.0, -1.0, -1.0, -1.0, -1.0])
        denom = 2.0 * n if single else 4.0 * n
        want = float(np.dot(c, T)) / denom
        tol = 16 * 2.0 ** -53 * float(np.sum(np.abs(c * T))) / denom
        print(name, "distance", float(dist), "closed form", want, "tol", tol, "entropy", float(ent))
        assert np.all(st[:, 3] == 0.0), st
        assert abs(float(dist) - want) <= tol, (name, float(dist), want, tol)
        ent_want = np.float32(np.mean(st[:, 0] / n))
        assert abs(np.float32(float(ent)) - ent_want) <= np.spacing(ent_want), (name, float(ent), ent_want)
        return st

    # the single-batch closed form holds only with no mass on the diagonals of the a-a and b-b plans
    for x in (fa[:N].contiguous(), fb[:N].contiguous()):
        K = matching.cost_log_kernel(x, x, lam, diag_add=999.0).contiguous()
        plan, planT = torch.empty_like(K), torch.empty_like(K)
        pst = torch.empty((1, 4), dtype=torch.float64, device=dev)
        need = L.otgan_sinkhorn_workspace_bytes(1, N, N)
        ws = torch.empty(int(need), dtype=torch.uint8, device=dev)
        _lib.check(L.otgan_sinkhorn_plan_f32(K.data_ptr(), 1, N, N, iters, lam, plan.data_ptr(), planT.data_ptr(), pst.data_ptr(),
                                             ws.data_ptr(), int(need), s), "otgan_sinkhorn_plan_f32")
        assert float(plan.diagonal().abs().max()) == 0.0

    for single, rows in ((False, (N + N // 2, N // 2)), (True, (N // 2, N // 2))):
        full, part = call(single, None), call(single, rows)
        assert np.all(np.abs(part[:, :3] - full[:, :3]) <= 1e-12 * np.abs(full[:, :3])), (single, part, full)
