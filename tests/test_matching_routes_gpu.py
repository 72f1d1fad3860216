"""GPU: the training-mode matching entry points (otgan_matching_two_batch_grad_f32, _rows_grad_, the two single-batch ones)
and the inference row variant on every kernel route of csrc/sinkhorn.hip, through the C ABI: the calls of
tests/matching_routes.py -- pitched and offset buffers, ragged row ranges, 128 < N < 256, N >= 256 off the split-precision
engine's shapes, every way out of that engine, N > 1024 -- against the fp64 oracle on the fp32 inputs (oracle/matching_np.py).

Per call: return code and failure word; grad_a / grad_b to conftest.REL_DIFF_INJECTED relative L2 over the range, the distance
to 1e-4 |ref| + 1e-7, the entropy to 2e-4 (the project's figures for these quantities on the shipped routes, not loosened per
route; the inference variant's four arrays to the 2e-4 of tests/test_matching_gpu.py and their differences to its
2 x REL_DIFF_INJECTED, two separately rounded arrays); the outputs' padding columns, guard rows and the floats in front of an
offset output bit for bit untouched, no valid element left unwritten; the workspace used within the queried size;
need_b = 0 bit-identical in grad_a; pitched and packed twins bit-identical; with and without K_pre; a rows call's statistics
equal to the full call's to 1e-12 wherever both solve the same log-kernels (the same cost route; with K_pre or another cost
kernel the log-kernels differ in their last bits and so do the sums).

Worst relative L2 error of the injected gradients per (cost, Sinkhorn, plan application) route, printed by `pytest -s`;
measured on an MI355X:
  plan application on the split-precision engine (ragged row counts, N = 256 ... 1056)         4.6e-6 two-batch, 6.0e-6 single
  plan_apply128_h2_kernel, kdim <= 128                                                         5.0e-6 two-batch, 6.6e-6 single
  plan_apply128_h2_kernel, kdim = 144 ... 288 (3 / 2 terms; the a-priori 2^13 scales hold)     6.3e-6 two-batch, 6.8e-6 single
  plan_apply128_h2_kernel, kdim = 1040 (multi-launch Sinkhorn)                                 4.8e-6
  plan_apply_kernel<true> / <false>                                                            7.3e-6 / 7.2e-6
  inference row variant, differences of its arrays                                             6.3e-6
  distance 2.5e-6 relative at most, entropy 3.9e-7; otgan_plan_apply_f32 pitched 3.0e-7.
Before the engine's row-range condition was narrowed to row_begin % 32 == 0 (csrc/sinkhorn.hip, x3_row_begin_ok) the call
x3_smallest rows [240, 256) returned the rows 16 in front of them: relative error 1.35.
"""
import ctypes

import numpy as np
import pytest
import torch

import matching_routes as R
from conftest import REL_DIFF_INJECTED

pytestmark = pytest.mark.gpu
REL_FEAT = 2e-4          # matched arrays of the inference entry points (tests/test_matching_gpu.py)
REL_LOSS = 1e-4
SENT = 0x7FC0BEEF        # a NaN bit pattern no kernel produces
GUARD = 4                # guard rows on either side of an output
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from otgan_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    for key in sorted(WORST):
        print("worst", key, "grad %.2e  dist %.2e  entropy %.2e" % tuple(WORST[key]))


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)


class Inputs:
    """fa / fb of a case inside [rows, ldf] buffers (+ in_off floats), padding 7.0 / -3.0: finite, a kernel may read inside the
    buffer and mask.  `packed`: the same features as contiguous tensors (for the log-kernels handed in as K_pre)."""

    def __init__(self, case, dev):
        fa, fb = R.features(case)
        rows, D = fa.shape
        self.ldf = D + case["ldf_pad"]
        self.packed, self.bufs, self.ptrs = [], [], []
        for x, fill in ((fa, 7.0), (fb, -3.0)):
            buf = torch.full((rows * self.ldf + case["in_off"] + 8,), fill, dtype=torch.float32, device=dev)
            assert buf.data_ptr() % 256 == 0
            t = torch.as_tensor(x, device=dev)
            buf[case["in_off"]:case["in_off"] + rows * self.ldf].view(rows, self.ldf)[:, :D] = t
            self.packed.append(t)
            self.bufs.append(buf)
            self.ptrs.append(buf.data_ptr() + 4 * case["in_off"])
        self.k_pre = None

    def log_kernels(self, case):
        """two-batch: a1a2, b2b1, a1b1, a1b2, a2b1, a2b2; single-batch: aa and bb with 999 on the diagonal, then ab"""
        from otgan_amd.utils import matching
        if self.k_pre is None:
            a, b = self.packed
            N = case["N"]
            if case["mode"] == "two":
                a1, a2, b1, b2 = a[:N], a[N:], b[:N], b[N:]
                self.k_pre = matching.cost_log_kernels([a1, b2, a1, a1, a2, a2], [a2, b1, b1, b2, b1, b2], R.LAMBDA).clone()
            else:
                self.k_pre = torch.stack([matching.cost_log_kernel(a, a, R.LAMBDA, diag_add=999.0),
                                          matching.cost_log_kernel(b, b, R.LAMBDA, diag_add=999.0),
                                          matching.cost_log_kernel(a, b, R.LAMBDA)]).contiguous()
        return self.k_pre


class OutBuf:
    """[GUARD + rows + GUARD, ldo] floats (+ out_off in front), pre-filled with SENT; the call gets row GUARD"""

    def __init__(self, rows, D, ldo, off, dev):
        self.rows, self.D, self.ldo, self.off = rows, D, ldo, off
        self.buf = torch.full(((rows + 2 * GUARD) * ldo + off + 8,), SENT, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + 4 * (off + GUARD * ldo)

    def _valid(self, t):
        return t[self.off:self.off + (self.rows + 2 * GUARD) * self.ldo].view(self.rows + 2 * GUARD, self.ldo)[GUARD:GUARD + self.rows, :self.D]

    def untouched(self):
        return bool((self.buf == SENT).all())

    def check(self, what):
        """everything outside the valid [rows, D] block is the sentinel bit for bit, nothing inside it is"""
        valid = self._valid(self.buf)
        assert not bool((valid == SENT).any()), what + ": an element of the valid block was not written"
        rest = self.buf.clone()
        self._valid(rest).fill_(SENT)
        bad = int((rest != SENT).sum())
        assert bad == 0, "%s: %d floats outside the valid block were written (padding / guard rows / offset)" % (what, bad)
        return valid.contiguous().view(torch.float32)


def run_call(case, inp, rng, k_pre, need_b, dev, want_stats=True):
    """one call of the case's entry point -> dict(out=[float tensors], entropy, dist, stats)"""
    from otgan_amd import _lib
    L = _lib.lib()
    N, D = case["N"], case["D"]
    single, infer = case["mode"] == "single", case["entry"] == "infer"
    P = 3 if single else 6
    cnt = R.problem_rows(case) if rng is None else rng[1]
    ldo = D + case["ldo_pad"]
    nout = 4 if infer else 2
    outs = [OutBuf(cnt, D, ldo, case["out_off"], dev) for _ in range(nout)]
    passed = [o.ptr for o in outs]
    if not need_b:
        passed[1] = None                                     # the buffer stays, unpassed: it must come back untouched
    if infer:
        need = L.otgan_matching_workspace_bytes(0, N, D)
    else:
        need = (L.otgan_matching_single_batch_grad_workspace_bytes if single else L.otgan_matching_grad_workspace_bytes)(N, D)
    need = int(need)
    big = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=dev)
    assert big.data_ptr() % 256 == 0
    ent = torch.full((), float("nan"), dtype=torch.float32, device=dev)
    dist = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    stats = torch.full((P, 4), float("nan"), dtype=torch.float64, device=dev)
    head = (inp.ptrs[0], inp.ptrs[1], N, D, inp.ldf, R.LAMBDA, case["iters"])
    tail = (*passed, ldo, ent.data_ptr(), dist.data_ptr(), stats.data_ptr() if want_stats else None, big.data_ptr() + 256, need,
            _lib.stream_ptr())
    K = inp.log_kernels(case) if k_pre else None
    if rng is None:
        name = "otgan_matching_%s_batch_grad_f32" % ("single" if single else "two")
        rc = getattr(L, name)(*head, *tail)
    else:
        name = "otgan_matching_two_batch_rows_f32" if infer else "otgan_matching_%s_batch_rows_grad_f32" % ("single" if single else "two")
        rc = getattr(L, name)(*head, int(rng[0]), int(rng[1]), _lib.ptr(K), *tail)
    what = "%s %s range %s k_pre %s need_b %s" % (case["name"], name, rng, k_pre, need_b)
    assert rc == 0, (what, rc, L.otgan_last_error())
    torch.cuda.synchronize()
    # the workspace: nothing in front of it, nothing in the 256 bytes behind the size the query reported
    assert bool((big[:256] == 0xA5).all()) and bool((big[256 + need:] == 0xA5).all()), what + ": wrote outside its workspace"
    res = dict(what=what, entropy=float(ent), dist=float(dist), stats=stats.cpu().numpy() if want_stats else None)
    res["out"] = [o.check(what) if p is not None else None for o, p in zip(outs, passed)]
    if not need_b:
        assert outs[1].untouched(), what + ": grad_b buffer touched by a call that was given none"
    if want_stats:
        assert np.all(res["stats"][:, 3] == 0.0), (what, res["stats"])
    return res


def check_against_oracle(case, rng, k_pre, res):
    ref = R.reference(case)
    b, n = (0, R.problem_rows(case)) if rng is None else rng
    sl = slice(b, b + n)
    want_a, want_b = ref["aa"][sl] - ref["ab"][sl], ref["bb"][sl] - ref["ba"][sl]
    out = [None if o is None else o.cpu().numpy().astype(np.float64) for o in res["out"]]
    if case["entry"] == "infer":
        for o, k in zip(out, ("aa", "bb", "ab", "ba")):
            e = _rel(o, ref[k][sl])
            assert e < REL_FEAT, (res["what"], k, e)
        ea, eb, tol = _rel(out[0] - out[2], want_a), _rel(out[1] - out[3], want_b), 2 * REL_DIFF_INJECTED
    else:
        ea, eb, tol = _rel(out[0], want_a), (_rel(out[1], want_b) if out[1] is not None else 0.0), REL_DIFF_INJECTED
    ed = abs(res["dist"] - ref["dist"])
    ee = abs(res["entropy"] - ref["entropy"]) / abs(ref["entropy"])
    route = R.expected_route(case, rng, k_pre)
    key = (case["mode"], case["entry"]) + route
    w = WORST.setdefault(key, [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], ea, eb), max(w[1], ed / abs(ref["dist"])), max(w[2], ee)
    print("%-90s %s grad_a %.2e grad_b %.2e dist %.2e (rel %.1e) entropy %.1e" % (res["what"], "/".join(route), ea, eb, ed,
                                                                                  ed / abs(ref["dist"]), ee))
    assert ea < tol and eb < tol, (res["what"], route, ea, eb, tol)
    assert ed <= REL_LOSS * abs(ref["dist"]) + 1e-7, (res["what"], res["dist"], ref["dist"])
    assert ee <= 2e-4, (res["what"], res["entropy"], ref["entropy"])


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_matching_route(dev, case):
    inp = Inputs(case, dev)
    twin = R.packed_twin(case)
    twin_inp = Inputs(twin, dev) if twin else None
    full = {}
    for rng, k_pre in R.calls(case):
        res = run_call(case, inp, rng, k_pre, True, dev)
        check_against_oracle(case, rng, k_pre, res)
        if rng is None:
            full = res
        elif full and not k_pre and R.expected_route(case, rng, False)[:2] == R.expected_route(case, None, False)[:2]:
            # the same log-kernels, the same Sinkhorn kernel: the same sums (fp64 atomics at N > 1024: 1e-12)
            part, whole = res["stats"][:, :3], full["stats"][:, :3]
            assert np.all(np.abs(part - whole) <= 1e-12 * np.abs(whole)), (res["what"], part, whole)
        if case["entry"] == "grad":
            gen = run_call(case, inp, rng, k_pre, False, dev, want_stats=False)     # generator step: grad_b == NULL, stats == NULL
            assert torch.equal(gen["out"][0].view(torch.int32), res["out"][0].view(torch.int32)), res["what"] + ": need_b = 0 differs"
            # (the statistics are sums by fp64 atomics: 1e-12 relative each, |sum c_p T_p| / denom <= 2 for the distance)
            assert abs(gen["dist"] - res["dist"]) <= 2e-12 and gen["entropy"] == pytest.approx(res["entropy"], rel=1e-6), res["what"]
        if twin:
            flat = run_call(twin, twin_inp, rng, k_pre, True, dev)
            for o, p in zip(res["out"], flat["out"]):
                assert torch.equal(o.view(torch.int32), p.view(torch.int32)), res["what"] + ": pitched and packed calls differ"


def test_matching_route_error_paths(dev):
    """calls the entry points refuse: OTGAN_ERR_INVALID, and the outputs stay untouched"""
    from otgan_amd import _lib
    L = _lib.lib()
    INVALID = -1
    N, D = 32, 64
    case = R._case("errors", "two", N, D, [None])
    inp = Inputs(case, dev)
    s = _lib.stream_ptr()
    sc = lambda: (torch.full((), float("nan"), dtype=torch.float32, device=dev), torch.full((), float("nan"), dtype=torch.float64, device=dev))
    need = int(L.otgan_matching_grad_workspace_bytes(N, D))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def refused(rc, outs, ent, dist, text=None):
        assert rc == INVALID, rc
        if text:
            assert text in L.otgan_last_error().decode(), L.otgan_last_error()
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs) and np.isnan(float(ent)) and np.isnan(float(dist))

    for ldf, ldo in ((D - 1, D), (D, D - 4)):
        for single in (False, True):
            outs = [OutBuf(2 * N, D, D, 0, dev) for _ in range(2)]
            ent, dist = sc()
            n = 2 * N if single else N
            need_g = int((L.otgan_matching_single_batch_grad_workspace_bytes if single else L.otgan_matching_grad_workspace_bytes)(n, D))
            wsg = torch.empty(need_g, dtype=torch.uint8, device=dev)
            fn = L.otgan_matching_single_batch_grad_f32 if single else L.otgan_matching_two_batch_grad_f32
            rc = fn(inp.ptrs[0], inp.ptrs[1], n, D, ldf, R.LAMBDA, 5, outs[0].ptr, outs[1].ptr, ldo, ent.data_ptr(), dist.data_ptr(),
                    None, wsg.data_ptr(), need_g, s)
            refused(rc, outs, ent, dist)
            rc = (L.otgan_matching_single_batch_rows_grad_f32 if single else L.otgan_matching_two_batch_rows_grad_f32)(
                inp.ptrs[0], inp.ptrs[1], n, D, ldf, R.LAMBDA, 5, 0, 16, None, outs[0].ptr, outs[1].ptr, ldo, ent.data_ptr(),
                dist.data_ptr(), None, wsg.data_ptr(), need_g, s)
            refused(rc, outs, ent, dist)
    # the inference entry points that walk their arrays linearly take packed arrays only
    for mode, fn, n in ((0, L.otgan_matching_two_batch_f32, N), (1, L.otgan_matching_single_batch_f32, 2 * N)):
        need_i = int(L.otgan_matching_workspace_bytes(mode, n, D))
        wsi = torch.empty(need_i, dtype=torch.uint8, device=dev)
        pitched = Inputs(R._case("errors", "two", N, D, [None], ldf_pad=4), dev)
        for src, ldf, ldo in ((pitched, D + 4, D), (inp, D, D + 4)):
            outs = [OutBuf(2 * N, D, ldo, 0, dev) for _ in range(4)]
            ent, dist = sc()
            extra = (0,) if mode == 0 else ()
            rc = fn(src.ptrs[0], src.ptrs[1], n, D, ldf, R.LAMBDA, 5, *extra, *[o.ptr for o in outs], ldo, ent.data_ptr(),
                    dist.data_ptr(), None, wsi.data_ptr(), need_i, s)
            refused(rc, outs, ent, dist, "contiguous")
    # the stack variant refuses what the others fall back on: a row range that does not start on a multiple of 32
    N, D = 256, 64
    case = R._case("errors_stack", "two", N, D, [None])
    inp = Inputs(case, dev)
    nbytes = int(L.otgan_matching_stack_bytes(N, D))
    assert nbytes > 0
    stack = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    begin, count = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(6 * N)
    _lib.check(L.otgan_matching_stack_split_f32(inp.ptrs[0], inp.ptrs[1], N, D, D, 1, ctypes.cast(begin, ctypes.c_void_p),
                                                ctypes.cast(count, ctypes.c_void_p), stack.data_ptr(), s), "stack split")
    K = inp.log_kernels(case)
    need = int(L.otgan_matching_grad_workspace_bytes(N, D))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for row_begin, ok in ((8, False), (16, False), (32, True)):
        outs = [OutBuf(32, D, D, 0, dev) for _ in range(2)]
        ent, dist = sc()
        rc = L.otgan_matching_two_batch_rows_grad_stack_f32(stack.data_ptr(), N, D, R.LAMBDA, 5, row_begin, 32, K.data_ptr(), outs[0].ptr,
                                                            outs[1].ptr, D, ent.data_ptr(), dist.data_ptr(), None, ws.data_ptr(), need, s)
        if ok:
            assert rc == 0, L.otgan_last_error()
            torch.cuda.synchronize()
            outs[0].check("stack rows call")
        else:
            refused(rc, outs, ent, dist)


@pytest.mark.parametrize("rows,kdim,D", [(130, 72, 100), (5, 257, 66)])
def test_plan_apply_pitched(dev, rows, kdim, D):
    """otgan_plan_apply_f32 with ldp > kdim, ldf > D, ldo > D: the fp64 product to 2e-6 (tests/test_matching_gpu.py), padding and
    guard rows untouched; pitches that keep 16-byte rows and pitches that do not"""
    from otgan_amd import _lib
    L = _lib.lib()
    rng = np.random.RandomState(rows + kdim + D)
    P, F = rng.rand(rows, kdim).astype(np.float32), rng.randn(kdim, D).astype(np.float32)
    ref = 0.5 * (P.astype(np.float64) @ F.astype(np.float64))
    for padp, padf, pado in ((4, 4, 4), (3, 1, 5)):
        ldp, ldf, ldo = kdim + padp, D + padf, D + pado
        pw, fw = torch.full((rows, ldp), 7.0, device=dev), torch.full((kdim, ldf), -3.0, device=dev)
        pw[:, :kdim], fw[:, :D] = torch.as_tensor(P, device=dev), torch.as_tensor(F, device=dev)
        out = OutBuf(rows, D, ldo, 0, dev)
        _lib.check(L.otgan_plan_apply_f32(pw.data_ptr(), ldp, rows, kdim, fw.data_ptr(), ldf, D, 0.5, out.ptr, ldo, _lib.stream_ptr()),
                   "apply")
        torch.cuda.synchronize()
        got = out.check("plan apply %s" % ((ldp, ldf, ldo),))
        e = _rel(got.cpu().numpy(), ref)
        print("plan_apply", (rows, kdim, D), (ldp, ldf, ldo), "rel %.2e" % e)
        assert e < 2e-6, e
