"""CPU: the references and detectors of tests/pointwise_ref.py.  Three parts: the fp64 references agree with the oracle
(oracle/nets_torch.py) where it has the operation; the float32 optimiser emulations agree with their fp64 forms; and every
comparison helper FIRES on the output of a deliberately wrong numpy implementation -- the proof that
tests/test_pointwise_edges_gpu.py would fail if a kernel were subtly wrong (no mutated kernel is ever built or run)."""
import numpy as np
import pytest
import torch

import pointwise_ref as R
from oracle import nets_torch as O


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- references vs the oracle
def test_references_agree_with_the_oracle():
    g = _gen(1)
    V = torch.randn(3, 3, 7, 5, generator=g, dtype=torch.float64)
    gain = torch.rand(5, generator=g, dtype=torch.float64) + 0.5
    w, inv = R.weight_norm_fwd(V.reshape(-1, 5), gain)
    assert float((w.reshape(V.shape) - O.weight_norm(V, gain)).abs().max()) <= 1e-12
    assert float((inv - torch.rsqrt((V * V).sum((0, 1, 2)))).abs().max()) <= 1e-12

    x = torch.randn(2, 3, 3, 12, generator=g, dtype=torch.float64) * 4
    assert float((R.glu_fwd(x) - O.glu(x, 3)).abs().max()) <= 1e-12
    dy = torch.randn(2, 3, 3, 6, generator=g, dtype=torch.float64)
    xo = x.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(O.glu(xo, 3), xo, dy)
    assert float((R.glu_bwd(x, dy) - ref).abs().max()) <= 1e-12

    h = torch.randn(3, 2, 2, 5, generator=g, dtype=torch.float64)
    f, norm = R.feature_head_fwd(h.reshape(3, 4, 5))
    assert float((f - O.feature_head(h)).abs().max()) <= 1e-12
    assert float((norm - h.reshape(3, -1).norm(dim=1)).abs().max()) <= 1e-12
    df = torch.randn(3, 40, generator=g, dtype=torch.float64)
    ho = h.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(O.feature_head(ho), ho, df)
    assert float((R.feature_head_bwd(h.reshape(3, 4, 5), df).reshape(h.shape) - ref).abs().max()) <= 1e-12


def test_weight_norm_backward_is_the_oracles_gradient():
    g = _gen(2)
    V = torch.randn(18, 4, generator=g, dtype=torch.float64)
    gain = torch.rand(4, generator=g, dtype=torch.float64) + 0.5
    dw = torch.randn(18, 4, generator=g, dtype=torch.float64)
    Vo, go = V.clone().requires_grad_(True), gain.clone().requires_grad_(True)
    rV, rg = torch.autograd.grad(O.weight_norm(Vo, go), [Vo, go], dw)
    dV, dg = R.weight_norm_bwd(V, gain, dw)
    assert float((dV - rV).abs().max()) <= 1e-12 and float((dg - rg).abs().max()) <= 1e-12


def test_fp64_optimiser_steps_agree_with_the_oracle():
    g = _gen(3)
    n = 257
    p, gr, v, mg = (torch.randn(n, generator=g, dtype=torch.float64) for _ in range(4))
    mg = mg.abs()
    for mom1 in (0.5, 0.0):
        for t in (1, 2, 7):
            st = {"t": t, "v": v.clone(), "mg": mg.clone()}
            ref = O.adam_update(p, gr, st, 3e-4, mom1, 0.999)
            c1 = float(np.float32(1) - np.float32(mom1) ** np.float32(t))
            c2 = float(np.float32(1) - np.float32(0.999) ** np.float32(t))
            pn, vn, mgn = R.adam64(p, gr, v, mg, 3e-4, mom1, 0.999, c1, c2)
            assert np.abs(pn - ref.numpy()).max() <= 1e-12 and np.abs(mgn - st["mg"].numpy()).max() <= 1e-12
            if mom1 > 0:
                assert np.abs(vn - st["v"].numpy()).max() <= 1e-12
        st = {"v": v.clone(), "mg": mg.clone()}
        ref = O.adamax_update(p, gr, st, 3e-4, mom1, 0.999)
        pn, vn, mgn = R.adamax64(p, gr, v, mg, 3e-4, mom1, 0.999)
        assert np.abs(pn - ref.numpy()).max() <= 1e-12 and np.abs(mgn - st["mg"].numpy()).max() <= 1e-12
    st = {"v": v.clone()}
    ref = O.nesterov_update(p, gr, st, 3e-4, 0.9)
    pn, vn = R.nesterov64(p, gr, v, 3e-4, 0.9)
    assert np.abs(pn - ref.numpy()).max() <= 1e-12 and np.abs(vn - st["v"].numpy()).max() <= 1e-12


def _rel(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


def test_float32_emulations_agree_with_fp64():
    """3e-7 relative: the bound tests/test_reference_run_gpu.py holds the optimiser kernels to."""
    g = _gen(4)
    n = 4099
    p, v = torch.randn(n, generator=g), torch.randn(n, generator=g)
    gr = R.optimiser_gradient(n, g)
    mg = gr.abs() * torch.rand(n, generator=g) + 1e-3
    c1, c2 = np.float32(1) - np.float32(0.5) ** np.float32(3), np.float32(1) - np.float32(0.999) ** np.float32(3)
    for mom1 in (0.5, 0.0):
        for lr in (3e-4, -3e-4):
            got = R.adam_f32(p, gr, v, mg, lr, mom1, 0.999, c1, c2)
            ref = R.adam64(p, gr, v, mg, lr, mom1, 0.999, float(c1), float(c2))
            for a, b in zip(got, ref):
                if mom1 > 0 or a is not got[1]:
                    assert _rel(a, b) <= 3e-7
            got = R.adamax_f32(p, gr, v, mg, lr, mom1, 0.999)
            ref = R.adamax64(p, gr, v, mg, lr, mom1, 0.999)
            assert _rel(got[0], ref[0]) <= 3e-7 and _rel(got[2], ref[2]) <= 3e-7
    got, ref = R.nesterov_f32(p, gr, v, 3e-4, 0.9), R.nesterov64(p, gr, v, 3e-4, 0.9)
    assert _rel(got[0], ref[0]) <= 3e-7 and _rel(got[1], ref[1]) <= 3e-7
    assert _rel(R.ema_f32(v, p, 0.999), R.ema64(v, p, 0.999)) <= 3e-7


def test_fma_emulation_is_exact():
    a, b = np.float32(1 + 2 ** -13), np.float32(1 - 2 ** -13)
    assert R.fma_f32(a, b, np.float32(-1.0)) == np.float32(-2.0 ** -26)      # the product rounds to 1.0 in fp32
    assert np.float32(a * b) - np.float32(1.0) == 0.0


# ---------------------------------------------------------------------------------------------- the detectors fire
def _pitched_ints(rows, cols, lda, seed, lead=0):
    g = R.guarded((rows, cols), pitch=lda, lead=lead, bits=R.POISON_BITS)
    g.view.copy_(R.int_valued((rows, cols), -8, 8, _gen(seed)))
    return g


def _full(g):
    """The buffer as the [rows, pitch] matrix a kernel with a wrong column bound would walk."""
    return g.buf[g.start:g.start + g.rows * g.pitch].view(g.rows, g.pitch).numpy()


def test_a_correct_column_sum_passes():
    g = _pitched_ints(100, 36, 52, 0, lead=8)
    R.assert_bits_equal(g.view.numpy().sum(0, dtype=np.float32), R.colsum_exact(g.view).astype(np.float32))


def test_detects_a_column_sum_that_drops_the_last_row():
    g = _pitched_ints(65, 4, 4, 1)
    g.view[-1] = torch.tensor([1.0, -3.0, 8.0, 2.0])           # (a row of zeros would hide the defect)
    with pytest.raises(AssertionError, match="differ in their bits"):
        R.assert_bits_equal(g.view.numpy()[:-1].sum(0, dtype=np.float32), R.colsum_exact(g.view).astype(np.float32))


def test_detects_a_column_sum_that_drops_the_last_row_chunk():
    rows, cols = 16385, 8
    nchunk, per = R.colreduce_geometry(rows, cols)
    assert (nchunk, per) == (256, 65) and (nchunk - 1) * per >= rows        # trailing chunks are empty ...
    last = (rows - 1) // per                                                # ... the last one with rows holds 5
    g = _pitched_ints(rows, cols, cols, 2)
    g.view[last * per:] = 1.0
    with pytest.raises(AssertionError, match="differ in their bits"):
        R.assert_bits_equal(g.view.numpy()[:last * per].sum(0, dtype=np.float32), R.colsum_exact(g.view).astype(np.float32))


def test_detects_a_column_sum_that_reads_a_pitch_column():
    g = _pitched_ints(100, 36, 52, 3, lead=8)
    wrong = _full(g)[:, 1:37].sum(0, dtype=np.float32)                      # off by one column: ends in the pitch
    assert np.isnan(wrong[-1])                                              # the NaN fill poisons it
    with pytest.raises(AssertionError, match="differ in their bits"):
        R.assert_bits_equal(wrong, R.colsum_exact(g.view).astype(np.float32))


def _planted(rows, C, ld, where, seed=5):
    g = R.guarded((rows, C), pitch=ld, bits=R.POISON_BITS)
    g.view.copy_(torch.rand(rows, C, generator=_gen(seed)) * 2 - 1)
    R.plant(g.view, where, -7.0)
    return g


def test_detects_an_amax_that_skips_the_last_quad():
    g = _planted(7, 36, 52, (6, 35))
    assert R.amax_exact(g.view) == np.float32(7.0)
    flat = g.view.numpy().reshape(-1)
    wrong = np.float32(np.abs(flat[:-4]).max())
    assert wrong < 7.0
    with pytest.raises(AssertionError):
        R.assert_bits_equal(wrong, R.amax_exact(g.view))


def test_detects_an_amax_that_includes_a_pitch_column():
    g = _planted(7, 36, 52, (0, 0))
    wide = _full(g)[:, :37]
    a = np.abs(wide)
    wrong = np.float32(np.nan) if np.isnan(a).any() else np.float32(a.max())
    with pytest.raises(AssertionError):
        R.assert_bits_equal(wrong, R.amax_exact(g.view))                    # NaN from the fill ...
    _full(g)[:, 36] = 1e30                                                  # ... or a larger finite value there
    with pytest.raises(AssertionError):
        R.assert_bits_equal(np.float32(np.abs(_full(g)[:, :37]).max()), R.amax_exact(g.view))


def test_record_value_reads_bit_patterns():
    rec = np.zeros(R.AMAX_RECORD_FLOATS, dtype=np.float32)
    rec[3 * 32], rec[5 * 32], rec[1] = 2.5, 7.0, 99.0                      # (floats between the sub-slots do not count)
    assert R.record_value(rec) == np.float32(7.0)
    rec[9 * 32] = np.inf
    assert np.isinf(R.record_value(rec))
    rec[0] = np.nan
    assert np.isnan(R.record_value(rec))


def test_detects_a_copy_that_writes_one_column_too_many():
    rows, cols = 5, 7
    src = R.guarded((rows, cols), pitch=12, bits=R.POISON_BITS)
    src.view.copy_(torch.randn(rows, cols, generator=_gen(6)))
    dst = R.guarded((rows, cols), pitch=9)
    _full(dst)[:, :cols] = _full(src)[:, :cols]
    R.assert_bits_equal(dst.view, src.view)
    R.assert_guards_intact(dst)
    _full(dst)[:, :cols + 1] = _full(src)[:, :cols + 1]
    R.assert_bits_equal(dst.view, src.view)                                 # the payload is still right ...
    with pytest.raises(AssertionError, match="pitch column"):
        R.assert_guards_intact(dst)                                         # ... the guard is not


def test_guards_see_writes_in_front_and_behind():
    for lead in (0, 1, 8):
        g = R.guarded((3, 4), lead=lead)
        assert g.view.data_ptr() - g.buf.data_ptr() == 4 * (R.GUARD + lead)
        g.view.zero_()
        R.assert_guards_intact(g)
        g.buf[g.start - 1] = 0.0
        with pytest.raises(AssertionError, match="in front"):
            R.assert_guards_intact(g)
        g = R.guarded((2, 3, 4), pitch=6)
        assert g.view.stride() == (18, 6, 1)
        g.buf[g.start + 6 * 6] = 1.0
        with pytest.raises(AssertionError, match="behind"):
            R.assert_guards_intact(g)
    g = R.guarded((4,))
    g.buf.view(torch.int32)[3] = R.SENTINEL_BITS ^ 1                        # another NaN: only the bit pattern tells
    with pytest.raises(AssertionError):
        R.assert_guards_intact(g)


def test_detects_a_transpose_that_skips_the_last_ragged_tile():
    K, Cout = 65, 68
    w = torch.randn(K, Cout, generator=_gen(7)).numpy()
    out = R.guarded((Cout, K))
    out.view.zero_()
    o = out.view.numpy()
    for k0 in range(0, K - K % 32, 32):                                     # full tiles only
        o[:, k0:k0 + 32] = w[k0:k0 + 32].T
    with pytest.raises(AssertionError, match="differ in their bits"):
        R.assert_bits_equal(out.view, w.T)
    o[:, K - K % 32:] = w[K - K % 32:].T
    R.assert_bits_equal(out.view, w.T)
    R.assert_guards_intact(out)


@pytest.mark.parametrize("fused", ["v", "mg", "p"])
def test_detects_an_adam_step_with_one_fused_multiply_add(fused):
    g = _gen(8)
    n = 4099
    p, v = torch.randn(n, generator=g), torch.randn(n, generator=g)
    gr = R.optimiser_gradient(n, g)
    mg = gr.abs() * torch.rand(n, generator=g) + 1e-3
    # (mom1 = 0.9: with 0.5 the product mom1 * v is exact and fusing it changes nothing)
    ref = R.adam_f32(p, gr, v, mg, 3e-4, 0.9, 0.999, 0.271, 0.003)
    got = R.adam_f32(p, gr, v, mg, 3e-4, 0.9, 0.999, 0.271, 0.003, fused=fused)
    assert R.ulp_distance(got[0], ref[0]).max() <= 2                        # a last-bit defect ...
    with pytest.raises(AssertionError, match="differ in their bits"):       # ... that only a bit comparison sees
        for a, b in zip(got, ref):
            R.assert_bits_equal(a, b)


def test_bits_equal_counts_signed_zero_and_nan_payloads():
    R.assert_bits_equal(np.float32([0.0, np.nan]), np.float32([0.0, np.nan]))
    with pytest.raises(AssertionError):
        R.assert_bits_equal(np.float32([0.0]), np.float32([-0.0]))
    a = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)
    b = np.array([0x7FC00001], dtype=np.uint32).view(np.float32)
    with pytest.raises(AssertionError):
        R.assert_bits_equal(a, b)


def test_close_elementwise_reports_the_worst_element():
    ref = np.float64([1.0, 100.0, 0.0])
    assert R.assert_close_elementwise(np.float32([1.0, 100.0, 0.0]), ref, np.abs(ref), 1e-6) == 0.0
    r = R.assert_close_elementwise(np.float64([1.0 + 5e-7, 100.0, 0.0]), ref, np.abs(ref), 1e-6)
    assert 0.49 < r < 0.51
    with pytest.raises(AssertionError, match=r"at \(0,\)"):                 # a whole-tensor L2 norm would pass this
        R.assert_close_elementwise(np.float64([1.0 + 3e-6, 100.0, 0.0]), ref, np.abs(ref), 1e-6)
    with pytest.raises(AssertionError, match=r"at \(2,\)"):                 # zero scale: must be equal
        R.assert_close_elementwise(np.float64([1.0, 100.0, 1e-30]), ref, np.abs(ref), 1e-6)
    with pytest.raises(AssertionError):
        R.assert_close_elementwise(np.float64([np.nan, 100.0, 0.0]), ref, np.abs(ref), 1e-6)


# ---------------------------------------------------------------------------------------------- exactness of the integer cases
def test_integer_cases_stay_below_two_to_the_24():
    """Largest row count of tests/test_pointwise_edges_gpu.py: 16385.  Column sums of integers in [-8, 8]; the GLU form with
    dy in [-8, 8], gates 0 (s = 1/2) and even a in [-8, 8]: da = dy / 2 (multiples of 1/2, |da| <= 4) and
    dl = dy * a / 4 (multiples of 1/2, |dl| <= 16).  Every partial sum is a multiple of the unit below 2^24 units."""
    rows = 16385
    assert R.int_sum_bound(rows, 8) < 2 ** 24
    assert R.int_sum_bound(rows, 4, unit=0.5) < 2 ** 24
    assert R.int_sum_bound(rows, 16, unit=0.5) < 2 ** 24
    assert R.int_sum_bound(9 * 400, 64) < 2 ** 24                            # sums of squares of the integer weight-norm case
    g = _gen(9)
    a = R.int_valued((rows, 8), -8, 8, g)
    exact = R.colsum_exact(a)
    for order in (torch.arange(rows), torch.randperm(rows, generator=g)):   # any order, pairwise or sequential
        b = a[order].numpy()
        assert (b.sum(0, dtype=np.float32).astype(np.int64) == exact).all()
        assert (b.cumsum(0, dtype=np.float32)[-1].astype(np.int64) == exact).all()


def test_launch_geometry_matches_the_cases():
    assert R.colreduce_geometry(64, 4) == (1, 64) and R.colreduce_geometry(65, 4) == (2, 33)
    assert R.colreduce_geometry(1, 4) == (1, 1)
    assert R.colsum_chain_length(16385, 8) == 5 + 16 + 64 + 4
    # (8197, 256) contiguous: 524 608 quads, 256 blocks; every thread sweeps 8 quads, 320 threads one more
    n4, blocks, stride, last_unrolled, first_tail = R.absmax_geometry(8197, 256, 256)
    assert (n4, blocks, stride, last_unrolled, first_tail) == (524608, 256, 65536, 524287, 524288)
    assert R.absmax_geometry(1, 1028, 1028)[3:] == (None, 0)                 # too short for the unrolled sweep
    assert R.absmax_geometry(7, 36, 52)[3:] == (None, 0)                     # pitched: never unrolled
    assert R.grid_wrap_elements() == 4194304
