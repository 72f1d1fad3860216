"""The Kernel Inception Distance on the GPU: the fused fp64-MFMA kernel-sum launch (csrc/kid.hip) against the brute-force
numpy fp64 restatement (tests/kid_ref.py), the host wrapper (utils/kid.py), the training hook against the op-by-op fp64
interpreter (tests/inception_graphs.py), its truncation to `eval_samples`, two ranks against the documented rule, and
train.main with --kid_subsets end to end.

Bars.  Kernel, per output: |got - ref| <= 2 (3 C + P + 8) 2^-53 sum (|X_i| . |Y_j| / C + 1)^3 over the counted pairs --
derived, not measured (kid_ref.error_bound: exact products, at most C additions per dot product, the cube triples its
relative error, P summed terms, the factor 2 for the reference's own rounding).  The hook against the fp64 interpreter:
TOL_NET = 1e-5 (the network's own bar, tests/test_inception_gpu.py) times the kernel scale
s0 / (m (m - 1)) + s1 / (m (m - 1)) + 2 s2 / m^2 -- an absolute bar, MMD^2 being a difference.  Device features against the
same device features through numpy: 1e-9 times the scale.  The standard deviation of a vector moves by at most the largest
change of an entry, so it is held to the largest subset's bar.
Measured on an MI355X, error / bar: kernel 2.7e-6 (2 x 1000 x 2048), 2.6e-4 (3 x 70 x 40), 4.6e-4 (33 x 100), 1.9e-3 ... 6.3e-3
(m = 7, 16, 17), 0 at the minimum shape, signed rows 4.3e-6, large diagonal 1.3e-5, repeated row numbers 0.028, slices
2.9e-3; the hook against the fp64 interpreter 8.5e-5 on the worst subset and 3.4e-5 on the mean (KID 0.060870, bar
5.4e-5); 50 of 96 rows 1.0e-8 of the device bar; two ranks 1.0e-8 (96 samples) and 3.1e-8 (95).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import kid_ref
import metric_harness as H
from metric_harness import (DEV, EVALS, SEED, Replay as _Replay, interpreter as _interpreter, kinds as _kinds, net as _net,
                            pool3 as _pool3, sets as _sets, train_args as _common)
from otgan_amd import _lib
from otgan_amd.utils import kid
from otgan_amd.utils.inception import inception_score_from_probs

pytestmark = pytest.mark.gpu
TOL_NET = 1e-5
TOL_DEVICE = 1e-9


# ---------------------------------------------------------------- the kernel
def _features(rng, n, C):
    """pool_3-like rows: non-negative, a different scale per channel, some dead channels."""
    x = np.abs(rng.standard_normal((n, C))) * rng.uniform(0.05, 3.0, C) + rng.uniform(0.0, 1.0, C)
    x[:, rng.integers(0, C, max(C // 16, 1))] = 0.0
    return x.astype(np.float32)


def _tables(rng, nsub, m, nx, ny):
    xi = np.stack([rng.choice(nx, m, replace=False) for _ in range(nsub)]).astype(np.int32)
    yi = np.stack([rng.choice(ny, m, replace=False) for _ in range(nsub)]).astype(np.int32)
    return xi, yi


def _dev(a):
    return torch.as_tensor(a, device=DEV)


def _call(nsub, m, C, x_ptr, ldx, xi, y_ptr, ldy, yi, out, ws=None):
    """The C entry point as it is, with a workspace of the queried size unless one is given."""
    L = _lib.lib()
    if ws is None:
        ws = torch.empty(max(L.otgan_kid_workspace_bytes(max(nsub, 0), max(m, 2)) // 8, 1), dtype=torch.float64, device=DEV)
    return L.otgan_kid_sums_f64(nsub, m, C, x_ptr, ldx, xi.data_ptr(), y_ptr, ldy, yi.data_ptr(),
                                out.data_ptr() if out is not None else None, ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr())


def _check(tag, got, x, xi, y, yi):
    """Every subset and output against the reference within the derived bar; returns the largest error / bar."""
    got = got.cpu().numpy()
    worst = 0.0
    for s in range(xi.shape[0]):
        X, Y = x[xi[s]], y[yi[s]]
        ref, bar = kid_ref.kernel_sums(X, Y), kid_ref.error_bound(X, Y)
        ratio = np.abs(got[s] - ref) / bar
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (tag, s, got[s], ref, bar)
    print("kid_sums %s: largest error / bar %.3g" % (tag, worst))
    return worst


SHAPES = [(1, 2, 4), (3, 7, 40), (2, 16, 40), (2, 17, 40), (2, 33, 100), (3, 70, 40), (2, 1000, 2048)]


@pytest.mark.parametrize("nsub,m,C", SHAPES)
def test_kernel_against_numpy_fp64(nsub, m, C):
    rng = np.random.default_rng(nsub + 10 * m + C)
    nx, ny = m + 5, m + 9                                    # more rows than a subset takes, different on the two sides
    x, y = _features(rng, nx, C), _features(rng, ny, C) * 0.8
    xi, yi = _tables(rng, nsub, m, nx, ny)
    got = kid.kid_sums(_dev(x), xi, _dev(y), yi)
    assert got.shape == (nsub, 3) and got.dtype == torch.float64 and got.is_cuda
    _check("pool_3-like nsub=%d m=%d C=%d" % (nsub, m, C), got, x, xi, y, yi)
    assert torch.equal(got, kid.kid_sums(_dev(x), xi, _dev(y), yi))          # the same call gives the same bits


@pytest.mark.parametrize("nsub,m,C", [(3, 70, 40), (2, 33, 100)])
def test_kernel_with_signed_rows(nsub, m, C):
    """g / C + 1 takes both signs: the cube must keep the sign."""
    rng = np.random.default_rng(m)
    x = (rng.standard_normal((m + 3, C)) * 4.0).astype(np.float32)
    y = (rng.standard_normal((m + 3, C)) * 4.0).astype(np.float32)
    xi, yi = _tables(rng, nsub, m, m + 3, m + 3)
    g = x[xi[0]].astype(np.float64) @ y[yi[0]].astype(np.float64).T / C + 1.0
    assert (g < -0.5).any() and (g > 0.5).any()
    _check("signed nsub=%d m=%d C=%d" % (nsub, m, C), kid.kid_sums(_dev(x), xi, _dev(y), yi), x, xi, y, yi)


@pytest.mark.parametrize("m", [20, 70])
def test_diagonal_is_excluded(m):
    """Rows of large norm that are nearly orthogonal: sum_i k(X_i, X_i) dwarfs the off-diagonal sum, so a kernel that
    kept the diagonal (or masked the wrong elements of a diagonal block) is far off."""
    rng = np.random.default_rng(m)
    C = 40
    x = (rng.standard_normal((m, C)) * 10.0).astype(np.float32)
    y = (rng.standard_normal((m, C)) * 10.0).astype(np.float32)
    xi = yi = np.arange(m, dtype=np.int32)[None]
    ref, with_diag, bar = kid_ref.kernel_sums(x, y), kid_ref.kernel_sums(x, y, with_diagonal=True), kid_ref.error_bound(x, y)
    assert (with_diag[:2] - ref[:2] > np.abs(ref[:2])).all()                 # the diagonal alone exceeds the rest
    got = kid.kid_sums(_dev(x), xi, _dev(y), yi)
    _check("large diagonal m=%d" % m, got, x, xi, y, yi)
    g = got.cpu().numpy()[0]
    assert (np.abs(g[:2] - with_diag[:2]) > 1e6 * bar[:2]).all()
    assert abs(g[2] - with_diag[2]) <= bar[2]                                # the cross sum has no excluded diagonal


def test_diagonal_is_by_position_not_by_row_number():
    rng = np.random.default_rng(4)
    x, y = _features(rng, 12, 40), _features(rng, 12, 40)
    xi = np.array([[3, 5, 3, 7, 3, 0, 11, 5, 1]], np.int32)                 # row 3 three times, row 5 twice
    yi = np.array([[2, 2, 2, 2, 2, 2, 2, 2, 2]], np.int32)                  # one row nine times
    got = kid.kid_sums(_dev(x), xi, _dev(y), yi)
    _check("repeated row numbers", got, x, xi, y, yi)                        # (the reference gathers: repeats are rows)
    # k(Y_2, Y_2) counted for the 72 pairs of different positions
    kyy = (float(np.dot(y[2].astype(np.float64), y[2].astype(np.float64))) / 40 + 1.0) ** 3
    assert float(got[0, 1]) == pytest.approx(72 * kyy, rel=1e-13)


def test_subsets_in_one_call_equal_separate_calls_bit_for_bit():
    rng = np.random.default_rng(6)
    x, y = _features(rng, 90, 40), _features(rng, 80, 40)
    xi, yi = _tables(rng, 5, 70, 90, 80)
    xt, yt = _dev(x), _dev(y)
    together = kid.kid_sums(xt, xi, yt, yi)
    for s in range(5):
        assert torch.equal(together[s:s + 1], kid.kid_sums(xt, xi[s:s + 1], yt, yi[s:s + 1])), s
    assert not torch.equal(together[0], together[1])
    assert torch.equal(together, kid.kid_sums(xt, xi, yt, yi))


def test_out_is_overwritten():
    rng = np.random.default_rng(7)
    m, C = 33, 40
    x, y = _features(rng, m, C), _features(rng, m, C)
    xi, yi = _tables(rng, 2, m, m, m)
    out = torch.full((2, 3), 1e300, dtype=torch.float64, device=DEV)
    xt, yt = _dev(x), _dev(y)
    assert _call(2, m, C, xt.data_ptr(), C, _dev(xi), yt.data_ptr(), C, _dev(yi), out) == 0
    _check("prefilled out", out, x, xi, y, yi)
    assert torch.equal(out, kid.kid_sums(xt, xi, yt, yi))


def test_reads_column_slices_of_wider_buffers():
    rng = np.random.default_rng(11)
    m, C = 21, 40
    nx, ldx, offx, ny, ldy, offy = 45, 72, 16, 30, 100, 8                   # different strides and row counts per side
    x, y = _features(rng, nx, C), _features(rng, ny, C)
    widex, widey = np.full((nx, ldx), 1e30, np.float32), np.full((ny, ldy), 1e30, np.float32)     # poison beside the slices
    widex[:, offx:offx + C], widey[:, offy:offy + C] = x, y
    wx, wy = _dev(widex), _dev(widey)
    xi, yi = _tables(rng, 3, m, nx, ny)
    out = torch.zeros(3, 3, dtype=torch.float64, device=DEV)
    assert _call(3, m, C, wx.data_ptr() + 4 * offx, ldx, _dev(xi), wy.data_ptr() + 4 * offy, ldy, _dev(yi), out) == 0
    _check("slices of wider buffers (C call)", out, x, xi, y, yi)
    # the wrapper passes the row strides of sliced tensors on: the same launch, the same bits
    assert torch.equal(kid.kid_sums(wx[:, offx:offx + C], xi, wy[:, offy:offy + C], yi), out)
    # a slice the kernel cannot read in 16-byte pieces is copied, not refused
    got = kid.kid_sums(wx[:, offx:offx + C], xi, _dev(np.pad(widey, ((0, 0), (1, 3))))[:, offy + 1:offy + 1 + C], yi)
    _check("a misaligned slice", got, x, xi, y, yi)


def test_bad_arguments_leave_out_untouched():
    x = torch.ones(8, 48, device=DEV)
    idx = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    out = torch.full((2, 3), 7.0, dtype=torch.float64, device=DEV)
    p = x.data_ptr()
    assert _call(2, 1, 40, p, 48, idx, p, 48, idx, out) != 0                # m = 1
    assert _call(2, 4, 6, p, 48, idx, p, 48, idx, out) != 0                 # C not a multiple of 4
    assert _call(2, 4, 40, p, 36, idx, p, 48, idx, out) != 0                # ldx < C
    assert _call(2, 4, 40, p, 48, idx, p, 36, idx, out) != 0                # ldy < C
    assert _call(-1, 4, 40, p, 48, idx, p, 48, idx, out) != 0
    assert _call(2, 4, 40, p, 48, idx, p, 48, idx, None) != 0               # null out
    assert _call(2, 4, 40, p + 4, 48, idx, p, 48, idx, out) != 0            # rows not 16-byte aligned
    small = torch.empty(1, dtype=torch.float64, device=DEV)
    assert _call(2, 4, 40, p, 48, idx, p, 48, idx, out, ws=small) != 0      # a workspace below the queried size
    assert _call(0, 4, 40, p, 48, idx, p, 48, idx, out) == 0                # nothing to do: OTGAN_OK, nothing launched
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((2, 3), 7.0, dtype=torch.float64, device=DEV))
    L = _lib.lib()
    assert L.otgan_kid_workspace_bytes(100, 1000) == 100 * (16 * 17 + 16 * 16) * 8
    assert L.otgan_kid_workspace_bytes(0, 1000) == 0 and L.otgan_kid_workspace_bytes(3, 64) == 3 * 3 * 8


def test_wrapper_rejects_bad_inputs_on_the_host():
    x = torch.ones(8, 40, device=DEV)
    ok = np.zeros((2, 4), np.int32) + np.arange(4, dtype=np.int32)
    with pytest.raises(_lib.OtganError):
        kid.kid_sums(x.cpu(), ok, x, ok)                                     # a CPU tensor: no fallback
    bad = ok.copy()
    bad[1, 2] = 8
    with pytest.raises((IndexError, ValueError)):
        kid.kid_sums(x, bad, x, ok)                                          # row 8 of 8
    with pytest.raises((IndexError, ValueError)):
        kid.kid_sums(x, ok, x[:3], ok)                                       # row 3 of 3 on the other side
    bad[1, 2] = -1
    with pytest.raises((IndexError, ValueError)):
        kid.kid_sums(x, ok, x, bad)
    with pytest.raises(ValueError):
        kid.kid_sums(x.double(), ok, x, ok)                                  # wrong feature dtype
    with pytest.raises(ValueError):
        kid.kid_sums(x, ok.astype(np.int64), x, ok)                          # wrong index dtype
    with pytest.raises(ValueError):
        kid.kid_sums(x, ok[:, :1], x, ok[:, :1])                             # m = 1
    with pytest.raises(ValueError):
        kid.kid_sums(x, ok, x, ok[:1])                                       # tables of different shapes
    assert kid.kid_sums(x, ok[:0], x, ok[:0]).shape == (0, 3)


def test_feature_bank():
    bank = kid.FeatureBank(10, 8, DEV)
    a = torch.rand(6, 8, device=DEV)
    bank.append(a[:4]).append(a[4:])
    assert bank.n == 6 and torch.equal(bank.rows, a) and bank.rows.is_cuda
    with pytest.raises(ValueError):
        bank.append(torch.rand(5, 8, device=DEV))                            # does not fit
    with pytest.raises(ValueError):
        bank.append(torch.rand(1, 12, device=DEV))
    with pytest.raises(_lib.OtganError):
        bank.append(torch.rand(1, 8))
    assert bank.clear().n == 0 and bank.rows.shape == (0, 8)


# ---------------------------------------------------------------- end to end on the narrow graph (C = 40)
def _args(eval_samples, subsets=8, size=32):
    return SimpleNamespace(eval_samples=eval_samples, kid_subsets=subsets, kid_subset_size=size, seed=SEED)


def _state(real):
    return H.state(kid_real=real)


def test_hook_against_the_fp64_interpreter(capsys):
    from otgan_amd.train import inception_hook
    net = _net()
    xa, xb = _sets()
    real = kid.real_bank(net, xb, 96)
    assert real.n == 96 and real.total == 96 and real.rows.is_cuda
    state = _state(real)
    m = _Replay(xa)
    out = inception_hook(m, _args(96), net, state)
    printed = capsys.readouterr().out
    (p3a, pra), (p3b, _) = _interpreter(0), _interpreter(1)
    xi, yi = kid.subset_indices(96, 32, 8, SEED, 0), kid.subset_indices(96, 32, 8, SEED, 1)
    ref, scale = kid_ref.kid_values(p3a, xi, p3b, yi)
    full = kid_ref.kernel_sums(p3a, p3b)
    bar = TOL_NET * scale
    got = kid.kid_values(state["kid_gen"], real, 8, 32, SEED)               # the bank holds the rows of the last model
    with capsys.disabled():
        print("hook: full-96 MMD^2 %.5f (scale %.3f); subsets mean %.6f std %.6f in [%.4f, %.4f]; device mean %.6f std %.6f; "
              "largest subset error / bar %.3g, mean error / bar %.3g"
              % (kid_ref.mmd2(full, 96), kid_ref.scale(full, 96), ref.mean(), ref.std(), ref.min(), ref.max(),
                 out["kid_live"][0], out["kid_live"][1], float((np.abs(got - ref) / bar).max()),
                 abs(out["kid_live"][0] - ref.mean()) / bar.mean()))
    assert ref.mean() > 100.0 * bar.mean()                                   # (the bar is far below the value: not vacuous)
    assert (np.abs(got - ref) <= bar).all(), (got, ref, bar)
    for key in ("kid_live", "kid_EMA"):
        assert abs(out[key][0] - ref.mean()) <= bar.mean(), (key, out[key], ref.mean())
        assert abs(out[key][1] - ref.std()) <= bar.max(), (key, out[key], ref.std())
    assert out["kid_live"] == (float(np.mean(got)), float(np.std(got))) and out["kid_EMA"] == out["kid_live"]
    assert m.at == {False: 96, True: 96}                                    # one pass over the samples per evaluated model
    assert state["kid_min"] == out["kid_live"][0] and state["kid_iter"] == 3 and state["kid_m"] == 32
    # the score outputs of the same call are unchanged
    sref = inception_score_from_probs(pra, splits=10)
    for key in ("live", "EMA"):
        assert out[key][0] == pytest.approx(sref[0], rel=TOL_NET) and out[key][1] == pytest.approx(sref[1], rel=1e-3, abs=1e-6)
    lines = printed.splitlines()
    assert len(lines) == 6
    assert lines[0].startswith("inception score was") and lines[1] == "KID was %.6f, std was %.6f" % out["kid_live"]
    assert lines[2].startswith("EMA inception score was") and lines[3] == "EMA KID was %.6f, std was %.6f" % out["kid_EMA"]
    assert lines[4].startswith("max inception score was") and lines[5] == "min KID was %.6f, iter was 3" % state["kid_min"]
    # with --kid_subsets 0 the hook is the one it was: same dict, state and prints as without any of it
    state0, state1 = _state(real), {"max": 0.0, "iter": 0, "epoch": 3}
    out0 = inception_hook(_Replay(xa), _args(96, subsets=0), net, state0)
    printed0 = capsys.readouterr().out
    out1 = inception_hook(_Replay(xa), SimpleNamespace(eval_samples=96), net, state1)
    printed1 = capsys.readouterr().out
    assert set(out0) == {"live", "EMA"} and out0 == out1 and out0["live"] == out["live"]
    assert printed0 == printed1 and "KID" not in printed0
    del state0["kid_real"]
    assert state0 == state1


def test_hook_covers_exactly_eval_samples_rows():
    from otgan_amd.train import inception_hook
    net = _net()
    xa, xb = _sets()
    real = kid.real_bank(net, xb, 96)
    out = inception_hook(_Replay(xa), _args(50), net, _state(real))
    pa, pb = _pool3(net, xa).cpu().numpy(), real.rows.cpu().numpy()
    yi = kid.subset_indices(96, 32, 8, SEED, 1)
    ref, scale = kid_ref.kid_values(pa[:50], kid.subset_indices(50, 32, 8, SEED, 0), pb, yi)
    print("50 of 96 rows: KID %.9f against %.9f, error / bar %.3g"
          % (out["kid_live"][0], ref.mean(), abs(out["kid_live"][0] - ref.mean()) / (TOL_DEVICE * scale.mean())))
    assert abs(out["kid_live"][0] - ref.mean()) <= TOL_DEVICE * scale.mean() and out["kid_EMA"] == out["kid_live"]
    assert abs(out["kid_live"][1] - ref.std()) <= TOL_DEVICE * scale.max()
    full, _ = kid_ref.kid_values(pa, kid.subset_indices(96, 32, 8, SEED, 0), pb, yi)
    assert abs(full.mean() - ref.mean()) > 1e4 * TOL_DEVICE * scale.mean()  # (the other 46 rows would have shown)


def _rank_worker(rank, world, path):
    from otgan_amd.train import inception_hook
    net = _net()
    xa, xb = _sets()
    real = kid.real_bank(net, xb, 96, rank, world)
    assert real.n == 48 and real.total == 96
    res = {}
    for ev in EVALS:
        share = -(-ev // world)
        out = inception_hook(_Replay(xa[rank * share:(rank + 1) * share]), _args(ev), net, _state(real), rank, world)
        res[ev] = (out["kid_live"], out["kid_EMA"], out["live"][0])
    return res


def test_two_ranks_follow_the_documented_rule():
    """Subset b comes from rank b % 2's own rows of both banks; both ranks end with the same (mean, std)."""
    net = _net()
    xa, xb = _sets()
    got = H.two_ranks(_rank_worker)
    pa, pb = _pool3(net, xa).cpu().numpy(), _pool3(net, xb).cpu().numpy()
    for ev in EVALS:
        assert got[0][ev] == got[1][ev], (ev, got)           # every rank ends with the same values
        share = -(-ev // 2)
        ref, scale = np.zeros(8), np.zeros(8)
        for r in range(2):
            mine = min(max(ev - r * share, 0), share)
            gen, real = pa[r * share:r * share + mine], pb[r * 48:(r + 1) * 48]
            v, s = kid_ref.kid_values(gen, kid.subset_indices(mine, 32, 8, SEED, 0, r, 2),
                                      real, kid.subset_indices(48, 32, 8, SEED, 1, r, 2))
            ref[r::2], scale[r::2] = v, s
        for k, key in enumerate(("kid_live", "kid_EMA")):
            mean, std = got[0][ev][k]
            print("two ranks, %d samples, %s: (%.9f, %.9f) against (%.9f, %.9f), error / bar %.3g"
                  % (ev, key, mean, std, ref.mean(), ref.std(), abs(mean - ref.mean()) / (TOL_DEVICE * scale.mean())))
            assert abs(mean - ref.mean()) <= TOL_DEVICE * scale.mean()
            assert abs(std - ref.std()) <= TOL_DEVICE * scale.max()


def test_train_main_with_kid(tmp_path, capsys):
    from otgan_amd import train
    common = _common(tmp_path)
    train.main(common + ["--kid_subsets", "4", "--kid_subset_size", "8"])
    out = capsys.readouterr().out
    assert "KID features of the real data: pool_3 of the first 20 training images" in out and "KID subsets hold" not in out
    lines = out.splitlines()
    assert _kinds(lines, ("KID was", "EMA KID was", "min KID was")) == ["KID was", "EMA KID was", "min KID was"], out
    i, j = lines.index([l for l in lines if l.startswith("KID was")][0]), lines.index([l for l in lines if l.startswith("EMA KID was")][0])
    assert lines[i - 1].startswith("inception score was") and lines[j - 1].startswith("EMA inception score was")
    k = [n for n, l in enumerate(lines) if l.startswith("min KID was")][0]
    assert lines[k - 1].startswith("max inception score was") and "FID" not in out
    mean, std = float(lines[i].split()[2].rstrip(",")), float(lines[i].split()[-1])
    assert np.isfinite(mean) and std >= 0.0
    # with --fid_stats as well: each KID line follows its FID line
    train.main(common + ["--kid_subsets", "4", "--kid_subset_size", "8", "--fid_stats", str(tmp_path / "real_stats.npz"),
                         "--fid_real_samples", "40"])
    lines = capsys.readouterr().out.splitlines()
    names = ("inception score was", "FID was", "KID was", "EMA inception score was", "EMA FID was", "EMA KID was",
             "max inception score was", "min FID was", "min KID was")
    assert _kinds(lines, names) == list(names), lines
    first = [n for n, l in enumerate(lines) if l.startswith("inception score was")][0]
    assert [l.split(" was")[0] for l in lines[first:first + 9]] == [n[:-4] for n in names]     # consecutive lines
    # without the flag: nothing of it
    train.main(common)
    out = capsys.readouterr().out
    assert "KID" not in out and "max inception score was" in out


def test_train_main_kid_notices(tmp_path, capsys):
    from otgan_amd import train
    common = _common(tmp_path)
    # with a classifier that is not the 2015 graph: said once, training goes on
    train.main(common[:-2] + ["--kid_subsets", "4", "--kid_subset_size", "8"])
    out = capsys.readouterr().out
    assert out.count("KID needs the 2015 Inception graph") == 1 and "KID was" not in out and "Iteration 1" in out
    # a subset size beyond the 20 samples: shrunk, said once
    train.main(common + ["--kid_subsets", "4", "--kid_subset_size", "1000"])
    out = capsys.readouterr().out
    assert out.count("KID subsets hold 20 rows, not --kid_subset_size 1000") == 1
    assert "min KID was" in out
    # and one that leaves fewer than 2 rows is an error before the first step
    with pytest.raises(ValueError, match="at least 2 rows"):
        train.main(common + ["--kid_subsets", "4", "--kid_subset_size", "1"])
    assert "starting training" in capsys.readouterr().out
