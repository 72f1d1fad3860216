"""The k-NN probe on the GPU: the fused fp64-MFMA top-k launch (csrc/topk.hip) against the numpy fp64 restatement
(tests/probe_ref.py), its order and masking rules, the host layer (utils/probe.py) alone and on two ranks, the hook of
train.main against the reference on the feature rows it handed to the kernel, and training with the probe against training
without it, bit for bit, eagerly and under step graphs.

Bars.  A score: probe_ref.bar = 2 (C + 8) 2^-53 |q| |y|^T.  Indices: EXACT, after the test has shown on the reference alone
that consecutive reference scores among each row's top k + 1 are at least 1000 bars apart, so a mismatch is a kernel
error and not a tie.  Ties, order, position, split and role: the same BITS.
Measured on an MI355X: smallest reference gap 1.55e5 bars (65 x 257 x 32768) ... 1.5e10; worst |err| / bar of a score 0.030
(70 x 300 x 36), 6.3e-5 (65 x 257 x 32768), 2.4e-4 (130 x 520 x 7296 and 1 x 9 x 2048), 0 (64 x 64 x 4).
"""
import functools

import numpy as np
import pytest
import torch

import probe_ref
import metric_harness as H
from metric_harness import DEV
from otgan_amd import _lib
from otgan_amd.utils import probe

pytestmark = pytest.mark.gpu
MARGIN = 1000.0
KS = (1, 3, 4, 5, 8)
# (nq, ny, C): ragged query block, ragged channel slab and two column splits with a one-block tail; the DCGAN width, one
# row and one column past a block; the DenseNet width; one exact block of the narrowest rows; a single row
SHAPES = [(70, 300, 36), (65, 257, 32768), (130, 520, 7296), (64, 64, 4), (1, 9, 2048)]


def _unit(rng, n, C):
    x = rng.standard_normal((n, C))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(nq, ny, C):
    """(q, y, reference index and score at k = 9, bar [nq, ny]) -- computed once, never written to"""
    rng = np.random.default_rng(0)
    q, y = _unit(rng, nq, C), _unit(rng, ny, C)
    idx, sc = probe_ref.topk(q, y, min(9, ny))
    return q, y, idx, sc, probe_ref.bar(q, y)


def _dev(x):
    return torch.as_tensor(x, device=DEV)


def _topk(q, y, k, self0=-1):
    i, s = probe.topk(_dev(q), _dev(y), k, self0)
    return i.cpu().numpy(), s.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


@pytest.mark.parametrize("nq,ny,C", SHAPES)
def test_against_reference(nq, ny, C):
    q, y, ridx, rsc, bar = _case(nq, ny, C)
    # precondition, on the reference alone: no near-tie among the top k + 1 of any row
    rows = np.arange(nq)[:, None]
    gap = rsc[:, :-1] - rsc[:, 1:]
    ratio = (gap / np.maximum(bar[rows, ridx[:, :-1]], bar[rows, ridx[:, 1:]])).min()
    print("smallest gap / bar", ratio)
    assert ratio >= MARGIN
    worst = 0.0
    for k in KS:
        idx, sc = _topk(q, y, k)
        assert idx.dtype == np.int32 and idx.shape == (nq, k)
        assert np.array_equal(idx, ridx[:, :k])
        err = np.abs(sc - rsc[:, :k]) / bar[rows, ridx[:, :k]]
        worst = max(worst, float(err.max()))
        assert err.max() <= 1.0
    print("worst |err| / bar", worst)


def test_short_on_columns():
    rng = np.random.default_rng(1)
    q = _unit(rng, 67, 40)
    y = np.concatenate([_unit(rng, 2, 40), -0.999 * q[:1]])        # column 2: score -0.999 with row 0, very negative
    for k in (3, 4, 8):
        idx, sc = _topk(q, y, k)
        ridx, rsc = probe_ref.topk(q, y, k)
        assert np.array_equal(idx, ridx)                            # every real column is there, the rest -1
        assert (np.sort(idx[:, :3], axis=1) == np.arange(3)).all() and (idx[:, 3:] == -1).all()
        assert np.isneginf(sc[:, 3:]).all() and np.isfinite(sc[:, :3]).all()
        assert idx[0, 2] == 2 and abs(sc[0, 2] + 0.999) < 1e-6      # the planted column, last of the three, not displaced
    idx, sc = _topk(q, y[:0], 5)
    assert (idx == -1).all() and np.isneginf(sc).all()
    idx, sc = _topk(q[:0], y, 5)
    assert idx.shape == (0, 5) and sc.shape == (0, 5)


def test_ties_go_to_the_smaller_column():
    q, y, _, _, _ = _case(70, 300, 36)
    y = y.copy()
    y[[3, 131, 290]] = q[7]                                                # blocks 0, 2, 4: both splits
    q2 = np.concatenate([q, q[7:8]])                                       # row 70 = row 7
    dots = q2.astype(np.float64) @ y.astype(np.float64).T
    dots[:, 131] = dots[:, 290] = dots[:, 3]
    for k in (3, 5):
        idx, sc = _topk(q2, y, k)
        ridx, _ = probe_ref.topk_from_dots(dots, k)
        assert idx[7, :3].tolist() == [3, 131, 290]                        # the copies of the row itself: nothing is nearer
        assert len(set(_bits(sc[7, :3]).tolist())) == 1
        for i in range(71):                                                # wherever the copies appear: ascending, same bits
            at = [int(np.nonzero(idx[i] == j)[0][0]) for j in (3, 131, 290) if j in idx[i]]
            assert at == sorted(at) and len(set(_bits(sc[i, at]).tolist())) <= 1
        assert np.array_equal(idx, ridx)
        assert np.array_equal(idx[70], idx[7]) and np.array_equal(_bits(sc[70]), _bits(sc[7]))


def test_self_exclusion_by_position():
    _, bank, _, _, _ = _case(70, 300, 36)
    bank = bank.copy()
    bank[250] = bank[140]                        # a second copy of row 140 elsewhere: a neighbour, with the score s(a, a)
    lo, hi = 130, 200
    idx, sc = _topk(bank[lo:hi], bank, 4, self0=lo)
    dots = bank[lo:hi].astype(np.float64) @ bank.astype(np.float64).T
    dots[:, 250] = dots[:, 140]
    ridx, _ = probe_ref.topk_from_dots(dots, 4, self0=lo)
    assert np.array_equal(idx, ridx)
    assert not (idx == np.arange(lo, hi)[:, None]).any()
    assert idx[10, 0] == 250
    full_i, full_s = _topk(bank[lo:hi], bank, 5)                # nothing excluded: own column first (or its copy: the smaller)
    assert full_i[10, :2].tolist() == [140, 250] and _bits(full_s[10, 0]) == _bits(full_s[10, 1]) == _bits(sc[10, 0])
    keep = full_i != np.arange(lo, hi)[:, None]
    assert np.array_equal(full_i[keep].reshape(hi - lo, 4), idx) and np.array_equal(_bits(full_s[keep]).reshape(hi - lo, 4), _bits(sc))


@pytest.mark.parametrize("nq,ny,C", [(70, 300, 36), (65, 257, 2048)])
def test_order_free(nq, ny, C):
    rng = np.random.default_rng(2)
    q, y = _unit(rng, nq, C), _unit(rng, ny, C)
    k = 5
    idx, sc = _topk(q, y, k)
    perm = rng.permutation(ny)
    pidx, psc = _topk(q, y[perm], k)
    assert np.array_equal(perm[pidx], idx) and np.array_equal(_bits(psc), _bits(sc))
    for lo, hi in ((0, 1), (nq - 3, nq), (5, 69)):                # rows of one call equal separate calls
        i2, s2 = _topk(q[lo:hi], y, k)
        assert np.array_equal(i2, idx[lo:hi]) and np.array_equal(_bits(s2), _bits(sc[lo:hi]))
    # swapped roles: s(q_i, y_j) is found with the same bits where topk(y, q) holds the mirrored pair
    # (planted mutual nearest pairs -- a column that IS a query row -- make the check independent of the random geometry;
    # every other pair that happens to be in both results is compared as well)
    k8 = 8
    planted = [(0, 5), (nq - 1, 70), (33, ny - 1), (63, 200)]       # distinct rows and columns, in every block
    y = y.copy()
    for i, j in planted:
        y[j] = q[i]
    idx8, sc8 = _topk(q, y, k8)
    tidx, tsc = _topk(y, q, k8)
    for i, j in planted:
        assert idx8[i, 0] == j and tidx[j, 0] == i and _bits(sc8[i, 0]) == _bits(tsc[j, 0])
    for i in range(nq):
        for t in range(k8):
            j = idx8[i, t]
            at = np.nonzero(tidx[j] == i)[0]
            if len(at):
                assert _bits(tsc[j, at[0]]) == _bits(sc8[i, t])


def test_slices_guards_and_overwrite():
    rng = np.random.default_rng(3)
    nq, ny, C, k = 70, 300, 36, 5
    wq, wy = rng.standard_normal((nq, C + 12)).astype(np.float32), rng.standard_normal((ny, C + 8)).astype(np.float32)
    dq, dy = _dev(wq)[:, 4:4 + C], _dev(wy)[:, 8:8 + C]
    assert dq.stride(0) == C + 12 and dq.data_ptr() % 16 == 0
    ridx, _ = probe_ref.topk(wq[:, 4:4 + C], wy[:, 8:8 + C], k)
    want_i, want_s = probe.topk(dq.contiguous(), dy.contiguous(), k)
    assert np.array_equal(want_i.cpu().numpy(), ridx)
    L = _lib.lib()
    nbytes = L.otgan_topk_dot_workspace_bytes(nq, ny, k)
    ws = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=DEV)
    guard_s = torch.full((nq + 2, k), float("nan"), dtype=torch.float64, device=DEV)
    guard_i = torch.full((nq + 2, k), -77, dtype=torch.int32, device=DEV)
    for _ in range(2):              # the second call overwrites the first: nothing accumulates
        _lib.check(L.otgan_topk_dot_f64(nq, ny, C, dq.data_ptr(), dq.stride(0), dy.data_ptr(), dy.stride(0), k, -1,
                                        guard_i[1:].data_ptr(), guard_s[1:].data_ptr(), ws.data_ptr(), nbytes,
                                        _lib.stream_ptr()), "topk")
    torch.cuda.synchronize()
    assert torch.equal(guard_i[1:-1], want_i) and torch.equal(guard_s[1:-1].view(torch.int64), want_s.view(torch.int64))
    for r in (0, -1):
        assert bool(torch.isnan(guard_s[r]).all()) and bool((guard_i[r] == -77).all())
    # a null score: the indices alone
    guard_i.fill_(-77)
    _lib.check(L.otgan_topk_dot_f64(nq, ny, C, dq.data_ptr(), dq.stride(0), dy.data_ptr(), dy.stride(0), k, -1,
                                    guard_i[1:].data_ptr(), None, ws.data_ptr(), nbytes, _lib.stream_ptr()), "topk")
    assert torch.equal(guard_i[1:-1], want_i)


def test_bad_arguments():
    L = _lib.lib()
    nq, ny, C, k = 8, 12, 8, 3
    q, y = torch.randn(nq, C, device=DEV), torch.randn(ny, C, device=DEV)
    out_i = torch.full((nq, 8), -77, dtype=torch.int32, device=DEV)
    out_s = torch.full((nq, 8), float("nan"), dtype=torch.float64, device=DEV)
    nbytes = L.otgan_topk_dot_workspace_bytes(nq, ny, 8)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=DEV)

    def call(nq=nq, ny=ny, C=C, qp=q.data_ptr(), ldq=C, yp=y.data_ptr(), ldy=C, k=k, self0=-1, ip=out_i.data_ptr(),
             wsp=ws.data_ptr(), wsb=nbytes):
        return L.otgan_topk_dot_f64(nq, ny, C, qp, ldq, yp, ldy, k, self0, ip, out_s.data_ptr(), wsp, wsb, _lib.stream_ptr())
    bad = [dict(k=0), dict(k=9), dict(self0=-2), dict(C=6), dict(C=0), dict(ldq=4), dict(ldy=6), dict(nq=-1), dict(ny=-1),
           dict(qp=q.data_ptr() + 4), dict(yp=None), dict(ip=None), dict(ip=out_i.data_ptr() + 2), dict(wsb=8), dict(wsp=None)]
    for kw in bad:
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert bool((out_i == -77).all()) and bool(torch.isnan(out_s).all())
    assert call() == 0 and call(nq=0, qp=None, ip=None) == 0
    assert L.otgan_topk_dot_workspace_bytes(nq, ny, 0) == 0 and L.otgan_topk_dot_workspace_bytes(nq, ny, 9) == 0
    # the wrapper raises on the host, before any launch
    for args in ((q, y, 0), (q, y, 9), (q, y, 3, -2), (q, y[:, :4], 3), (q.double(), y, 3), (q[0], y, 3)):
        with pytest.raises(ValueError):
            probe.topk(*args)
    with pytest.raises(_lib.OtganError):
        probe.topk(q.cpu(), y, 3)


# ---------------------------------------------------------------- accuracy
@functools.lru_cache(maxsize=None)
def _planted(n_bank=96, n_q=95, C=64):
    """ten unit class centres plus small noise, labels = the centre"""
    rng = np.random.default_rng(4)
    centres = _unit(rng, 10, C)

    def draw(n):
        lab = rng.integers(0, 10, n)
        x = centres[lab] + 0.02 * rng.standard_normal((n, C))
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), lab.astype(np.int64)
    return draw(n_bank) + draw(n_q)


def test_accuracy_on_planted_features():
    bank, bl, q, ql = _planted()
    for k in (1, 5, 8):
        got = probe.accuracy(_dev(bank), _dev(bl), _dev(q), _dev(ql), k)
        assert got == probe_ref.accuracy(bank, bl, q, ql, k)
        assert got[1] == got[2] == 95                        # 1.0 at 1-NN
    assert probe.accuracy(_dev(bank), _dev(bl), None, None, 3, leave_one_out=True) == \
        probe_ref.accuracy(bank, bl, None, None, 3, leave_one_out=True)
    wrong = (ql + 1) % 10
    assert probe.accuracy(_dev(bank), _dev(bl), _dev(q), _dev(wrong), 1)[:2] == (0, 0)


def _rank_accuracy(rank, world, path):
    from otgan_amd.utils import features
    bank, bl, q, ql = _planted()
    out = []
    for loo in (False, True):
        (b0, b1), (q0, q1) = features.share(len(bank), rank, world), features.share(len(q), rank, world)
        out.append(probe.accuracy(_dev(bank[b0:b1]), _dev(bl[b0:b1]), _dev(q[q0:q1]), _dev(ql[q0:q1]), 5, rank, world, loo))
    return out


def test_two_ranks_return_the_single_process_counts():
    bank, bl, q, ql = _planted()
    one = [probe.accuracy(_dev(bank), _dev(bl), _dev(q), _dev(ql), 5, leave_one_out=loo) for loo in (False, True)]
    assert one[0][2] == 95 and one[1][2] == 96
    for got in H.two_ranks(_rank_accuracy):
        assert [tuple(g) for g in got] == one


# ---------------------------------------------------------------- the hook in train.main
def _fake_cifar(root, n_train=48, n_test=16):
    """the CIFAR-10 python layout with labels i % 4: n_train images over data_batch_1 ... 5, n_test in test_batch"""
    import pickle
    d = root / "cifar-10-python" / "cifar-10-batches-py"
    d.mkdir(parents=True)
    rng = np.random.default_rng(7)
    cuts = np.linspace(0, n_train, 6).astype(int)
    parts = [("data_batch_%d" % (b + 1), np.arange(cuts[b], cuts[b + 1])) for b in range(5)] + [("test_batch", np.arange(n_test))]
    for name, ids in parts:
        with open(d / name, "wb") as fo:
            pickle.dump({"data": rng.integers(0, 256, (len(ids), 3072), dtype=np.uint8), "labels": [int(i % 4) for i in ids]}, fo)
    return str(root)


def _run_args(tmp_path, data, steps, extra=()):
    return ["--nr_gpu", "2", "--batch_size", "8", "--nr_sinkhorn_iter", "10", "--sinkhorn_lambda", "100", "--nr_gen_per_disc", "2",
            "--save_dir", str(tmp_path / "run"), "--seed", "3", "--max_steps", str(steps)] + list(data) + list(extra)


PROBE_LINE = "critic k-NN accuracy was"


def test_hook_against_reference(tmp_path, capsys, monkeypatch):
    from otgan_amd import train
    data = ["--data_dir", _fake_cifar(tmp_path / "data")]
    seen = []
    real_topk = probe.topk

    def recording(q, y, k, self0=-1):
        seen.append((q.cpu().numpy(), y.cpu().numpy(), k, self0))
        return real_topk(q, y, k, self0)
    monkeypatch.setattr(probe, "topk", recording)
    flags = ["--probe_every", "1", "--probe_neighbours", "3", "--probe_train_samples", "40", "--probe_test_samples", "12"]
    train.main(_run_args(tmp_path, data, 6, flags)).close()
    lines = [l for l in capsys.readouterr().out.splitlines() if PROBE_LINE in l or l.startswith("max critic")]
    assert len(seen) == 1 and len(lines) == 2              # once, after epoch 1 (the first epoch of a run is skipped)
    q, y, k, self0 = seen[0]
    assert q.shape == (12, 32768) and y.shape == (40, 32768) and (k, self0) == (3, -1)
    np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, rtol=1e-5)
    at_k, at_1, n = probe_ref.accuracy(y, np.arange(40) % 4, q, np.arange(12) % 4, 3)
    assert lines[0] == "critic k-NN accuracy was %.4f (K = 3), 1-NN was %.4f, 12 held-out against 40 training images" % (at_k / n, at_1 / n)
    assert lines[1] == "max critic k-NN accuracy was %.4f, iter was 1" % (at_k / n)
    # the device-resident path reads the same images
    seen.clear()
    train.main(_run_args(tmp_path, data, 6, flags + ["--data_on_device"])).close()
    assert lines[0] in capsys.readouterr().out and np.array_equal(seen[0][0], q) and np.array_equal(seen[0][1], y)
    # no labels: one notice, no probe, the run trains
    seen.clear()
    train.main(_run_args(tmp_path, ["--synthetic", "--synthetic_size", "48"], 6, flags)).close()
    out = capsys.readouterr().out
    assert out.count("the critic k-NN probe is skipped") == 1 and PROBE_LINE not in out and not seen
    # a bank with no more than K rows: before the first step
    with pytest.raises(ValueError, match="more than 3 rows"):
        train.main(_run_args(tmp_path, data, 6, flags[:4] + ["--probe_train_samples", "3"]))


def _trajectory(tmp_path, capsys, data, model_flags, probe_on):
    from otgan_amd import train
    extra = list(model_flags) + (["--probe_every", "1", "--probe_neighbours", "3"] if probe_on else [])
    model = train.main(_run_args(tmp_path, data, 18, extra))
    sd = model.state_dict()
    graphs = None if model.graphs is None else (model.graphs.dead, sorted(model.graphs.graphs))
    model.close()
    out = capsys.readouterr().out
    dist = [l.split("time = ")[1].split(", ", 1)[1] for l in out.splitlines() if l.startswith("Iteration")]
    return sd, dist, graphs, sum(l.startswith(PROBE_LINE) for l in out.splitlines())


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for key in a:
            _same(a[key], b[key], path + "/" + str(key))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for n, (x, y) in enumerate(zip(a, b)):
            _same(x, y, path + "/" + str(n))
    elif torch.is_tensor(a):
        assert torch.equal(a, b), path
    else:
        assert a == b, path


# 48 images, 2 x 8 per step: epochs of 3 steps, the probe runs after epochs 1 ... 5.  With --nr_gen_per_disc 2 the period is 3
# steps and every graph kind is captured and replayed after a probe; the last case has a period of 4, so the probes land on
# every phase of it
@pytest.mark.parametrize("model_flags", [("--model", "dcgan", "--step_graph", "0"), ("--model", "dcgan", "--step_graph", "1"),
                                         ("--model", "densenet"),
                                         ("--model", "dcgan", "--step_graph", "1", "--nr_gen_per_disc", "3")],
                         ids=["dcgan-eager", "dcgan-graphs", "densenet", "dcgan-graphs-period4"])
def test_training_unchanged(tmp_path, capsys, model_flags):
    data = ["--data_dir", _fake_cifar(tmp_path / "data")]
    sd0, dist0, graphs0, probes0 = _trajectory(tmp_path, capsys, data, model_flags, False)
    sd1, dist1, graphs1, probes1 = _trajectory(tmp_path, capsys, data, model_flags, True)
    assert (probes0, probes1) == (0, 5) and len(dist0) == 6
    if "0" != model_flags[-1]:
        assert graphs1 is not None and graphs1[0] is None and graphs1[1] == ["disc", "gen", "gen1"]    # all three kinds replayed
    assert dist1 == dist0
    _same(sd1, sd0)
