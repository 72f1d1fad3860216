"""The Frechet Inception Distance on the GPU: the fp64-MFMA moment kernel (csrc/moments.hip) against numpy fp64, the
device accumulator and host finalisation (utils/fid.py) against numpy moments of the same pool_3, the training hook
against the op-by-op fp64 interpreter (tests/inception_graphs.py), its truncation to `eval_samples`, two ranks against
one process, and train.main with --fid_stats end to end.

Bars.  Kernel: |got - ref|_F <= 1e-12 | |X|^T |X| |_F -- derived, not measured: the products of fp32 values are exact
in fp64 and at most n fp64 additions follow, n 2^-53 <= 4.5e-13 for n <= 4096.  Device moments against host moments
of the same features: 1e-9 relative on d^2.  The hook against the fp64 interpreter: 1e-5 relative on d^2, the bar of
the network itself (TOL_NET of tests/test_inception_gpu.py).
Measured on an MI355X: kernel 6.1e-16 (500 x 2048), 8.8e-16 (1003 x 2048 in three calls), <= 1.3e-16 on the small
cases, column sums exact; device against host moments 2.1e-13; the hook against the fp64 interpreter 5.8e-8
(d^2 = 0.589626047 against 0.589626082); 50 of 96 rows 1.5e-11; two ranks against one process 9.6e-14 (96 samples) and
9.9e-13 (95).
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import metric_harness as H
from metric_harness import DEV, EVALS, Replay as _Replay, interpreter as _interpreter, net as _net, pool3 as _pool3, sets as _sets
from otgan_amd import _lib
from otgan_amd.utils import fid
from otgan_amd.utils.inception import inception_score_from_probs

pytestmark = pytest.mark.gpu
TOL_KERNEL = 1e-12
TOL_MOMENTS = 1e-9
TOL_NET = 1e-5


# ---------------------------------------------------------------- the kernel
def _features(rng, n, C):
    """pool_3-like rows: non-negative, a different scale per channel, some dead channels."""
    x = np.abs(rng.standard_normal((n, C))) * rng.uniform(0.05, 3.0, C) + rng.uniform(0.0, 1.0, C)
    x[:, rng.integers(0, C, max(C // 16, 1))] = 0.0
    return x.astype(np.float32)


def _call(n, C, ldx, x_ptr, s, o):
    return _lib.lib().otgan_moments_update_f64(n, C, ldx, x_ptr, s.data_ptr(), o.data_ptr(), _lib.stream_ptr())


def _buffers(rng, C, fill):
    """(sum, outer) on the device and their host copies: zeros, or a random symmetric start value."""
    if not fill:
        return (torch.zeros(C, dtype=torch.float64, device=DEV), torch.zeros(C, C, dtype=torch.float64, device=DEV),
                np.zeros(C), np.zeros((C, C)))
    s0, o0 = rng.standard_normal(C), rng.standard_normal((C, C))
    o0 = o0 + o0.T
    return torch.as_tensor(s0, device=DEV), torch.as_tensor(o0, device=DEV), s0, o0


def _check_moments(tag, s, o, x, s0, o0):
    x64 = x.astype(np.float64)
    got_s, got_o = s.cpu().numpy(), o.cpu().numpy()
    ax = np.abs(x64)
    es = np.linalg.norm(got_s - (s0 + x64.sum(0))) / max(np.linalg.norm(ax.sum(0)), 1e-300)
    eo = np.linalg.norm(got_o - (o0 + x64.T @ x64)) / max(np.linalg.norm(ax.T @ ax), 1e-300)
    print("moments %s: relative error sum %.2e, outer %.2e" % (tag, es, eo))
    assert es <= TOL_KERNEL and eo <= TOL_KERNEL, (tag, es, eo)
    assert torch.equal(o, o.T), "outer is not bitwise symmetric"


@pytest.mark.parametrize("n,C,chunks,fill", [(500, 2048, (500,), False), (1003, 2048, (500, 500, 3), False),
                                             (7, 40, (7,), True), (0, 40, (0,), True), (37, 100, (33, 4), True)])
def test_moments_kernel_against_numpy_fp64(n, C, chunks, fill):
    rng = np.random.default_rng(n + C)
    x = _features(rng, n, C)
    runs = []
    for _ in range(2):
        s, o, s0, o0 = _buffers(np.random.default_rng(1), C, fill)
        xt = torch.as_tensor(x, device=DEV)
        at = 0
        for c in chunks:
            assert _call(c, C, C, xt[at:at + c].data_ptr() if c else xt.data_ptr(), s, o) == 0
            at += c
        runs.append((s, o))
    _check_moments("n=%d C=%d in %d calls" % (n, C, len(chunks)), runs[0][0], runs[0][1], x, s0, o0)
    # the same sequence of calls gives the same bits
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    if n == 0:
        assert np.array_equal(runs[0][0].cpu().numpy(), s0) and np.array_equal(runs[0][1].cpu().numpy(), o0)


def test_moments_kernel_reads_a_column_slice_of_a_wider_buffer():
    rng = np.random.default_rng(11)
    n, C, ldx, off = 45, 40, 72, 16
    wide = np.full((n, ldx), 1e30, np.float32)               # poison beside the slice
    x = _features(rng, n, C)
    wide[:, off:off + C] = x
    wt = torch.as_tensor(wide, device=DEV)
    s, o, s0, o0 = _buffers(rng, C, False)
    assert _call(n, C, ldx, wt.data_ptr() + 4 * off, s, o) == 0
    _check_moments("slice of a wider buffer", s, o, x, s0, o0)
    # the accumulator passes the row stride of a sliced tensor on
    acc = fid.MomentAccumulator(C, DEV).update(wt[:, off:off + C])
    assert acc.n == n and torch.equal(acc.outer, o) and torch.equal(acc.sum, s)


def test_moments_kernel_rejects_bad_arguments():
    x = torch.zeros(8, 48, device=DEV)
    s, o = torch.zeros(48, dtype=torch.float64, device=DEV), torch.zeros(48, 48, dtype=torch.float64, device=DEV)
    assert _call(8, 6, 6, x.data_ptr(), s, o) != 0           # C not a multiple of 4
    assert _call(8, 40, 36, x.data_ptr(), s, o) != 0         # ldx < C
    assert _call(-1, 40, 48, x.data_ptr(), s, o) != 0
    assert _lib.lib().otgan_moments_update_f64(8, 40, 48, x.data_ptr(), None, o.data_ptr(), _lib.stream_ptr()) != 0
    assert float(o.abs().sum()) == 0.0 and float(s.abs().sum()) == 0.0
    acc = fid.MomentAccumulator(48, DEV)
    with pytest.raises(_lib.OtganError):
        acc.update(torch.zeros(8, 48))                       # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        acc.update(torch.zeros(8, 40, device=DEV))


# ---------------------------------------------------------------- end to end on the narrow graph (C = 40)
def _host_stats(p3):
    p3 = np.asarray(p3, np.float64)
    return np.mean(p3, 0), np.cov(p3, rowvar=False)


def _device_stats(p3):
    acc = fid.MomentAccumulator(p3.shape[1], DEV)
    for i in range(0, p3.shape[0], 40):                      # in uneven pieces: 40 + 40 + 16
        acc.update(p3[i:i + 40])
    n, s, o = acc.all_reduce().moments()
    assert n == p3.shape[0]
    return fid.stats_from_moments(n, s, o)


def _state(real):
    return H.state(fid_real=real)


def test_device_moments_against_host_moments_of_the_same_pool3():
    net = _net()
    xa, xb = _sets()
    pa, pb = _pool3(net, xa), _pool3(net, xb)
    got = fid.frechet_distance(*_device_stats(pa), *_device_stats(pb))
    ref = fid.frechet_distance(*_host_stats(pa.cpu().numpy()), *_host_stats(pb.cpu().numpy()))
    print("device moments against host moments: d^2 %.12g / %.12g, relative difference %.2e" % (got, ref, abs(got - ref) / ref))
    assert ref > 0.1 and abs(got - ref) <= TOL_MOMENTS * ref


def test_hook_against_the_fp64_interpreter(capsys):
    from otgan_amd.train import inception_hook
    net = _net()
    xa, xb = _sets()
    mu_b, sigma_b, n_b = fid.dataset_stats(net, xb)
    assert n_b == 96
    state = _state((mu_b, sigma_b))
    m = _Replay(xa)
    out = inception_hook(m, SimpleNamespace(eval_samples=96), net, state)
    printed = capsys.readouterr().out
    (p3a, pra), (p3b, _) = _interpreter(0), _interpreter(1)
    ref = fid.frechet_distance(*_host_stats(p3a), *_host_stats(p3b))
    for key in ("fid_live", "fid_EMA"):
        e = abs(out[key] - ref) / ref
        with capsys.disabled():
            print("hook %s: d^2 %.9g, fp64 interpreter %.9g, relative error %.2e" % (key, out[key], ref, e))
        assert e <= TOL_NET, (key, out[key], ref)
    assert m.at == {False: 96, True: 96}                    # one pass over the samples per evaluated model
    # the score outputs of the same call are unchanged
    sref = inception_score_from_probs(pra, splits=10)
    for key in ("live", "EMA"):
        assert out[key][0] == pytest.approx(sref[0], rel=TOL_NET) and out[key][1] == pytest.approx(sref[1], rel=1e-3, abs=1e-6)
    assert state["fid_min"] == min(out["fid_live"], out["fid_EMA"]) and state["fid_iter"] == 3
    lines = printed.splitlines()
    assert lines[1] == "FID was %.4f" % out["fid_live"] and lines[3] == "EMA FID was %.4f" % out["fid_EMA"]
    assert lines[0].startswith("inception score was") and lines[2].startswith("EMA inception score was")
    assert lines[4].startswith("max inception score was") and lines[5] == "min FID was %.4f, iter was 3" % state["fid_min"]
    # without the statistics the hook is the one it was
    state2 = {"max": 0.0, "iter": 0, "epoch": 3}
    out2 = inception_hook(_Replay(xa), SimpleNamespace(eval_samples=96), net, state2)
    assert set(out2) == {"live", "EMA"} and out2["live"] == out["live"] and "fid_min" not in state2
    assert "FID" not in capsys.readouterr().out


def test_hook_covers_exactly_eval_samples_rows():
    from otgan_amd.train import inception_hook
    net = _net()
    xa, xb = _sets()
    real = _device_stats(_pool3(net, xb))
    out = inception_hook(_Replay(xa), SimpleNamespace(eval_samples=50), net, _state(real))
    ref = fid.frechet_distance(*_host_stats(_pool3(net, xa[:50]).cpu().numpy()), *real)
    print("50 of 96 rows: d^2 %.12g / %.12g" % (out["fid_live"], ref))
    assert abs(out["fid_live"] - ref) <= TOL_MOMENTS * ref and out["fid_EMA"] == out["fid_live"]
    full = fid.frechet_distance(*_host_stats(_pool3(net, xa).cpu().numpy()), *real)
    assert abs(full - ref) > 1e-3 * ref                      # (the other 46 rows would have shown)


def _rank_worker(rank, world, path):
    from otgan_amd.train import inception_hook
    net = _net()
    mu, sigma, _ = fid.load_stats(path + "real.npz", net.plan.pool3_channels)
    xa = _sets()[0]
    res = {}
    for ev in EVALS:
        share = -(-ev // world)
        out = inception_hook(_Replay(xa[rank * share:(rank + 1) * share]), SimpleNamespace(eval_samples=ev), net,
                             _state((mu, sigma)), rank, world)
        res[ev] = (out["fid_live"], out["fid_EMA"], out["live"][0])
    return res


def test_two_ranks_equal_one_process():
    from otgan_amd.train import inception_hook
    net = _net()
    xa, xb = _sets()
    mu, sigma, n = fid.dataset_stats(net, xb)
    got = H.two_ranks(_rank_worker, lambda path: fid.save_stats(path + "real.npz", mu, sigma, n))
    for ev in EVALS:
        one = inception_hook(_Replay(xa), SimpleNamespace(eval_samples=ev), net, _state((mu, sigma)))
        assert got[0][ev] == got[1][ev], (ev, got)           # every rank ends with the same values
        for k, key in enumerate(("fid_live", "fid_EMA")):
            e = abs(got[0][ev][k] - one[key]) / one[key]
            print("two ranks, %d samples, %s: %.12g against one process %.12g, relative difference %.2e"
                  % (ev, key, got[0][ev][k], one[key], e))
            assert e <= TOL_MOMENTS
        assert got[0][ev][2] == pytest.approx(one["live"][0], rel=1e-6)


def test_train_main_with_fid_stats(tmp_path, capsys):
    from otgan_amd import train
    stats = str(tmp_path / "real_stats.npz")
    common = H.train_args(tmp_path)
    train.main(common + ["--fid_stats", stats, "--fid_real_samples", "40"])
    out = capsys.readouterr().out
    assert "computed from 40 training images" in out and stats in out
    with np.load(stats) as f:
        assert set(f.files) == {"mu", "sigma", "n"} and int(f["n"]) == 40
        assert f["mu"].shape == (40,) and f["sigma"].shape == (40, 40) and f["sigma"].dtype == np.float64
    lines = out.splitlines()
    kinds = [k for l in lines for k in ("FID was", "EMA FID was", "min FID was") if l.startswith(k)]
    assert kinds == ["FID was", "EMA FID was", "min FID was"], out
    i = [n for n, l in enumerate(lines) if l.startswith("FID was")][0]
    assert lines[i - 1].startswith("inception score was") and float(lines[i].split()[-1]) > 0.0
    # a second run loads the file
    before = os.path.getmtime(stats)
    train.main(common + ["--fid_stats", stats])
    out = capsys.readouterr().out
    assert "loaded " + stats in out and "computed from" not in out and "min FID was" in out
    assert os.path.getmtime(stats) == before
    # without the flag: nothing of it
    train.main(common)
    out = capsys.readouterr().out
    assert "FID" not in out and "max inception score was" in out
    # with a classifier that is not the 2015 graph: said once, training goes on
    train.main(common[:-2] + ["--fid_stats", str(tmp_path / "never.npz")])
    out = capsys.readouterr().out
    assert out.count("FID needs the 2015 Inception graph") == 1 and not os.path.exists(str(tmp_path / "never.npz"))
