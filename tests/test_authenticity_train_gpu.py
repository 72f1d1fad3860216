"""GPU: --authenticity_samples in train.main: the lines it prints against authenticity_ref.py on the same samples, the held-out
baseline and its absence, the training run unmoved by the hook (eager and replayed DCGAN, DenseNet), two ranks against one."""
import contextlib
import io
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch

import authenticity_ref as R
import metric_harness as H

pytestmark = pytest.mark.gpu

FLAGS = ["--authenticity_samples", "12", "--authenticity_neighbours", "3", "--authenticity_train_samples", "40"]
LINE, LOW = "authenticity was", "min authenticity was"
FORM = ('%sauthenticity was %.4f%s, median nearest distance was %.2f%s, exact copies %d, %d generated against %d training images')


def _fake_cifar(root, n_train=48, n_test=16):
    """the CIFAR-10 python layout: n_train random images over data_batch_1 ... 5, n_test in test_batch"""
    d = os.path.join(str(root), "cifar-10-python", "cifar-10-batches-py")
    os.makedirs(d)
    rng = np.random.default_rng(7)
    cuts = np.linspace(0, n_train, 6).astype(int)
    parts = [("data_batch_%d" % (b + 1), cuts[b + 1] - cuts[b]) for b in range(5)] + [("test_batch", n_test)]
    for name, n in parts:
        with open(os.path.join(d, name), "wb") as fo:
            pickle.dump({"data": rng.integers(0, 256, (int(n), 3072), dtype=np.uint8), "labels": [0] * int(n)}, fo)
    return str(root)


def _run_args(tmp_path, data, steps, extra=()):
    return ["--nr_gpu", "2", "--batch_size", "8", "--nr_sinkhorn_iter", "10", "--sinkhorn_lambda", "100", "--nr_gen_per_disc", "2",
            "--save_dir", str(tmp_path / "run"), "--seed", "3", "--eval_every", "1", "--max_steps", str(steps)] + list(data) + list(extra)


def _rms(d, D=3072):
    return float(np.sqrt(float(d) / D))


def _want(tag, samples, bank, radii, held=None):
    index, dist = R.nearest(samples, bank, 1)
    a, c, med = R.score(index[:, 0], dist[:, 0], radii)
    return (FORM % (tag, a / len(samples), ' (held-out %.4f)' % held[0] if held else '', _rms(med),
                    ' (held-out %.2f)' % held[1] if held else '', c, len(samples), len(bank)), a / len(samples))


def _lines(out):
    return [l for l in out.splitlines() if l.startswith(LINE) or l.startswith("EMA " + LINE) or l.startswith(LOW)]


def test_train_main_prints_the_score(tmp_path, capsys, monkeypatch):
    """6 steps = two epochs of three: the hook runs once, after epoch 1, without an --inception_model."""
    from otgan_amd import train
    from otgan_amd.utils import data as udata, swd
    root = _fake_cifar(tmp_path / "data")
    seen = []
    real_sample = swd.sample_images

    def recording(*a, **kw):
        seen.append(real_sample(*a, **kw))
        return seen[-1]
    monkeypatch.setattr(swd, "sample_images", recording)
    train.main(_run_args(tmp_path, ["--data_dir", root], 6, FLAGS)).close()
    out = capsys.readouterr().out
    lines = _lines(out)
    assert len(seen) == 2 and len(lines) == 3, out
    bank = udata.load_u8("cifar10", root)[:40]
    held = udata.load_u8("cifar10", root, "test")[:12]
    radii = R.radii(bank)
    assert "authenticity: 12 generated against 40 training images, %d of which have an exact duplicate among them" \
        % int((radii == 0).sum()) in out
    hi, hd = R.nearest(held, bank, 1)
    ha, hc, hmed = R.score(hi[:, 0], hd[:, 0], radii)
    assert out.count("held-out authenticity was %.4f, median nearest distance was %.2f, exact copies %d, 12 held-out against 40 "
                     "training images" % (ha / 12, _rms(hmed), hc)) == 1
    best = float("inf")
    for tag, images, line in (("", seen[0], lines[0]), ("EMA ", seen[1], lines[1])):
        assert images.dtype == torch.uint8 and tuple(images.shape) == (12, 32, 32, 3)
        want, a = _want(tag, images.cpu().numpy(), bank, radii, held=(ha / 12, _rms(hmed)))
        assert line == want
        best = min(best, a)
    assert lines[2] == "min authenticity was %.4f, iter was 1" % best
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        for name, images in (("nn_sample1.png", seen[0]), ("ema_nn_sample1.png", seen[1])):
            index, dist = R.nearest(images.cpu().numpy(), bank, 3)
            sheet = np.asarray(Image.open(str(tmp_path / "run" / name)))
            assert np.array_equal(sheet, R.sheet(images.cpu().numpy(), bank, index, dist, rows=10))
    # the device-resident path searches the same bank and prints the same held-out line
    seen.clear()
    train.main(_run_args(tmp_path, ["--data_dir", root], 6, FLAGS + ["--data_on_device"])).close()
    again = capsys.readouterr().out
    assert "held-out authenticity was %.4f" % (ha / 12) in again and len(_lines(again)) == 3
    for tag, images, line in (("", seen[0], _lines(again)[0]), ("EMA ", seen[1], _lines(again)[1])):
        assert line == _want(tag, images.cpu().numpy(), bank, radii, held=(ha / 12, _rms(hmed)))[0]
    # a bank of one image: before the first step
    with pytest.raises(ValueError, match="at least 2 training images"):
        train.main(_run_args(tmp_path, ["--data_dir", root], 6, FLAGS[:4] + ["--authenticity_train_samples", "1"]))
    with pytest.raises(ValueError, match="--authenticity_neighbours"):
        train.main(_run_args(tmp_path, ["--data_dir", root], 6, FLAGS[:2] + ["--authenticity_neighbours", "9"]))


def test_synthetic_data_has_no_held_out_clause(tmp_path, capsys, monkeypatch):
    from otgan_amd import train
    from otgan_amd.utils import swd
    seen = []
    real_sample = swd.sample_images

    def recording(*a, **kw):
        seen.append(real_sample(*a, **kw))
        return seen[-1]
    monkeypatch.setattr(swd, "sample_images", recording)
    train.main(_run_args(tmp_path, ["--synthetic", "--synthetic_size", "48", "--data_on_device"], 6, FLAGS)).close()
    out = capsys.readouterr().out
    lines = _lines(out)
    assert len(lines) == 3 and "held-out" not in "".join(lines) and out.count("has no held-out subset") == 1
    np.random.seed(3)                                              # the set train.main draws for --seed 3
    bank = np.random.randint(0, 256, (48, 32, 32, 3), dtype=np.uint8)[:40]
    radii = R.radii(bank)
    assert lines[0] == _want("", seen[0].cpu().numpy(), bank, radii)[0]
    assert lines[1] == _want("EMA ", seen[1].cpu().numpy(), bank, radii)[0]


def test_without_the_flag_nothing_is_said(tmp_path, capsys):
    from otgan_amd import train
    train.main(_run_args(tmp_path, ["--synthetic", "--synthetic_size", "48"], 6)).close()
    out = "\n".join(l for l in capsys.readouterr().out.splitlines() if not l.startswith("Namespace("))     # the flags' names
    assert "authenticity" not in out and "nearest distance" not in out and "Iteration 1" in out
    assert not [f for f in os.listdir(str(tmp_path / "run")) if "nn_sample" in f]


def _flat(prefix, v, out):
    if torch.is_tensor(v):
        out[prefix] = v.detach().cpu()
    elif isinstance(v, dict):
        for k in v:
            _flat("%s/%s" % (prefix, k), v[k], out)
    elif isinstance(v, (list, tuple)):
        for i, w in enumerate(v):
            _flat("%s/%d" % (prefix, i), w, out)
    else:
        out[prefix] = v
    return out


# 48 images, 2 x 8 per step: epochs of 3 steps, 12 steps = 4 epochs, the hook runs after epochs 1, 2 and 3 and training goes on
@pytest.mark.parametrize("model_flags", [("--model", "dcgan", "--step_graph", "0"), ("--model", "dcgan", "--step_graph", "1"),
                                         ("--model", "densenet")], ids=["dcgan-eager", "dcgan-graphs", "densenet"])
def test_the_hook_does_not_move_the_run(tmp_path, capsys, model_flags):
    """Parameters, optimiser moments and EMA shadows are the bits of the run without the flag."""
    from otgan_amd import train
    data = ["--data_dir", _fake_cifar(tmp_path / "data")]
    states = []
    for flags in ([], FLAGS):
        m = train.main(_run_args(tmp_path, data, 12, list(model_flags) + flags))
        assert m.step_counter == 12
        if model_flags[-1] != "0":
            assert m.graphs is not None and m.graphs.dead is None and len(m.graphs.graphs) > 0       # the steps were replayed
        states.append(_flat("", m.state_dict(full=True), {}))
        m.close()
        assert capsys.readouterr().out.count(LOW) == (3 if flags else 0)
    a, b = states
    assert a.keys() == b.keys() and sum(torch.is_tensor(v) for v in a.values()) > 20
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _hook_run(rank, world, root):
    """State and hook on a freshly initialised model (every process builds the same one from the seeds below) against the fake
    CIFAR under `root`; SAMPLE_BATCH is lowered so that both ranks draw batches of the 20 samples."""
    from otgan_amd import train
    from otgan_amd.trainer import OTGAN, default_args
    from otgan_amd.utils import swd
    dev = torch.device("cuda:0")
    np.random.seed(3)
    torch.manual_seed(3)
    args = default_args(model="dcgan", batch_size=4, nr_gpu=2, nr_sinkhorn_iter=10, seed=3, data_dir=root, save_dir=root,
                        authenticity_samples=20, authenticity_neighbours=2, authenticity_train_samples=45)
    m = OTGAN(args, dev)
    trainx = train.load_cifar(root)
    buf = io.StringIO()
    batch, swd.SAMPLE_BATCH = swd.SAMPLE_BATCH, 8
    try:
        with contextlib.redirect_stdout(buf):
            state = train.authenticity_state(args, trainx, dev, rank, world)
            state["epoch"] = 7
            res = train.authenticity_hook(m, args, state, rank, world)
    finally:
        swd.SAMPLE_BATCH = batch
        m.close()
    res = {k: {n: (v.cpu() if torch.is_tensor(v) else v) for n, v in r.items()} for k, r in res.items()}
    held = {n: (v.cpu() if torch.is_tensor(v) else v) for n, v in state["held"].items()}
    return buf.getvalue(), res, held, state["radii"].cpu()


def _rank_hook(rank, world, path):
    return _hook_run(rank, world, path + "data")


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


def test_two_ranks_print_what_one_prints():
    got = H.two_ranks(_rank_hook, before=lambda path: _fake_cifar(path + "data"))
    with tempfile.TemporaryDirectory() as td:
        text, res, held, radii = _hook_run(0, 1, _fake_cifar(os.path.join(td, "data")))
    print(text)
    said = [l for l in text.splitlines() if "authenticity" in l]
    assert len(said) == 5 and len(_lines(text)) == 3             # the bank, the held-out baseline, live, EMA, the minimum
    assert [l for l in got[0][0].splitlines() if "authenticity" in l] == said
    assert "authenticity" not in got[1][0]                         # rank 1 says nothing
    for r in range(2):
        assert torch.equal(got[r][3], radii)
        _same(got[r][2], held)
        for k in ("live", "EMA"):
            _same(got[r][1][k], res[k])
