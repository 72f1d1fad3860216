"""GPU: --swd_samples in train.main: the three lines it prints against utils.swd.distances recomputed from the same seed, the
training run unmoved by the hook (eager DCGAN, and DenseNet with replayed step graphs), and two ranks against one process."""
import contextlib
import io
import math
import os
import re
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SWD = ["--swd_samples", "32", "--swd_patches", "8", "--swd_dirs", "4", "--swd_repeats", "2"]
LINE = r"sliced Wasserstein distance x 1e3 was 32x32: ([0-9.]+|nan|inf), 16x16: ([0-9.]+|nan|inf), average ([0-9.]+|nan|inf)"


def _main(save_dir, steps, extra):
    from otgan_amd import train
    argv = ["--synthetic", "--synthetic_size", "64", "--batch_size", "4", "--nr_gpu", "2", "--nr_sinkhorn_iter", "10",
            "--eval_every", "2", "--max_steps", str(steps), "--save_dir", str(save_dir)] + list(extra)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        m = train.main(argv)
    return m, buf.getvalue()


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


def test_train_main_prints_the_distances(tmp_path):
    """16 steps = two epochs of eight, --eval_every 2: the hook runs once, after the last step, without an --inception_model.
    The printed figures are those of swd.distances on the same training images, positions, directions and latents."""
    from otgan_amd import train
    from otgan_amd.utils import swd
    m, out = _main(tmp_path, 16, SWD)
    try:
        assert m.step_counter == 16
        assert "no --inception_model" in out
        live = [l for l in out.splitlines() if l.startswith("sliced Wasserstein distance x 1e3 was")]
        ema = [l for l in out.splitlines() if l.startswith("EMA sliced Wasserstein distance x 1e3 was")]
        low = [l for l in out.splitlines() if l.startswith("min average SWD was")]
        assert len(live) == len(ema) == len(low) == 1, out
        for line in live + ema:
            vals = [float(v) for v in re.search(LINE, line).groups()]
            assert all(math.isfinite(v) and v > 0 for v in vals), line
        # the same numbers from the parts: the data of --seed 1, the state the hook builds, the model as the run left it
        args = train.build_parser().parse_args(["--synthetic", "--synthetic_size", "64"] + SWD)
        np.random.seed(args.seed)
        trainx = np.random.rand(64, 32, 32, 3).astype(np.float32) * 2 - 1
        with contextlib.redirect_stdout(io.StringIO()):
            state = train.swd_state(args, trainx, m.device)
        assert state["n"] == 32 and tuple(state["real"].sorted[0].shape) == (8, 32 * 8)
        best = float("inf")
        for tag, is_ema, line in (("", False, live[0]), ("EMA ", True, ema[0])):
            images = swd.sample_images(m, 32, args.seed, ema=is_ema)
            assert images.dtype == torch.uint8 and tuple(images.shape) == (32, 32, 32, 3)
            per, avg = swd.summary(swd.distances(images, state["real"]))
            want = '%ssliced Wasserstein distance x 1e3 was 32x32: %.4f, 16x16: %.4f, average %.4f' % (tag, per[0], per[1], avg)
            print(want)
            assert line == want
            best = min(best, avg)
        assert low[0] == 'min average SWD was %.4f, iter was 1' % best
    finally:
        m.close()


def test_without_the_flag_nothing_is_said(tmp_path):
    m, out = _main(tmp_path, 16, [])
    m.close()
    assert "SWD" not in out and "sliced Wasserstein" not in out


def _identical(tmp_path, extra):
    """24 steps = three epochs: the hook runs after the second, the third trains on."""
    states = []
    for flags in ([], SWD):
        m, out = _main(tmp_path, 24, list(extra) + flags)
        assert m.step_counter == 24
        assert out.count("min average SWD was") == (1 if flags else 0)
        if "--step_graph" in extra:
            assert m.graphs is not None and m.graphs.dead is None and len(m.graphs.graphs) > 0      # the steps were replayed
        states.append(_flat("", m.state_dict(full=True), {}))
        m.close()
    a, b = states
    assert a.keys() == b.keys() and sum(torch.is_tensor(v) for v in a.values()) > 20
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_the_hook_does_not_move_the_run(tmp_path):
    """Eager DCGAN: parameters, optimiser moments and EMA shadows after 24 steps are the bits of the run without the flag -- the
    hook saves the device generator's state, samples from its own seeds and puts the state back."""
    _identical(tmp_path, ["--model", "dcgan"])


def test_the_hook_does_not_move_a_run_of_replayed_step_graphs(tmp_path):
    """--model densenet --step_graph 1: the same guarantee with the steps replayed as graphs."""
    _identical(tmp_path, ["--model", "densenet", "--step_graph", "1"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _hook_run(rank, world):
    """The hook on a freshly initialised model (every process builds the same one from the seeds below) against 48 synthetic
    uint8 images: 40 samples in batches of 500 are one batch, so SAMPLE_BATCH is lowered to 16 to give both ranks batches."""
    from otgan_amd import train
    from otgan_amd.trainer import OTGAN, default_args
    from otgan_amd.utils import swd
    dev = torch.device("cuda:0")
    np.random.seed(3)
    torch.manual_seed(3)
    args = default_args(model="dcgan", batch_size=4, nr_gpu=2, nr_sinkhorn_iter=10, seed=3, swd_samples=40, swd_patches=8,
                        swd_dirs=5, swd_repeats=3)
    m = OTGAN(args, dev)
    trainx = np.random.RandomState(9).rand(48, 32, 32, 3).astype(np.float32) * 2 - 1
    buf = io.StringIO()
    batch, swd.SAMPLE_BATCH = swd.SAMPLE_BATCH, 16
    try:
        with contextlib.redirect_stdout(buf):
            state = train.swd_state(args, trainx, dev, rank, world)
            state["epoch"] = 7
            res = train.swd_hook(m, args, state, rank, world)
    finally:
        swd.SAMPLE_BATCH = batch
        m.close()
    return buf.getvalue(), res, tuple(state["real"].sorted[0].shape)


def _worker(rank, world, port, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from otgan_amd import parallel
    parallel.init_from_env(backend="gloo")
    torch.cuda.set_device(0)
    torch.save(_hook_run(rank, world), path + str(rank))
    parallel.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_print_what_one_prints():
    """Two gloo ranks on one device: each samples its share of the batches and computes its share of the 15 directions (8 and
    7); the gathered table is averaged in one order, so rank 0's lines are the single process's, digit for digit, and the
    returned floats are equal."""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out")
        port = _free_port()
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_worker, args=(r, 2, port, path)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
            assert p.exitcode == 0
        got = [torch.load(path + str(r), weights_only=False) for r in range(2)]
    text, res, shape = _hook_run(0, 1)
    print(text)
    assert shape == (15, 40 * 8) and got[0][2] == (8, 40 * 8) and got[1][2] == (7, 40 * 8)
    lines = [l for l in text.splitlines() if "liced Wasserstein distance x 1e3 was" in l or l.startswith("min average SWD")]
    assert len(lines) == 3
    assert [l for l in got[0][0].splitlines() if l in lines] == lines
    assert "sliced Wasserstein distance x 1e3" not in got[1][0]                # rank 1 says nothing
    assert got[0][1] == res and got[1][1] == res
