"""What the end-to-end tests of the metrics beside the Inception score (tests/test_fid_gpu.py, test_kid_gpu.py,
test_pr_gpu.py) share: the narrow graph (C = 40) lowered for the device, two 96-image sets, their fp64 interpreter
outputs, a model that replays rows as device-only samples, the two-rank plumbing and train.main's common flags."""
import functools
import os
import socket
import tempfile

import numpy as np
import torch

import inception_graphs as G
from otgan_amd.utils import inception_net, tfgraph

DEV = torch.device("cuda:0")
SEED = 5
EVALS = (96, 95)        # 95: the ranks draw 48 each and the last row of rank 1 falls to the truncation


@functools.lru_cache(maxsize=None)
def graph():
    nodes, data = G.narrow_graph()
    return nodes, data, inception_net.lower(tfgraph.parse_graph(data))


@functools.lru_cache(maxsize=None)
def sets():
    """Set A and set B as generator output in [-1, 1] (fp32), the form the hook and `trainx` have."""
    a = G.images(96, seed=1)
    b = G.images(96, seed=2)
    b = np.clip(0.5 * b + 0.25 * np.roll(b, 1, axis=2) + 40, 0, 255)
    return tuple((im / 127.5 - 1.0).astype(np.float32) for im in (a, b))


@functools.lru_cache(maxsize=None)
def interpreter(which):
    """fp64 (pool_3, probabilities) of the images the device network sees for set `which`: 127.5 (x + 1)."""
    x = sets()[which].astype(np.float64)
    p3, _, pr = G.reference_outputs(graph()[0], 127.5 * (x + 1.0))
    return p3, pr


def net():
    return inception_net.InceptionNet(graph()[2], DEV)


def pool3(net, x):
    return net.run(torch.as_tensor(x, device=DEV), 127.5, 127.5)[0]


class DeviceOnly(torch.Tensor):
    """A sample tensor that must stay on the device: reading it on the host fails."""
    def cpu(self, *a, **k):
        raise AssertionError("a generated sample reached the host")

    def numpy(self, *a, **k):
        raise AssertionError("a generated sample reached the host")

    def __array__(self, *a, **k):
        raise AssertionError("a generated sample reached the host")

    def tolist(self):
        raise AssertionError("a generated sample reached the host")


class Replay:
    """A model whose generator (and EMA generator) replays the rows of x in the batches the hook asks for."""
    def __init__(self, x):
        self.device = DEV
        self.x = torch.as_tensor(x, device=DEV)
        self.at = {False: 0, True: 0}

    def sample(self, n, ema=False):
        i = self.at[ema]
        assert i + n <= self.x.shape[0], "the hook drew more samples than its share"
        self.at[ema] = i + n
        return self.x[i:i + n].clone().as_subclass(DeviceOnly)


def state(**real):
    """the hook's state in epoch 3, with the real side of the metrics under test"""
    return {"max": 0.0, "iter": 0, "epoch": 3, **real}


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(worker, rank, world, port, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from otgan_amd import parallel
    parallel.init_from_env(backend="gloo")
    torch.cuda.set_device(0)
    torch.save(worker(rank, world, path), path + str(rank))
    parallel.barrier()
    torch.distributed.destroy_process_group()


def two_ranks(worker, before=None):
    """What worker(rank, world, path) -- a module-level function -- returns in each of two spawned rank processes on this
    device; `before(path)` may leave files beside `path` for them first."""
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r")
        if before is not None:
            before(path)
        port = free_port()
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_rank_main, args=(worker, r, 2, port, path)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
            assert p.exitcode == 0
        return [torch.load(path + str(r)) for r in range(2)]


def train_args(tmp_path):
    """train.main's flags for a six-step synthetic run with the narrow graph as --inception_model (the last two entries):
    3 steps per epoch, epochs 0 and 1; the hook runs after epoch 1 (train.py:245 skips the first epoch of a run)."""
    path = tmp_path / tfgraph.GRAPH_FILE
    path.write_bytes(graph()[1])
    return ["--synthetic", "--synthetic_size", "48", "--nr_gpu", "2", "--batch_size", "8", "--nr_sinkhorn_iter", "10",
            "--sinkhorn_lambda", "100", "--nr_gen_per_disc", "2", "--save_dir", str(tmp_path / "run"), "--seed", "3",
            "--max_steps", "6", "--eval_every", "1", "--eval_samples", "20", "--inception_model", str(path)]


def kinds(lines, names):
    return [k for l in lines for k in names if l.startswith(k)]
