"""Test helpers for DenseNet at 64x64 (tests/test_densenet64_cpu.py, tests/test_densenet64_gpu.py).

The oracle's DenseNet generator (oracle/nets_torch.densenet_generator, reference models/densenet.py:51-88) reshapes its stem
to 8 x 8, the reference's only size.  `generator` restates it from the oracle's own layers (NT.dense / NT.conv2d) with the stem
at image_size // 4 -- the build's `image_size` option -- and is pinned to the oracle at 32 (to 1e-12, CPU test).  `fix`
(optional) sees every tensor that a later CReLU rectifies, as (block, first channel, last channel, tensor), and returns what
the oracle goes on with: the GPU tests use it to differentiate both sides at the same CReLU signs (tests/test_cfg5_gpu.py:
_critic_layerwise)."""
import torch

from oracle import nets_torch as NT


def gen_shapes(image_size=32, nonlinearity="crelu", L=16, Fg=16):
    """Variable shapes of the generator: the oracle's at 32, with dense_0 widened to the (image_size // 4)^2 stem."""
    base = image_size // 4
    shapes = NT.densenet_gen_shapes(nonlinearity, L, Fg)
    assert shapes[0] == ("dense_0", (100, 8 * 8 * Fg))
    return [("dense_0", (100, base * base * Fg))] + shapes[1:]


def noise_shapes(B, image_size=32, Fg=16):
    base = image_size // 4
    return [(B, 100), (B, base, base, Fg), (B, 2 * base, 2 * base, Fg), (B, 4 * base, 4 * base, Fg)]


def generator(us, P, nonlinearity="crelu", L=16, Fg=16, image_size=32, scope="generator", fix=None):
    """models/densenet.py:51-88 with the stem at image_size // 4; us as noise_shapes()."""
    fix = fix or (lambda blk, c0, c1, t: t)
    B, base, k = us[0].shape[0], image_size // 4, 0
    x = NT.dense(us[0], P[f"{scope}/dense_0"], None).reshape(B, base, base, Fg)
    for blk in range(3):
        c = x.shape[-1]
        xs = [fix(blk, 0, c, x), us[blk + 1]]
        c += Fg
        for _r in range(L):
            xs.append(fix(blk, c, c + Fg, NT.conv2d(xs, P[f"{scope}/conv2d_{k}"], nonlinearity)))
            c, k = c + Fg, k + 1
        if blk < 2:
            x = NT.conv2d(xs, P[f"{scope}/conv2d_{k}"], nonlinearity, 1, True)
            k += 1
    return torch.tanh(NT.conv2d(xs, P[f"{scope}/conv2d_{k}"], nonlinearity, init_scale=0.1))


class SignSharing:
    """Units whose sign differs between the fp32 forward under test (`a`) and the fp64 oracle (`h`) are moved onto the fp32
    value in the oracle, so that both sides differentiate the same piecewise-linear function.  Only rounding-level units may
    differ: each by < 2e-6 (asserted here); the caller bounds `flips`."""

    def __init__(self):
        self.flips = 0

    def __call__(self, h, a):
        a = a.detach().double().cpu()
        differ = (torch.sign(a) != torch.sign(h.detach())) & (a != 0)
        if differ.any():
            assert float((h.detach() - a).abs()[differ].max()) < 2e-6
            self.flips += int(differ.sum())
        return h + torch.where(differ, a - h.detach(), torch.zeros_like(a))
