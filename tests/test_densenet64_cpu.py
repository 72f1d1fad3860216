"""CPU: the test-side restatement of the DenseNet generator with a size-dependent stem (tests/densenet64_ref.py) against the
oracle at 32 x 32 (oracle/nets_torch.densenet_generator, reference models/densenet.py:51-88), and the variable inventory of the
64 x 64 generator: `dense_0` feeds a 16 x 16 stem, every other variable is as at 32."""
import pytest
import torch

from oracle import nets_torch as NT
from tests import densenet64_ref as R64


def _draw(shapes, gen):
    return [torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1 for s in shapes]


@pytest.mark.parametrize("L", [2, 3])
def test_restated_generator_is_the_oracle_at_32(L):
    gen = torch.Generator().manual_seed(3 + L)
    P = NT.init_params(NT.densenet_gen_shapes("crelu", L), "generator", gen, dtype=torch.float64)
    for p in P.values():            # (g = 1, b = 0 would hide a swapped scale or bias)
        p["g"] = torch.rand(p["g"].shape, generator=gen, dtype=torch.float64) + 0.5
        p["b"] = torch.randn(p["b"].shape, generator=gen, dtype=torch.float64) * 0.1
    us = _draw(R64.noise_shapes(2, 32), gen)
    assert [tuple(u.shape) for u in us] == [(2, 100), (2, 8, 8, 16), (2, 16, 16, 16), (2, 32, 32, 16)]
    want = NT.densenet_generator(us, P, "crelu", L)
    seen = []
    got = R64.generator(us, P, "crelu", L, image_size=32, fix=lambda blk, c0, c1, t: (seen.append((blk, c0, c1)), t)[1])
    assert got.shape == (2, 32, 32, 3)
    assert float((got - want).abs().max()) < 1e-12
    # every rectified tensor is reported once, with its channel range inside its block's list
    width = [16, (32 + 16 * L) // 2, ((32 + 16 * L) // 2 + 16 + 16 * L) // 2]
    assert seen == [(b, c0, c1) for b in range(3)
                    for c0, c1 in [(0, width[b])] + [(width[b] + 16 * (1 + j), width[b] + 16 * (2 + j)) for j in range(L)]]


def test_generator_variables_at_64():
    at32, at64 = R64.gen_shapes(32), R64.gen_shapes(64)
    assert at32 == NT.densenet_gen_shapes()
    assert at64[0] == ("dense_0", (100, 16 * 16 * 16))
    assert at64[1:] == at32[1:] and len(at64) == 52
    gen = torch.Generator().manual_seed(1)
    L = 2
    P = NT.init_params(R64.gen_shapes(64, L=L), "generator", gen, dtype=torch.float64)
    us = _draw(R64.noise_shapes(2, 64), gen)
    assert [tuple(u.shape)[1:3] for u in us[1:]] == [(16, 16), (32, 32), (64, 64)]
    img = R64.generator(us, P, "crelu", L, image_size=64)
    assert img.shape == (2, 64, 64, 3) and float(img.abs().max()) < 1.0


def test_only_32_and_64():
    """The growth kernels take rows of up to 64 pixels: every other size is refused by name, before any GPU work."""
    from otgan_amd.models import densenet
    assert densenet.check_image_size(32) == 32 and densenet.check_image_size(64) == 64
    for size in (48, 128, 16):
        with pytest.raises(ValueError, match="32 or 64"):
            densenet.gen_spec(2, image_size=size, device="cpu")
