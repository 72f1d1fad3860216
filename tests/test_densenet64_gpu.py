"""GPU: `--model densenet --image_size 64`.  The reference hard-codes 32 x 32 (train.py:52,67; models/densenet.py:51-56) but its
DenseNet critic is size-agnostic (models/densenet.py:7-45); the generator takes the build's `image_size` option (stem at
image_size // 4).  Everything on the 64 x 64 path against the fp64 oracle (oracle/nets_torch.py) at the suite's tolerances
(DESIGN section 4): layer kernels 2e-5 relative L2, whole-net forward 5e-5, DenseNet whole-net gradients 2e-4.

The two-scaled-fp16-piece growth kernels pick their tile by N H W / (64 PT) >= 512: at 64 x 64 one row per workgroup up to 8
images, two rows at 16, four from 32 -- hence the batch sizes of the kernel tests: the halo rows between tiles, at the image
edges and across images only exist with more than one row per tile."""
import ctypes

import pytest
import torch

from oracle import nets_torch as NT
from tests import dense16_ref as D16
from tests import densenet64_ref as R64

pytestmark = pytest.mark.gpu

TOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from otgan_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _oracle_params(template):
    P = {}
    for name, v in template.named_variables().items():
        layer, leaf = name.rsplit("/", 1)
        P.setdefault(layer, {})[leaf] = v.detach().double().cpu().requires_grad_(True)
    return P


# ------------------------------------------------------------------------------- 1: growth forward at W = 64
@pytest.mark.parametrize("N,H,n_own", [(2, 64, 1), (2, 64, 3), (16, 64, 2), (32, 64, 7)])
def test_growth_forward_64_vs_fp64(dev, N, H, n_own):
    """dense16_fwd_h2_kernel<PT, 64>, PT = 1 (N = 2), 2 (N = 16), 4 (N = 32), called as tests/test_dense16_h2_gpu.py does at 32."""
    from otgan_amd import _lib, ops
    from otgan_amd._lib_layers import ConvDesc
    L = _lib.lib()
    g = torch.Generator().manual_seed(N + H + n_own)
    C0, F = 32, 16
    Ctot = C0 + 16 * F
    buf = torch.randn(N, H, H, Ctot, generator=g).to(dev)
    buf[..., C0 + 2 * F:C0 + 3 * F] *= 37.0                                # slices of different magnitudes
    g0, k = 1, 1 + n_own                                                  # chain over growth slices [g0, k), output slice k
    wT = (torch.randn(F, 9 * 2 * F * n_own, generator=g) * 0.05).to(dev)
    desc = ConvDesc(N, H, H, n_own * F, Ctot, 0, 3, 3, 1, F, Ctot, C0 + k * F, ops.ACT["crelu"], 1)
    desc.y_accumulate, desc.list_width = 1, F
    assert L.otgan_dense16_h2_ok(ctypes.byref(desc)) == 1
    R = torch.zeros((2 + n_own, ops.AMAX_RECORD_FLOATS), device=dev)
    for j in range(n_own):
        sl = buf[..., C0 + (g0 + j) * F:C0 + (g0 + j + 1) * F]
        R[1 + j, 32 * (j % 16)] = sl.abs().max()
    fq = torch.empty(int(L.otgan_dense16_filter_bytes(n_own)), dtype=torch.uint8, device=dev)
    pw, pn, pf = (ctypes.c_void_p * 1)(wT.data_ptr()), (ctypes.c_int * 1)(n_own), (ctypes.c_void_p * 1)(fq.data_ptr())
    _lib.check(L.otgan_dense16_prepare_filters_f32(ctypes.cast(pw, ctypes.c_void_p), ctypes.cast(pn, ctypes.c_void_p),
                                                   ctypes.cast(pf, ctypes.c_void_p), 1, _lib.stream_ptr()), "prepare")
    desc.x_amax, desc.x_amax_count = R[0].data_ptr(), 1 + n_own
    desc.y_amax_out = R[1 + n_own].data_ptr()
    cmap, _inv = ops.channel_maps((F,) * n_own, ops.ACT["crelu"], dev)
    y0 = buf[..., C0 + k * F:C0 + (k + 1) * F].double().cpu()
    xs = buf[..., C0 + g0 * F:C0 + k * F].double().cpu()
    before = buf.clone()
    ops.conv_fwd_raw(desc, buf[..., C0 + g0 * F:], cmap, wT, None, buf, fq)
    got = buf[..., C0 + k * F:C0 + (k + 1) * F].double().cpu()
    w = wT.double().cpu().reshape(16, 9, 32 * n_own).permute(0, 2, 1).reshape(16, 32 * n_own, 3, 3)
    want = y0 + torch.nn.functional.conv2d(D16.crelu_slices(xs), w, padding=1).permute(0, 2, 3, 1)
    err = float((got - want).norm() / want.norm())
    print(f"growth forward N={N} n_own={n_own}: rel L2 {err:.3e}")
    assert err < TOL, err
    # nothing but the output slice is written
    assert torch.equal(buf[..., :C0 + k * F], before[..., :C0 + k * F])
    assert torch.equal(buf[..., C0 + (k + 1) * F:], before[..., C0 + (k + 1) * F:])
    # the record of the sums written
    assert float(R[1 + n_own].max()) == float(got.abs().max().float())
    # a NaN record (a NaN anywhere in the slices it bounds) must not vanish in the fp16 pieces
    R[1, 0] = float("nan")
    ops.conv_fwd_raw(desc, buf[..., C0 + g0 * F:], cmap, wT, None, buf, fq)
    assert bool(torch.isnan(buf[..., C0 + k * F:C0 + (k + 1) * F]).all())


# ------------------------------------------------------------------------------- 2: growth backward by slice at W = 64
@pytest.mark.parametrize("N,npairs", [(2, 2), (16, 3), (32, 4)])
def test_growth_backward_by_slice_64_vs_fp64(dev, N, npairs):
    """dense16_bwd_h2_kernel<PT, 64> through otgan_dense16_bwd_slice_f32: the gradient of slice 0 of a group gathers from the
    `npairs` later layers of the group, layer k = 1 .. npairs reading slices [0, k) (CReLU backward, reference
    utils/nn.py:198-200).  Reference: fp64 autograd of sum_k <G_k, conv3x3(crelu(slices [0, k)), w_k)> with respect to slice 0,
    added onto the gradient the slice already holds."""
    D16.growth_backward_by_slice(dev, N, 64, npairs, TOL)


# ------------------------------------------------------------------------------- 3: a whole dense block at 64 x 64
_BLOCK_REF = {}


def _block_inputs(N, L):
    """Inputs of the block (C0 = 32, CReLU, 64 x 64) as fp64 copies of fp32 values, and the plain fp64 oracle: its output
    and gradients at its OWN CReLU signs.  Computed once per (batch size, depth), shared by both routes."""
    if (N, L) not in _BLOCK_REF:
        C0, F, H = 32, 16, 64
        gen = torch.Generator().manual_seed(640 + N + L)
        x64 = torch.randn(N, H, H, C0, generator=gen, dtype=torch.float64).float().double()
        P64 = []
        for k in range(L):
            V = (torch.randn(3, 3, (C0 + k * F) * 2, F, generator=gen, dtype=torch.float64) * 0.05).float().double()
            g = (torch.rand(F, generator=gen, dtype=torch.float64) + 0.5).float().double()
            b = (torch.randn(F, generator=gen, dtype=torch.float64) * 0.1).float().double()
            P64.append([V, g, b])
        dy64 = torch.randn(N, H, H, C0 + L * F, generator=gen, dtype=torch.float64).float().double()
        _BLOCK_REF[(N, L)] = (x64, P64, dy64) + _block_oracle(x64, P64, dy64)
    return _BLOCK_REF[(N, L)]


def _block_oracle(x64, P64, dy64, y_hip=None):
    """fp64 chain of convolutions over the growing list (reference models/densenet.py:11-16) and its gradients.  With `y_hip`
    (the fp32 forward under test) every layer output goes on at the signs that forward produced (R64.SignSharing): a unit
    within fp32 rounding of zero may legally land on the other side there, which flips one bit of a CReLU derivative mask --
    an O(1) change of that unit's gradient, not an arithmetic error (tests/test_layers_gpu.py:677-679 measures 9e-5 .. 5e-4
    on the input gradient of a block from it; tests/test_cfg5_gpu.py: _critic_layerwise).  Returns (y, gradients, flips)."""
    C0 = x64.shape[-1]
    x = x64.clone().requires_grad_(True)
    P = [[t.clone().requires_grad_(True) for t in p] for p in P64]
    share = R64.SignSharing()
    feats, c = [x], C0
    for V, g, b in P:
        h = NT.conv2d(feats, {"V": V, "g": g, "b": b}, "crelu", 1, False)
        feats.append(h if y_hip is None else share(h, y_hip[..., c:c + 16]))
        c += 16
    y = torch.cat(feats, 3)
    grads = torch.autograd.grad(y, [x] + [t for p in P for t in p], dy64)
    return y.detach(), grads, share.flips


@pytest.mark.parametrize("route", ["h2", "fp32"])
@pytest.mark.parametrize("N,L", [(2, 4), (32, 4), (2, 8), (32, 8)])
def test_dense_block_64_both_routes(dev, N, L, route, monkeypatch):
    """ops.dense_block_op at 64 x 64 with the plan's two settings for the growth chains -- the two-scaled-fp16-piece kernels
    (h2) and the fp32 / three-piece kernels (the route of the same library call before the 64-wide instantiations): forward and
    every gradient against the fp64 oracle at the block pin of tests/test_layers_gpu.py, 2e-5.  L = 4: the block input's
    convolution would have 64 columns, too few for the Winograd passes, so the block is not cut and both settings run the
    plain chain (dense16_fwd / dgrad / wgrad at W = 64); L = 8 is the shallowest block that is cut: its chains (1 .. 7 slices)
    take the route the plan names.

    The forward pass is compared with the oracle as it is.  The gradients are compared at the CReLU signs of the forward
    pass under test: at 32 images the block rectifies 6 - 12 million growth outputs and one or two of them sit within fp32
    rounding of zero (first run of this test at N = 32, L = 4 without the treatment: y 3.6e-7, dx 6.6e-5, layer 1 dV 1.6e-4).
    Such units must differ from the oracle's by < 2e-6 each and be at most 16 (the cap of the 64 x 64 net tests); where
    there is none the oracle's own gradients are used."""
    from otgan_amd import ops
    C0, F, H = 32, 16, 64
    x64, P64, dy64, y_ref, grads_ref, _ = _block_inputs(N, L)
    monkeypatch.setattr(ops, "DENSE_H2_AT_64", route == "h2")
    ops.bump_weights_epoch()
    plan = ops._split_block_plan(N, H, H, C0, L, F, (C0,), ops.ACT["crelu"], dev)
    if L == 4:
        assert plan is None
    else:
        assert plan is not None and len(plan["wide"]) >= 1       # the block keeps its split at 64 x 64
        assert plan["h2"] == (route == "h2") and max(plan["own_len"]) == 7
    x0 = x64.float().to(dev).requires_grad_(True)
    params = [[t.float().to(dev).requires_grad_(True) for t in p] for p in P64]
    y = ops.dense_block_op(x0, (C0,), params, 3, ops.ACT["crelu"])
    grads = torch.autograd.grad(y, [x0] + [t for p in params for t in p], dy64.float().to(dev))
    ops.join_side_stream(grads)
    torch.cuda.synchronize()
    y_hip = y.detach().double().cpu()
    err_y = _rel(y_hip, y_ref)
    # (the last layer's output is rectified by no layer of the block)
    rectified = slice(C0, C0 + (L - 1) * F)
    differ = int(((torch.sign(y_hip) != torch.sign(y_ref)) & (y_hip != 0))[..., rectified].sum())
    flips = 0
    if differ:
        _, grads_ref, flips = _block_oracle(x64, P64, dy64, y_hip)
    errs = {"y": err_y, "dx": _rel(grads[0], grads_ref[0])}
    for i, (a, r) in enumerate(zip(grads[1:], grads_ref[1:])):
        errs[f"layer {i // 3} d{'Vgb'[i % 3]}"] = _rel(a, r)
    worst = max(errs, key=errs.get)
    print(f"block N={N} L={L} route={route}: y {errs['y']:.2e}, dx {errs['dx']:.2e}, worst {worst} {errs[worst]:.2e}; "
          f"{differ} rectified units at the other sign ({flips} shared incl. the last layer's)")
    assert flips <= 16, flips
    for k, v in errs.items():
        assert v < TOL, (k, v)


# ------------------------------------------------------------------------------- 4: the other 64 x 64 layers
@pytest.mark.parametrize("case", [
    ("transition_64_to_32", 64, 64, 32, "crelu", 2, False, False),
    ("upsample_32_to_64", 32, 64, 32, "crelu", 1, True, False),
    ("rgb_in", 64, 3, 32, None, 1, False, False),
    ("rgb_out_tanh", 64, 64, 3, "crelu", 1, False, True),
], ids=lambda c: c[0])
def test_other_layers_64_vs_fp64(dev, case):
    from otgan_amd import ops
    name, H, Cin, Cout, pre, stride, up, tanh = case
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(2, H, H, Cin, generator=gen)
    V = torch.randn(3, 3, Cin * (2 if pre else 1), Cout, generator=gen) * 0.05
    g = torch.rand(Cout, generator=gen) + 0.5
    b = torch.randn(Cout, generator=gen) * 0.1
    leaves64 = [t.double().requires_grad_(True) for t in (x, V, g, b)]
    y_ref = NT.conv2d([leaves64[0]], dict(zip("Vgb", leaves64[1:])), pre, stride, up)
    if tanh:
        y_ref = torch.tanh(y_ref)
    assert tuple(y_ref.shape) == (2, 32 if stride == 2 else 64, 32 if stride == 2 else 64, Cout)
    dy = torch.randn(y_ref.shape, generator=gen)
    ref = torch.autograd.grad(y_ref, leaves64, dy.double())
    leaves = [t.to(dev).requires_grad_(True) for t in (x, V, g, b)]
    y = ops.conv2d_op(*leaves, stride=stride, upsample=up, preact=ops.ACT[pre], segs=[Cin])
    if tanh:
        y = ops.tanh(y)
    got = torch.autograd.grad(y, leaves, dy.to(dev))
    ops.join_side_stream(got)
    errs = {"y": _rel(y, y_ref)}
    errs.update({n: _rel(a, r) for n, a, r in zip(("dx", "dV", "dg", "db"), got, ref)})
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < TOL, (k, v)


# ------------------------------------------------------------------------------- 5: critic parity
def _critic_layerwise(dev, x, L):
    """The critic with the tensors that get rectified kept (the in-place block buffers and the last transition's output), and
    the oracle run layer by layer at the signs the HIP forward produced (tests/test_cfg5_gpu.py: _critic_layerwise)."""
    from otgan_amd.models import densenet
    from otgan_amd.utils import nn
    bufs, last = [], []

    def spec(z, **kw):
        with nn.arg_scope([nn.conv2d, nn.dense, nn.dense_block], counters={}, init=False, weight_norm=True, ema=None):
            room = L * 16
            z = nn.conv2d(z, 32, pre_activation=None, grow=room)
            for stage in range(3):
                feats = nn.dense_block(z, L, 16, pre_activation="crelu")
                bufs.append(feats.buffer)
                width = sum(int(t.shape[-1]) for t in feats)
                z = nn.conv2d(feats, width // 2, pre_activation="crelu", stride=[2, 2], grow=room if stage < 2 else 0)
            last.append(z)
            return nn.feature_head(z)

    t = nn.make_template("discriminator", spec)
    t.store = densenet.discriminator.store               # shared variables, like make_template
    xg = x.to(dev).requires_grad_(True)
    f = t(xg)
    P = _oracle_params(densenet.discriminator)
    x64 = x.double().requires_grad_(True)
    share = R64.SignSharing()
    k = 0
    h = NT.conv2d(x64, P["discriminator/conv2d_0"], None)
    for stage in range(3):
        buf = bufs[stage]
        c = h.shape[-1]
        xs = [share(h, buf[..., :c])]
        for _r in range(L):
            k += 1
            xs.append(share(NT.conv2d(xs, P[f"discriminator/conv2d_{k}"], "crelu"), buf[..., c:c + 16]))
            c += 16
        assert c == buf.shape[-1]
        k += 1
        h = NT.conv2d(xs, P[f"discriminator/conv2d_{k}"], "crelu", 2)
    f_ref = NT.feature_head(share(h, last[0]))
    units = sum(b.numel() for b in bufs) + last[0].numel()
    return xg, f, x64, f_ref, P, share.flips, units


def test_densenet_64_critic_parity_fwd_and_grads(dev):
    from otgan_amd.models import densenet
    L = 2
    densenet.discriminator.reset(seed=31)
    gen = torch.Generator().manual_seed(8)
    x = torch.rand(2, 64, 64, 3, generator=gen) * 2 - 1
    with torch.no_grad():
        f_plain = densenet.discriminator(x.to(dev), nonlinearity="crelu", layers_per_block=L, image_size=64)
        assert f_plain.shape == (2, 4096)
        f_oracle = NT.densenet_discriminator(x.double(), _oracle_params(densenet.discriminator), "crelu", L)
        print(f"critic 64 forward: rel L2 {_rel(f_plain, f_oracle):.3e}")
        assert _rel(f_plain, f_oracle) < 5e-5
    xg, f, x64, f_ref, P, flips, units = _critic_layerwise(dev, x, L)
    assert torch.equal(f.detach(), f_plain)                             # the layer-wise run IS the model
    print(f"critic 64: {flips} of {units} rectified units share the HIP forward's sign")
    assert 600000 < units < 800000
    assert flips <= 16, flips
    assert _rel(f, f_ref) < 5e-5
    gy = torch.randn(f_ref.shape, generator=gen, dtype=torch.float64).float()
    params = densenet.discriminator.trainable_variables()
    got = torch.autograd.grad(f, [xg] + params, gy.to(dev))
    names = list(densenet.discriminator.named_variables())
    leaves = [x64] + [P[n.rsplit("/", 1)[0]][n.rsplit("/", 1)[1]] for n in names]
    ref = torch.autograd.grad(f_ref, leaves, gy.double())
    errs = {n: _rel(a, r) for n, a, r in zip(["dx"] + names, got, ref)}
    worst = max(errs, key=errs.get)
    print(f"critic 64 gradients: worst {worst} {errs[worst]:.3e}")
    for n, e in errs.items():
        assert e < 2e-4, (n, e)


def test_densenet_64_critic_full_depth_features(dev):
    """layers_per_block = 16: 8 x 8 x 456 features per image, unit rows."""
    from otgan_amd.models import densenet
    densenet.discriminator.reset(seed=32)
    x = torch.rand(2, 64, 64, 3, generator=torch.Generator().manual_seed(9)) * 2 - 1
    with torch.no_grad():
        f = densenet.discriminator(x.to(dev), nonlinearity="crelu")
    assert f.shape == (2, 29184)
    assert bool(torch.isfinite(f).all())
    assert float((f.double().norm(dim=1) - 1).abs().max()) < 1e-5


# ------------------------------------------------------------------------------- 6: generator parity
def _generator_layerwise(dev, us, L, image_size):
    """gen_spec restated with the block buffers kept (every tensor a later CReLU rectifies is a channel slice of one)."""
    from otgan_amd.models import densenet
    from otgan_amd.utils import nn
    bufs = []

    def spec(noise, **kw):
        F, base, B = 16, image_size // 4, noise[0].shape[0]
        with nn.arg_scope([nn.conv2d, nn.dense, nn.dense_block], counters={}, init=False, weight_norm=True, ema=None):
            z = nn.dense(noise[0], base * base * F, pre_activation=None).view(B, base, base, F)
            feats = nn.dense_block([z, noise[1]], L, F, pre_activation="crelu")
            bufs.append(feats.buffer)
            for scale in (2, 3):
                width = sum(int(t.shape[-1]) for t in feats)
                z = nn.conv2d(feats, width // 2, pre_activation="crelu", upsample=True, grow=F + L * F)
                feats = nn.dense_block([z, noise[scale]], L, F, pre_activation="crelu")
                bufs.append(feats.buffer)
            return nn.tanh(nn.conv2d(feats, 3, pre_activation="crelu", init_scale=0.1))

    t = nn.make_template("generator", spec)
    t.store = densenet.generator.store
    img = t([u.to(dev) for u in us])
    return img, bufs


def test_densenet_64_generator_parity_fwd_and_grads(dev):
    from otgan_amd.models import densenet
    L = 3
    densenet.generator.reset(seed=33)
    gen = torch.Generator().manual_seed(10)
    us = [torch.rand(s, generator=gen) * 2 - 1 for s in R64.noise_shapes(2, 64)]
    with torch.no_grad():
        img_plain = densenet.generator(batch_size=2, nonlinearity="crelu", layers_per_block=L, noise=[u.to(dev) for u in us],
                                       image_size=64)
    assert img_plain.shape == (2, 64, 64, 3)
    inventory = {n: tuple(v.shape) for n, v in densenet.generator.named_variables().items()}
    want_inv = {f"generator/{layer}/{leaf}": (shp if leaf == "V" else shp[-1:])
                for layer, shp in R64.gen_shapes(64, L=L) for leaf in "Vgb"}
    assert inventory == want_inv
    img, bufs = _generator_layerwise(dev, us, L, 64)
    assert torch.equal(img.detach(), img_plain)                         # the layer-wise run IS the model
    P = _oracle_params(densenet.generator)
    share = R64.SignSharing()
    img_ref = R64.generator([u.double() for u in us], P, "crelu", L, image_size=64,
                            fix=lambda blk, c0, c1, t: share(t, bufs[blk][..., c0:c1]))
    units = sum(b.numel() for b in bufs)
    print(f"generator 64: image rel L2 {_rel(img, img_ref):.3e}, {share.flips} of {units} units share the HIP forward's sign")
    assert share.flips <= 16, share.flips
    assert _rel(img, img_ref) < 5e-5
    gy = torch.randn(img_ref.shape, generator=gen, dtype=torch.float64).float()
    params = densenet.generator.trainable_variables()
    got = torch.autograd.grad(img, params, gy.to(dev))
    names = list(densenet.generator.named_variables())
    leaves = [P[n.rsplit("/", 1)[0]][n.rsplit("/", 1)[1]] for n in names]
    ref = torch.autograd.grad(img_ref, leaves, gy.double())
    errs = {n: _rel(a, r) for n, a, r in zip(names, got, ref)}
    worst = max(errs, key=errs.get)
    print(f"generator 64 gradients: worst {worst} {errs[worst]:.3e}")
    for n, e in errs.items():
        assert e < 2e-4, (n, e)


def test_generator_at_32_is_unchanged(dev):
    """image_size = 32 (explicit or default) is the generator as it was: same variables, same values for a fixed noise list
    (bit for bit between the two spellings; against the oracle at the whole-net tolerance), same own draws in the same order."""
    from otgan_amd.models import densenet
    L = 3
    densenet.generator.reset(seed=6)
    gen = torch.Generator().manual_seed(1)
    us = [torch.rand(s, generator=gen) * 2 - 1 for s in R64.noise_shapes(2, 32)]
    with torch.no_grad():
        a = densenet.generator(batch_size=2, nonlinearity="crelu", layers_per_block=L, noise=[u.to(dev) for u in us])
        b = densenet.generator(batch_size=2, nonlinearity="crelu", layers_per_block=L, noise=[u.to(dev) for u in us], image_size=32)
    assert torch.equal(a, b) and a.shape == (2, 32, 32, 3)
    inventory = [(n, tuple(v.shape)) for n, v in densenet.generator.named_variables().items() if n.endswith("/V")]
    assert inventory == [(f"generator/{layer}/V", shp) for layer, shp in NT.densenet_gen_shapes("crelu", L)]
    assert _rel(a, NT.densenet_generator([u.double() for u in us], _oracle_params(densenet.generator), "crelu", L)) < 5e-5
    # the generator's own latent: four uniform draws, (B,100), (B,8,8,F), (B,16,16,F), (B,32,32,F), in this order
    torch.manual_seed(5)
    own = [torch.empty(s, device=dev).uniform_(-1.0, 1.0) for s in R64.noise_shapes(2, 32)]
    torch.manual_seed(5)
    with torch.no_grad():
        c = densenet.generator(batch_size=2, nonlinearity="crelu", layers_per_block=L, device=dev)
        d = densenet.generator(batch_size=2, nonlinearity="crelu", layers_per_block=L, noise=own)
    assert torch.equal(c, d)


# ------------------------------------------------------------------------------- 7: trainer
_KW = dict(model="densenet", image_size=64, batch_size=4, nr_gpu=2, nr_sinkhorn_iter=10, nr_gen_per_disc=2)


def _data(m, dev, n, seed):
    gen = torch.Generator().manual_seed(seed)
    xs = [(torch.rand(m.nb, 64, 64, 3, generator=gen) * 2 - 1).to(dev) for _ in range(n)]
    us = [[(torch.rand(s, generator=gen) * 2 - 1).to(dev) for s in R64.noise_shapes(m.nb, 64)] for _ in range(n)]
    return xs, us


def test_trainer_64_constructs_steps_and_samples(dev):
    from otgan_amd.trainer import OTGAN, default_args
    m = OTGAN(default_args(step_graph=False, **_KW), dev)
    try:
        assert m.num_features == 29184
        xs, _ = _data(m, dev, 1, 2)
        kinds = []
        for _ in range(3):                                   # one period: d g g
            r = m.step(xs[0])
            m.check_finite()
            assert bool(torch.isfinite(r["distance"])) and bool(torch.isfinite(r["entropy"]))
            kinds.append(r["kind"])
        assert kinds == ["disc", "gen", "gen"]
        for p in m.disc_params + m.gen_params:
            assert bool(torch.isfinite(p).all())
        for ema in (False, True):
            with torch.no_grad():
                s = m.sample(3, ema=ema)
            assert s.shape == (3, 64, 64, 3)
            assert bool(torch.isfinite(s).all()) and float(s.abs().max()) < 1.0
    finally:
        m.close()


def test_trainer_refuses_other_sizes(dev):
    from otgan_amd.trainer import OTGAN, default_args
    with pytest.raises(ValueError, match="32 or 64"):
        OTGAN(default_args(**dict(_KW, image_size=48)), dev)


def test_resumed_step_64_is_bit_identical(dev, tmp_path):
    from otgan_amd.trainer import OTGAN, default_args
    kw = dict(_KW, step_graph=False)
    m = OTGAN(default_args(seed=6, **kw), dev)
    xs, us = _data(m, dev, 5, 1)
    for i in range(3):
        m.step(xs[i], noise=us[i])
    path = tmp_path / "ckpt"
    torch.save(m.state_dict(), path)
    for i in range(3, 5):                        # uninterrupted: a critic step and a generator step more
        m.step(xs[i], noise=us[i])
    want = {k: v.clone() for k, v in m.state_dict().items() if torch.is_tensor(v)}
    want_ema = {k: v.clone() for k, v in m.state_dict()["__ema__"].items()}
    m.close()
    m2 = OTGAN(default_args(seed=77, **kw), dev)  # different init: everything must come from the file
    m2.load_state_dict(torch.load(path))
    assert m2.step_counter == 3
    for i in range(3, 5):
        m2.step(xs[i], noise=us[i])
    got = m2.state_dict()
    m2.close()
    assert tuple(got["generator/dense_0/V"].shape) == (100, 16 * 16 * 16)
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    for k, v in want_ema.items():
        assert torch.equal(got["__ema__"][k], v), k


def _run(dev, graph, steps):
    from otgan_amd.trainer import OTGAN, default_args
    m = OTGAN(default_args(seed=3, sinkhorn_lambda=100.0, step_graph=graph, **_KW), dev)
    xs, _ = _data(m, dev, 4, 11)
    torch.manual_seed(7)
    dists, kinds = [], []
    for i in range(steps):
        r = m.step(xs[i % 4])
        dists.append(r["distance"].clone())
        kinds.append(r["kind"])
    sd = m.state_dict(full=True)
    out = {"state": {k: v.clone() for k, v in sd.items() if torch.is_tensor(v)}, "opt": sd["__optim__"], "ema": sd["__ema__"],
           "dists": torch.stack(dists).cpu(), "kinds": kinds,
           "captured": sorted(m.graphs.graphs) if m.graphs is not None else [],
           "dead": m.graphs.dead if m.graphs is not None else None,
           "default_on": graph is None and m.graphs is not None}
    m.close()
    return out


def test_replayed_steps_64_equal_eager_steps(dev):
    """Step graphs (on by default for densenet) at 64 x 64: one eager period, then two replayed ones, against the same steps
    run eagerly -- parameters, EMA shadows, optimiser moments and losses bit for bit (tests/test_step_graph_gpu.py)."""
    steps = 3 * 3
    eager = _run(dev, False, steps)
    graph = _run(dev, None, steps)                       # None: the model's default
    assert graph["default_on"] and eager["captured"] == [] and graph["dead"] is None
    assert graph["captured"] == ["disc", "gen", "gen1"]
    assert eager["kinds"] == graph["kinds"] == ["disc", "gen", "gen"] * 3
    assert torch.equal(eager["dists"], graph["dists"]), (eager["dists"], graph["dists"])
    for k in eager["state"]:
        assert torch.equal(eager["state"][k], graph["state"][k]), k
    for k in eager["ema"]:
        assert torch.equal(eager["ema"][k], graph["ema"][k]), k
    for net in ("gen", "disc"):
        assert eager["opt"][net]["t"] == graph["opt"][net]["t"]
        for sa, sb in zip(eager["opt"][net]["slots"], graph["opt"][net]["slots"]):
            for k in sa:
                assert (sa[k] is None and sb[k] is None) or torch.equal(sa[k], sb[k]), (net, k)
