"""Test helpers for the growth-layer kernels on two scaled fp16 pieces (tests/test_dense16_h2_gpu.py,
tests/test_densenet64_gpu.py): fp64 references of the CReLU chains (reference utils/nn.py:198-200, models/densenet.py:11-16)
and the calls that prepare the kernels' filters."""
import ctypes

import torch


def crelu_slices(xs):
    """[N,H,W,16 n] -> [N, 32 n, H, W]: the slices interleaved [x_0, -x_0, x_1, -x_1, ...] and rectified (utils/nn.py:198-200)."""
    parts = []
    for s in range(xs.shape[-1] // 16):
        sl = xs[..., 16 * s:16 * s + 16]
        parts += [sl.clamp(min=0), (-sl).clamp(min=0)]
    return torch.cat(parts, -1).permute(0, 3, 1, 2)


def chain_layer(xs, w):
    """conv3x3_same(crelu(xs)) in NHWC; xs [N,H,W,16 k] fp64, w HWIO [9][32 k][16]."""
    k = xs.shape[-1] // 16
    w4 = w.double().reshape(3, 3, 32 * k, 16).permute(3, 2, 0, 1)
    return torch.nn.functional.conv2d(crelu_slices(xs), w4, padding=1).permute(0, 2, 3, 1)


def prepare_filters(L, _lib, ws, dev):
    """ws[k - 1]: HWIO weights [9][32 k][16] of chain layer k = 1 .. len(ws).  Returns (device weights, forward prepared buffers,
    their pointer array): the forward prepare call takes the transposes wT [16][9 * 32 k]."""
    wd = [w.to(dev) for w in ws]
    wTd = [w.reshape(-1, 16).t().contiguous().to(dev) for w in ws]
    nsl = list(range(1, len(ws) + 1))
    fwd = [torch.empty(int(L.otgan_dense16_filter_bytes(n)), dtype=torch.uint8, device=dev) for n in nsl]
    n = len(nsl)
    pw = (ctypes.c_void_p * n)(*[w.data_ptr() for w in wTd])
    pn = (ctypes.c_int * n)(*nsl)
    pf = (ctypes.c_void_p * n)(*[f.data_ptr() for f in fwd])
    _lib.check(L.otgan_dense16_prepare_filters_f32(ctypes.cast(pw, ctypes.c_void_p), ctypes.cast(pn, ctypes.c_void_p),
                                                   ctypes.cast(pf, ctypes.c_void_p), n, _lib.stream_ptr()), "prepare")
    return wd, fwd, pf


def prepare_bwd_filters(L, _lib, wd, fwd, pf, c, dev):
    """Prepared weights of output slice c of a group of len(wd) + 1 slices: one pair per later layer k = c + 1 .. of the group."""
    from otgan_amd._lib_layers import Dense16BwdPair
    S = len(wd) + 1
    npairs = S - 1 - c
    bq = torch.empty(int(L.otgan_dense16_bwd_filter_bytes(npairs)), dtype=torch.uint8, device=dev)
    pairs = [Dense16BwdPair(wd[k - 1].data_ptr(), fwd[k - 1].data_ptr(), bq.data_ptr(), k, c, k - c - 1) for k in range(c + 1, S)]
    arr = (Dense16BwdPair * npairs)(*pairs)
    _lib.check(L.otgan_dense16_prepare_bwd_filters_f32(ctypes.cast(arr, ctypes.c_void_p), npairs, ctypes.cast(pf, ctypes.c_void_p),
                                                       len(wd), _lib.stream_ptr()), "prepare_bwd")
    return bq


def growth_backward_by_slice(dev, N, H, npairs, tol):
    """dense16_bwd_h2_kernel<PT, H> through otgan_dense16_bwd_slice_f32: the gradient of slice 0 of a group gathers from the
    `npairs` later layers of the group, layer k = 1 .. npairs reading slices [0, k) (CReLU backward, reference
    utils/nn.py:198-200).  Reference: fp64 autograd of sum_k <G_k, conv3x3(crelu(slices [0, k)), w_k)> with respect to slice 0,
    added onto the gradient the slice already holds."""
    from otgan_amd import _lib, ops
    L = _lib.lib()
    F = 16
    g = torch.Generator().manual_seed(100 + N + npairs + 64 - H)
    S = npairs + 1                                                        # slices of the group
    ld = S * F + 16                                                       # (a row stride wider than the group)
    X = torch.randn(N, H, H, ld, generator=g)
    G = torch.randn(N, H, H, ld, generator=g)
    G[..., 2 * F:3 * F] *= 37.0                                           # source slices of different magnitudes
    G[3 % N] *= 5.0
    # layer k: HWIO weights [9][32 k][16]
    ws = [(torch.randn(9, 2 * F * k, F, generator=g) * 0.05) for k in range(1, S)]
    # fp64 reference
    x0 = X[..., :F].double().requires_grad_(True)
    total = 0.0
    for k in range(1, S):
        xs = torch.cat([x0, X[..., F:k * F].double()], -1)
        total = total + (chain_layer(xs, ws[k - 1]) * G[..., k * F:(k + 1) * F].double()).sum()
    want = G[..., :F].double() + torch.autograd.grad(total, x0)[0]

    Xd, Gd = X.to(dev), G.to(dev)
    wd, fwd, pf = prepare_filters(L, _lib, ws, dev)
    bq = prepare_bwd_filters(L, _lib, wd, fwd, pf, 0, dev)
    # records: one bounding record, then one per source slice (as otgan_dense16_chain_bwd_f32 passes them), then the output's
    R = torch.zeros((2 + npairs, ops.AMAX_RECORD_FLOATS), device=dev)
    for j in range(npairs):
        R[1 + j, 32 * (j % 16)] = Gd[..., (1 + j) * F:(2 + j) * F].abs().max()
    before = Gd.clone()
    _lib.check(L.otgan_dense16_bwd_slice_f32(N, H, H, npairs, Gd.data_ptr() + 4 * F, ld, bq.data_ptr(), Xd.data_ptr(), ld,
                                             Gd.data_ptr(), R[0].data_ptr(), 1, R[1].data_ptr(), npairs,
                                             R[1 + npairs].data_ptr(), _lib.stream_ptr()), "bwd_slice")
    torch.cuda.synchronize()
    got = Gd[..., :F].double().cpu()
    err = float((got - want).norm() / want.norm())
    print(f"growth backward N={N} H={H} npairs={npairs}: rel L2 {err:.3e}")
    assert err < tol, err
    assert torch.equal(Gd[..., F:], before[..., F:])                     # only slice 0 is written
    assert float(R[1 + npairs].max()) == float(got.abs().max().float())


def chain_backward_reference(X, G, ws):
    """X, G [N,H,W,16 S] fp64: forward values and incoming gradients of a group's S slices; ws[k - 1]: HWIO weights of chain layer
    k, which adds conv3x3(crelu(slices < k)) onto slice k.  Gradient of sum_j <G_j, slice_j> with respect to the slices' initial
    values, by autograd through the chain at the forward values X (initial values chosen so that the chain reproduces X)."""
    S = X.shape[-1] // 16
    with torch.no_grad():
        init = [X[..., :16]] + [X[..., 16 * k:16 * k + 16] - chain_layer(X[..., :16 * k], ws[k - 1]) for k in range(1, S)]
    leaves = [t.clone().requires_grad_(True) for t in init]
    slices = [leaves[0]]
    for k in range(1, S):
        slices.append(leaves[k] + chain_layer(torch.cat(slices, -1), ws[k - 1]))
    total = sum((slices[j] * G[..., 16 * j:16 * j + 16]).sum() for j in range(S))
    return torch.cat(torch.autograd.grad(total, leaves), -1)
