"""The Inception evaluation network on the GPU (csrc/inception.hip through utils/inception_net.py) against fp64: every
convolution geometry of the full 2015 topology, the four pool forms, the resize with its affine, the head, whole
networks against the op-by-op fp64 interpreter (tests/inception_graphs.py), the training hook end to end, and the
reference's own graph file when it is present."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_graphs as G
from otgan_amd import _lib
from otgan_amd._lib_layers import IncepConvDesc, IncepPoolDesc, INCEP_POOL_AVG, INCEP_POOL_MAX
from otgan_amd.utils import inception_net, tfgraph
from otgan_amd.utils.inception import inception_score_from_probs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# relative L2 errors against fp64.  Measured on an MI355X: convolutions worst 7.4e-7 over the 43 geometries; networks
# pool_3 1.3e-7 / 3.0e-7, logits 1.8e-7 / 8.6e-7, probabilities 1.9e-7 / 2.9e-6 (narrow / full).  Bar: 1e-5.
TOL_KERNEL = 1e-5
TOL_NET = 1e-5


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@functools.lru_cache(maxsize=None)
def _plan(which):
    nodes, data = G.full_graph() if which == "full" else G.narrow_graph()
    return nodes, inception_net.lower(tfgraph.parse_graph(data))


@functools.lru_cache(maxsize=None)
def _reference(which, n):
    nodes, _ = _plan(which)
    return G.reference_outputs(nodes, G.images(n, seed=n))


def _conv_ref(x, w, b, stride, same, relu):
    xp, _ = G._nchw_pad(torch.as_tensor(x, dtype=torch.float64), w.shape[:2], stride, same)
    y = F.conv2d(xp, torch.as_tensor(w, dtype=torch.float64).permute(3, 2, 0, 1), stride=stride).permute(0, 2, 3, 1)
    y = y + torch.as_tensor(b, dtype=torch.float64)
    return (y.clamp(min=0) if relu else y).numpy()


def test_every_conv_geometry_of_the_full_graph():
    _, plan = _plan("full")
    geos = sorted({(s[1].H, s[1].W, s[1].C, s[3].shape[0], s[3].shape[1], s[5][0], s[6], s[2].C) for s in plan.convs()})
    assert len(geos) >= 30 and any(g[2] == 3 for g in geos)
    rng = np.random.default_rng(0)
    L = _lib.lib()
    worst = 0.0
    for i, (H, W, C, KH, KW, st, same, Cout) in enumerate(geos):
        N = 2
        x = rng.standard_normal((N, H, W, C)).astype(np.float32)
        w = (rng.standard_normal((KH, KW, C, Cout)) / np.sqrt(KH * KW * C)).astype(np.float32)
        b = rng.standard_normal(Cout).astype(np.float32)
        relu = i % 2 == 0
        OH, OW = L.otgan_incep_out_size(H, KH, st, int(same)), L.otgan_incep_out_size(W, KW, st, int(same))
        coff, ldy = 4, Cout + 12                      # write at a channel offset of a wider buffer
        y = torch.full((N, OH, OW, ldy), 7.0, device=DEV)
        xt, wt, bt = (torch.as_tensor(a, device=DEV) for a in (x, w, b))
        d = IncepConvDesc(N=N, H=H, W=W, C=C, ldx=C, KH=KH, KW=KW, stride_h=st, stride_w=st, same=int(same), Cout=Cout,
                          ldy=ldy, y_coff=coff, relu=int(relu))
        _lib.check(L.otgan_incep_conv2d_f32(ctypes.byref(d), xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), y.data_ptr(),
                                            _lib.stream_ptr()), "conv")
        got = y.cpu().numpy()
        ref = _conv_ref(x, w, b, (st, st), same, relu)
        e = rel(got[..., coff:coff + Cout], ref)
        worst = max(worst, e)
        assert e < TOL_KERNEL, ((H, W, C, KH, KW, st, same, Cout), e)
        assert (got[..., :coff] == 7.0).all() and (got[..., coff + Cout:] == 7.0).all()
    print("conv geometries: %d, worst relative error %.2e" % (len(geos), worst))


def test_conv_reads_a_channel_slice_of_a_wider_buffer():
    rng = np.random.default_rng(1)
    N, H, W, ldx, C, Cout = 2, 17, 17, 40, 12, 24
    x = rng.standard_normal((N, H, W, ldx)).astype(np.float32)
    w = rng.standard_normal((3, 1, C, Cout)).astype(np.float32)
    xt, wt = torch.as_tensor(x, device=DEV), torch.as_tensor(w, device=DEV)
    y = torch.empty(N, H, W, Cout, device=DEV)
    d = IncepConvDesc(N=N, H=H, W=W, C=C, ldx=ldx, KH=3, KW=1, stride_h=1, stride_w=1, same=1, Cout=Cout, ldy=Cout,
                      y_coff=0, relu=0)
    _lib.check(_lib.lib().otgan_incep_conv2d_f32(ctypes.byref(d), xt.data_ptr() + 4 * 8, wt.data_ptr(), None,
                                                 y.data_ptr(), _lib.stream_ptr()), "conv")
    ref = _conv_ref(x[..., 8:8 + C], w, np.zeros(Cout), (1, 1), True, False)
    assert rel(y.cpu().numpy(), ref) < TOL_KERNEL
    bad = IncepConvDesc(N=N, H=2, W=2, C=C, ldx=ldx, KH=3, KW=3, stride_h=1, stride_w=1, same=0, Cout=Cout, ldy=Cout,
                        y_coff=0, relu=0)
    assert _lib.lib().otgan_incep_conv2d_f32(ctypes.byref(bad), xt.data_ptr(), wt.data_ptr(), None, y.data_ptr(),
                                             _lib.stream_ptr()) != 0


@pytest.mark.parametrize("op,k,st,same,H", [("max", 3, 2, False, 35), ("avg", 3, 1, True, 17), ("max", 3, 1, True, 8),
                                            ("avg", 8, 1, False, 8)])
def test_pool_forms(op, k, st, same, H):
    rng = np.random.default_rng(2)
    N, C, ldy, coff = 3, 20, 28, 8
    x = rng.standard_normal((N, H, H, C))
    xt = torch.as_tensor(x, dtype=torch.float32, device=DEV)
    L = _lib.lib()
    OH = L.otgan_incep_out_size(H, k, st, int(same))
    y = torch.full((N, OH, OH, ldy), 3.0, device=DEV)
    d = IncepPoolDesc(N=N, H=H, W=H, C=C, ldx=C, KH=k, KW=k, stride_h=st, stride_w=st, same=int(same),
                      op=INCEP_POOL_MAX if op == "max" else INCEP_POOL_AVG, ldy=ldy, y_coff=coff)
    _lib.check(L.otgan_incep_pool_f32(ctypes.byref(d), xt.data_ptr(), y.data_ptr(), _lib.stream_ptr()), "pool")
    xd = torch.as_tensor(xt.cpu().numpy(), dtype=torch.float64)
    if op == "max":
        xp, _ = G._nchw_pad(xd, (k, k), (st, st), same, value=-float("inf"))
        ref = F.max_pool2d(xp, k, st).permute(0, 2, 3, 1).numpy()
    else:
        xp, _ = G._nchw_pad(xd, (k, k), (st, st), same)
        cnt, _ = G._nchw_pad(torch.ones_like(xd[..., :1]), (k, k), (st, st), same)
        ref = (F.avg_pool2d(xp, k, st) / F.avg_pool2d(cnt, k, st)).permute(0, 2, 3, 1).numpy()
    got = y.cpu().numpy()
    assert rel(got[..., coff:coff + C], ref) < (1e-7 if op == "max" else 1e-6)
    assert (got[..., :coff] == 3.0).all() and (got[..., coff + C:] == 3.0).all()


@pytest.mark.parametrize("size,align", [(299, 0), (75, 1)])
def test_resize_with_affine(size, align):
    x = G.images(3, 32, seed=5)
    y = torch.empty(3, size, size, 3, device=DEV)
    xt = torch.as_tensor(x, device=DEV)
    _lib.check(_lib.lib().otgan_incep_resize_f32(3, 32, 32, 3, size, size, align, 1 / 128.0, -1.0, xt.data_ptr(),
                                                 y.data_ptr(), _lib.stream_ptr()), "resize")
    ref = G.legacy_resize(torch.as_tensor(x, dtype=torch.float64), size, size, bool(align)).numpy() / 128.0 - 1.0
    assert rel(y.cpu().numpy(), ref) < TOL_KERNEL


def test_head():
    rng = np.random.default_rng(3)
    N, C, K = 5, 2048, 1008
    x = np.abs(rng.standard_normal((N, 8, 8, C))).astype(np.float32)
    w = (rng.standard_normal((C, K)) * 0.1).astype(np.float32)
    xt, wt = torch.as_tensor(x, device=DEV), torch.as_tensor(w, device=DEV)
    p3, lg, pr = (torch.empty(N, c, device=DEV) for c in (C, K, K))
    _lib.check(_lib.lib().otgan_incep_head_f32(N, 64, C, C, K, xt.data_ptr(), wt.data_ptr(), p3.data_ptr(), lg.data_ptr(),
                                               pr.data_ptr(), _lib.stream_ptr()), "head")
    p3r = x.astype(np.float64).reshape(N, 64, C).mean(1)
    lgr = p3r @ w.astype(np.float64)
    e = np.exp(lgr - lgr.max(1, keepdims=True))
    assert rel(p3.cpu().numpy(), p3r) < TOL_KERNEL and rel(lg.cpu().numpy(), lgr) < TOL_KERNEL
    assert rel(pr.cpu().numpy(), e / e.sum(1, keepdims=True)) < TOL_KERNEL


@pytest.mark.parametrize("which,n", [("narrow", 8), ("full", 4)])
def test_whole_network_against_the_fp64_interpreter(which, n):
    _, plan = _plan(which)
    net = inception_net.InceptionNet(plan, DEV)
    ims = G.images(n, seed=n)
    pool3, logits, probs = (t.cpu().numpy() for t in net.run(torch.as_tensor(ims, device=DEV)))
    p3r, lgr, prr = _reference(which, n)
    e = (rel(pool3, p3r), rel(logits, lgr), rel(probs, prr))
    print("%s network, %d images: relative errors pool_3 %.2e, logits %.2e, probs %.2e" % ((which, n) + e))
    assert max(e) < TOL_NET, e
    s, sr = inception_score_from_probs(probs, splits=2)[0], inception_score_from_probs(prr, splits=2)[0]
    assert abs(s - sr) <= TOL_NET * sr, (s, sr)
    np.testing.assert_allclose(probs.sum(1), 1.0, rtol=1e-5)
    # the same images given as generator output in [-1, 1]
    g = net.probs_from_generator(torch.as_tensor(ims / 127.5 - 1.0, dtype=torch.float32, device=DEV)).cpu().numpy()
    assert rel(g, prr) < TOL_NET


class _DeviceOnly(torch.Tensor):
    """A sample tensor that must stay on the device: reading it on the host fails."""
    def cpu(self, *a, **k):
        raise AssertionError("a generated sample reached the host")

    def numpy(self, *a, **k):
        raise AssertionError("a generated sample reached the host")

    def __array__(self, *a, **k):
        raise AssertionError("a generated sample reached the host")

    def tolist(self):
        raise AssertionError("a generated sample reached the host")


class _FakeModel:
    def __init__(self):
        self.device = DEV
        self.g = torch.Generator(device=DEV).manual_seed(0)
        self.drawn = {False: [], True: []}

    def sample(self, n, ema=False):
        x = torch.rand((n, 32, 32, 3), generator=self.g, device=DEV) * 2 - 1
        self.drawn[ema].append(x.clone())
        return x.as_subclass(_DeviceOnly)


def test_training_hook_with_the_device_classifier(tmp_path):
    from types import SimpleNamespace
    from otgan_amd.train import inception_hook
    from otgan_amd.utils.inception import load_classifier
    nodes, data = G.narrow_graph()
    path = tmp_path / tfgraph.GRAPH_FILE
    path.write_bytes(data)
    clf = load_classifier(str(path), DEV)
    assert isinstance(clf, inception_net.InceptionNet)
    m = _FakeModel()
    state = {"max": 0.0, "iter": 0, "epoch": 3}
    out = inception_hook(m, SimpleNamespace(eval_samples=20), clf, state)
    for key, ema in (("live", False), ("EMA", True)):
        x = torch.cat(m.drawn[ema]).cpu().numpy().astype(np.float64)
        _, _, pr = G.reference_outputs(nodes, 127.5 * (x + 1.0))
        ref = inception_score_from_probs(pr, splits=10)
        assert out[key][0] == pytest.approx(ref[0], rel=TOL_NET) and out[key][1] == pytest.approx(ref[1], rel=1e-3, abs=1e-6)


def _real_graph_path():
    for p in ("/tmp/imagenet/" + tfgraph.GRAPH_FILE, "/tmp/imagenet/inception-2015-12-05.tgz"):
        if os.path.exists(p):
            return p
    return None


@pytest.mark.skipif(_real_graph_path() is None, reason="the reference's 2015 Inception graph is not on this machine")
def test_the_reference_graph_file_if_present():
    net = inception_net.InceptionNet(_real_graph_path(), DEV)
    assert len(net.plan.convs()) == 94 and net.classes == 1008
    probs = net.probs(torch.as_tensor(G.images(10, seed=9), device=DEV)).cpu().numpy()
    assert probs.shape == (10, 1008) and np.all(np.isfinite(probs))
    np.testing.assert_allclose(probs.sum(1), 1.0, rtol=1e-5)
