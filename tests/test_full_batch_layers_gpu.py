"""Every layer call of the benchmarked training steps against fp64, in place, at the benchmarked batch.

The real trainer step (eager path: `noise=`, `apply_updates=False`) runs once plain and once with a recorder wrapped
around the layer entry points that `utils/nn.py` looks up on `ops` at call time (conv2d_op, dense_op, dense_block_op, glu,
tanh, feature_head).  The recorder keeps each call's flags and parameter objects, a clone of its input taken BEFORE the
call (a dense block grows in its producer's buffer), a clone of its output, and clones of the gradients that arrive at its
output and at its input (hooks that clone inside the hook: the library reuses gradient buffers in place).  Then every call
is evaluated alone in float64 (oracle/nets_torch.py) on the fp32 input the GPU saw:

  * forward output                  vs the recorded output;
  * VJP under the recorded output gradient:
      - parameter gradients          vs the step's returned gradients (each variable is used once per step kind, so the
                                       step's gradient of a variable IS that layer's weight gradient);
      - input gradient               vs the recorded gradient at the layer's input (every input here has one consumer);
  * dense blocks: each growth layer's forward on its recorded inputs; the backward through an fp64 block in which layer j
    sees the recorded outputs of layers < j (value of the GPU, gradient of the fp64 layer);
  * the junction with the matching (configs[1] / configs[3]): the gradient arriving at the feature head's output vs the
    injected gradient of the fp64 matching oracle on the recorded features (CpuOTGAN.match).

Errors do not compound from layer to layer: every link of the step is checked against fp64 on its own.  The fp64
reference runs on the GPU through torch's own convolution (no kernel of this library); test_fp64_reference_on_gpu pins
it to the CPU.  The reference is evaluated in chunks of images (every layer here is independent per image).

Metrics per tensor: relative L2 error, and the largest per-image relative L2 error (outputs, input gradients) or the
largest per-output-channel error (V: relative L2 of the channel's column; g, b: |error| of the channel over the RMS of
the whole reference gradient), so that a defect confined to the last images or to one column tile cannot hide in a norm
over 1e8 elements.

Configurations, all at their exact benchmarked batch (2 shards x batch_size, critic step on 2 x nb images):
    configs[1]  dcgan     32x32  128 x 2   critic on 512, generator on 256, 100 Sinkhorn iterations
    configs[3]  densenet  32x32  128 x 2   critic on 512, generator on 256, 200 Sinkhorn iterations
    configs[4]  dcgan     64x64  256 x 2   critic on 1024, generator on 512, 100 Sinkhorn iterations (bench's shape)

All three run both step kinds at the exact benchmarked batch.  Measured on an MI355X: 9.0 / 17.3 / 17.9 s per
configuration (steps and recording < 1 s each, the rest the fp64 references), 48 s for the module.

MEASURED worst error over the three configurations (relative L2 / largest per image or per channel) -> BARS (3 x):
    y      layer outputs         3.4e-6 / 3.7e-6   configs[1] critic conv2d_3 (gen step)      -> 1.0e-5 / 1.1e-5
    dx     layer input grads     5.0e-6 / 6.6e-6   configs[1] generator conv2d_0               -> 1.4e-5 / 1.9e-5
    dV                           5.5e-6 / 1.2e-5   configs[4] critic conv2d_1 at 1024 images   -> 1.6e-5 / 3.5e-5
    dg                           4.6e-6 / 2.7e-5   configs[4] critic conv2d_1 at 1024 images   -> 1.3e-5 / 8.0e-5
    db                           1.2e-6 / 2.5e-6   configs[3] critic dense block layer 1       -> 3.5e-6 / 7.5e-6
    y_pw   GLU / tanh / head     5.1e-8 / 6.4e-8                                               -> 1.5e-7 / 1.9e-7
    dx_pw  GLU / tanh / head     5.7e-8 / 1.0e-7                                               -> 1.7e-7 / 3.0e-7
    inj    matching junction     1.2e-5 / 4.0e-5   configs[1] critic step                      -> REL_DIFF_INJECTED / 1.1e-4
Every layer tensor is below the per-layer bar of tests/test_layers_gpu.py (2e-5 relative L2): the split-fp16 engines
cost nothing measurable at the benchmarked batch either.  The largest per-channel figure (dg, 2.7e-5) is a channel's
error over the RMS of the whole gradient, not a relative L2 error.
"""
import gc
import inspect
import math
import time

import pytest
import torch

from conftest import REL_DIFF_INJECTED
from oracle import nets_torch as NT
from oracle.train_step_cpu import CpuOTGAN

pytestmark = pytest.mark.gpu

CASES = {
    "configs1": dict(model="dcgan", batch_size=128, image_size=32, iters=100),
    "configs3": dict(model="densenet", batch_size=128, image_size=32, iters=200),
    "configs4": dict(model="dcgan", batch_size=256, image_size=64, iters=100),
}
LAM = 500.0
CHUNK = 64          # images per fp64 reference evaluation
PRE = {0: None, 1: "crelu", 2: "celu", 3: "elu", 4: "relu"}

# (relative L2, largest per-image / per-channel error) bar per tensor kind: 3 x the worst value measured on an MI355X over
# the three configurations (module docstring).  "_pw": the pointwise layers (GLU, tanh, feature head), plain fp32.
BARS = {
    "y": (1.0e-5, 1.1e-5),
    "dx": (1.4e-5, 1.9e-5),
    "dV": (1.6e-5, 3.5e-5),
    "dg": (1.3e-5, 8.0e-5),
    "db": (3.5e-6, 7.5e-6),
    "y_pw": (1.5e-7, 1.9e-7),
    "dx_pw": (1.7e-7, 3.0e-7),
    "inj": (REL_DIFF_INJECTED, 1.1e-4),
}
POINTWISE = ("glu", "tanh", "feature_head")


# ----------------------------------------------------------------------------------------------------------- recorder
class Recorder:
    """Wraps the layer entry points of `ops`; every wrapper calls the real function and returns its result unchanged."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch, ops):
        for name in ("conv2d_op", "dense_op", "dense_block_op"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name), True))
        for name in ("glu", "tanh", "feature_head"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name), False))

    def _wrap(self, name, fn, layer):
        sig = inspect.signature(fn) if layer else None

        def wrapper(*args, **kwargs):
            x = args[0]
            rec = {"op": name, "x": x.detach().clone(), "grad": torch.is_grad_enabled(), "dy": [], "dx": []}
            if layer:
                a = sig.bind(*args, **kwargs)
                a.apply_defaults()
                a = dict(a.arguments)
                if name == "dense_block_op":
                    rec["params"] = [p for lay in a["params"] for p in lay]
                    rec.update(segs=tuple(a["segs0"]), preact=a["preact"], ksize=a["ksize"], L=len(a["params"]))
                else:
                    rec["params"] = [a["V"], a["g"], a["b"]]
                    rec.update(preact=a["preact"], segs=tuple(a["segs"]) if a["segs"] else None)
                    if name == "conv2d_op":
                        rec.update(stride=a["stride"], upsample=a["upsample"], glu_hint=a["glu_hint"], grow=a["grow"])
            else:
                rec["params"] = []
            rec["diff"] = rec["grad"] and any(p.requires_grad for p in rec["params"])
            rec["x_req"] = rec["grad"] and x.requires_grad
            if rec["x_req"]:
                x.register_hook(lambda g, r=rec: r["dx"].append(g.detach().clone()))
            y = fn(*args, **kwargs)
            rec["y"] = y.detach().clone()
            rec["y_req"] = y.requires_grad
            if y.requires_grad:
                y.register_hook(lambda g, r=rec: r["dy"].append(g.detach().clone()))
            self.calls.append(rec)
            return y
        return wrapper


def _expected_calls(model, kind, nb):
    """(op, first variable of the call, images, flags) of every layer call of one step, in host order."""
    if model == "dcgan":
        def crit(n):
            return ([("conv2d_op", f"discriminator/conv2d_{k}", n, dict(stride=s, preact=p, upsample=False))
                     for k, (s, p) in enumerate(((1, 0), (2, 1), (2, 1), (2, 1)))] + [("feature_head", None, n, {})])

        def gen(n):
            out = [("dense_op", "generator/dense_0", n, dict(preact=0)), ("glu", None, n, {})]
            for k in range(3):
                out += [("conv2d_op", f"generator/conv2d_{k}", n, dict(stride=1, upsample=True, glu_hint=True, preact=0)),
                        ("glu", None, n, {})]
            return out + [("conv2d_op", "generator/conv2d_3", n, dict(stride=1, upsample=False, glu_hint=False, preact=0)),
                          ("tanh", None, n, {})]
    else:
        def crit(n):
            out = [("conv2d_op", "discriminator/conv2d_0", n, dict(stride=1, preact=0))]
            for s in range(3):
                out += [("dense_block_op", f"discriminator/conv2d_{1 + 17 * s}", n, dict(L=16, preact=1)),
                        ("conv2d_op", f"discriminator/conv2d_{17 + 17 * s}", n, dict(stride=2, preact=1))]
            return out + [("feature_head", None, n, {})]

        def gen(n):
            out = [("dense_op", "generator/dense_0", n, dict(preact=0))]
            for blk, first in enumerate((0, 17, 34)):
                out.append(("dense_block_op", f"generator/conv2d_{first}", n, dict(L=16, preact=1)))
                if blk < 2:
                    out.append(("conv2d_op", f"generator/conv2d_{first + 16}", n, dict(stride=1, upsample=True, preact=1)))
            return out + [("conv2d_op", "generator/conv2d_50", n, dict(stride=1, upsample=False, preact=1)),
                          ("tanh", None, n, {})]
    return gen(nb) + crit(2 * nb) if kind == "disc" else crit(nb) + gen(nb) + crit(nb)


# ----------------------------------------------------------------------------------------------------------- metrics
class _Acc:
    """Relative L2 error and largest per-image relative L2 error of a tensor compared chunk by chunk (dim 0 = images)."""

    def __init__(self):
        self.num = self.den = self.worst = 0.0

    def add(self, got, ref):
        d = (got.double() - ref).reshape(ref.shape[0], -1).pow(2).sum(1)
        r = ref.reshape(ref.shape[0], -1).pow(2).sum(1)
        self.num += float(d.sum())
        self.den += float(r.sum())
        self.worst = max(self.worst, float((d / r.clamp_min(1e-300)).sqrt().max()))

    def result(self):
        return math.sqrt(self.num / max(self.den, 1e-300)), self.worst


def _param_errors(got, ref):
    """(relative L2, largest per-output-channel error); the output channel is the last axis."""
    d = got.double() - ref
    l2 = float(d.norm() / ref.norm().clamp_min(1e-300))
    if ref.dim() > 1:
        C = ref.shape[-1]
        per = d.reshape(-1, C).norm(dim=0) / ref.reshape(-1, C).norm(dim=0).clamp_min(1e-300)
    else:
        per = d.abs() / ref.pow(2).mean().sqrt().clamp_min(1e-300)
    return l2, float(per.max())


# ----------------------------------------------------------------------------------------------------------- fp64 reference
def _split(x, segs, dim):
    return list(torch.split(x, list(segs), dim=dim)) if segs and len(segs) > 1 else [x]


def _layer_fn(call):
    """fp64 restatement of one recorded call: (x chunk, fp64 parameters, image slice) -> output chunk."""
    op = call["op"]
    if op == "conv2d_op":
        return lambda x, P, sl: NT.conv2d(_split(x, call["segs"], 3), dict(V=P[0], g=P[1], b=P[2]), PRE[call["preact"]],
                                          call["stride"], call["upsample"])
    if op == "dense_op":
        return lambda x, P, sl: NT.dense(_split(x, call["segs"], 1), dict(V=P[0], g=P[1], b=P[2]), PRE[call["preact"]])
    if op == "glu":
        return lambda x, P, sl: NT.glu(x, -1)
    if op == "tanh":
        return lambda x, P, sl: torch.tanh(x)
    if op == "feature_head":
        assert NT.FORCED_HEAD_SIGNS is None
        return lambda x, P, sl: NT.feature_head(x)
    assert op == "dense_block_op"
    L, C0 = call["L"], call["x"].shape[-1]
    F = call["params"][0].shape[-1]
    call["layer_acc"] = [_Acc() for _ in range(L)]

    def block(x, P, sl):
        rec = call["y"][sl]
        feats = _split(x, call["segs"], 3)
        hs = []
        for j in range(L):
            out = NT.conv2d(feats + hs, dict(V=P[3 * j], g=P[3 * j + 1], b=P[3 * j + 2]), PRE[call["preact"]])
            got = rec[..., C0 + j * F:C0 + (j + 1) * F]
            call["layer_acc"][j].add(got, out.detach())
            # the value the GPU produced, the gradient of the fp64 layer
            hs.append(got.double() + (out - out.detach()))
        return torch.cat([x] + hs, 3)
    return block


def _evaluate(call, grads_by_id):
    """fp64 evaluation of one call -> {tensor kind: (relative L2, largest per-image / per-channel), ...} (+ per-layer rows
    of a dense block)."""
    fn = _layer_fn(call)
    x, N = call["x"], call["x"].shape[0]
    dy = call["dy"][0] if call["dy"] else None
    dx_gpu = call["dx"][0] if call["dx"] else None
    want_p = call["diff"] and dy is not None
    want_x = dx_gpu is not None and dy is not None
    P = [p.detach().double().requires_grad_(want_p) for p in call["params"]]
    acc_y, acc_dx, pg = _Acc(), _Acc(), None
    for i0 in range(0, N, CHUNK):
        sl = slice(i0, min(N, i0 + CHUNK))
        xc = x[sl].double().requires_grad_(want_x)
        with torch.set_grad_enabled(want_p or want_x):
            yc = fn(xc, P, sl)
        if call["op"] != "dense_block_op":
            acc_y.add(call["y"][sl], yc.detach())
        if want_p or want_x:
            leaves = ([xc] if want_x else []) + (P if want_p else [])
            gs = list(torch.autograd.grad(yc, leaves, dy[sl].double()))
            if want_x:
                acc_dx.add(dx_gpu[sl], gs.pop(0))
            if want_p:
                pg = gs if pg is None else [a + b for a, b in zip(pg, gs)]
        del yc, xc
    res = []
    if call["op"] == "dense_block_op":
        res += [(f"[{j}] y", "y") + call["layer_acc"][j].result() for j in range(call["L"])]
    else:
        res.append(("y", "y") + acc_y.result())
    if want_x:
        res.append(("dx", "dx") + acc_dx.result())
    if want_p:
        for i, (p, ref) in enumerate(zip(call["params"], pg)):
            kind = "dV" if i % 3 == 0 else "dg" if i % 3 == 1 else "db"
            tag = kind if call["op"] != "dense_block_op" else f"[{i // 3}] {kind}"
            res.append((tag, kind) + _param_errors(grads_by_id[id(p)], ref))
    return res


def _injected(f_gen, f_dat, iters):
    """The fp64 matching oracle's injected gradients (CpuOTGAN.match, NumPy matching) on the recorded features."""
    o = CpuOTGAN.__new__(CpuOTGAN)
    o.use_c, o.dtype = False, torch.float64
    g_gen, g_dat, _dist, _ent = o.match(f_gen.double().cpu(), f_dat.double().cpu(), 2, LAM, iters)
    return g_gen, g_dat


# ----------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_fp64_reference_on_gpu(dev):
    """The reference path of this module: nets_torch.conv2d in float64 on the GPU (torch's own convolution) equals the
    same on the CPU -- forward and VJP -- upsampled, stride 2, and a list input with CReLU."""
    gen = torch.Generator().manual_seed(5)
    cases = [((3, 4, 4, 32), (32,), 5, 16, None, 1, True),
             ((3, 9, 9, 24), (24,), 5, 32, "crelu", 2, False),
             ((2, 8, 8, 40), (16, 8, 16), 3, 16, "crelu", 1, False)]
    for shape, segs, k, cout, pre, stride, up in cases:
        mult = 2 if pre == "crelu" else 1
        x = torch.randn(shape, generator=gen, dtype=torch.float64)
        p = dict(V=torch.randn(k, k, shape[-1] * mult, cout, generator=gen, dtype=torch.float64) * 0.05,
                 g=1 + 0.1 * torch.randn(cout, generator=gen, dtype=torch.float64),
                 b=0.1 * torch.randn(cout, generator=gen, dtype=torch.float64))
        outs = []
        for d in ("cpu", dev):
            xd = x.to(d).requires_grad_(True)
            pd = {n: t.to(d).requires_grad_(True) for n, t in p.items()}
            y = NT.conv2d(_split(xd, segs, 3), pd, pre, stride, up)
            dy = torch.sin(torch.arange(y.numel(), dtype=torch.float64)).reshape(y.shape).to(d)
            outs.append([y] + list(torch.autograd.grad(y, [xd, pd["V"], pd["g"], pd["b"]], dy)))
        for a, b in zip(*outs):
            err = float((a.detach().cpu() - b.detach().cpu()).norm() / b.detach().cpu().norm())
            assert err < 1e-12, (shape, pre, stride, up, err)


@pytest.mark.parametrize("case", list(CASES))
def test_full_batch_layers_vs_fp64(dev, case, monkeypatch):
    from otgan_amd import ops
    from otgan_amd.trainer import OTGAN, default_args
    c = CASES[case]
    t0 = time.perf_counter()
    kw = dict(image_size=c["image_size"]) if c["image_size"] != 32 else {}
    args = default_args(model=c["model"], batch_size=c["batch_size"], nr_gpu=2, sinkhorn_lambda=LAM,
                        nr_sinkhorn_iter=c["iters"], seed=3, **kw)
    m = OTGAN(args, dev)
    nb, S = m.nb, c["image_size"]
    gen = torch.Generator().manual_seed(17)
    x = (torch.rand(nb, S, S, 3, generator=gen) * 2 - 1).to(dev)
    if c["model"] == "dcgan":
        noise = (torch.rand(nb, 100, generator=gen) * 2 - 1).to(dev)
    else:
        noise = [(torch.rand(shp, generator=gen) * 2 - 1).to(dev)
                 for shp in ((nb, 100), (nb, 8, 8, 16), (nb, 16, 16, 16), (nb, 32, 32, 16))]
    names = {id(p): n for tpl in (m.discriminator, m.generator) for n, p in tpl.named_variables().items()}

    def run(kind):
        m.step_counter = 0 if kind == "disc" else 1
        r = m.step(x, noise=noise, apply_updates=False)
        torch.cuda.synchronize()
        assert r["kind"] == kind
        return r

    steps = {}
    for kind in ("disc", "gen"):
        plain = run(kind)
        plain = (plain["distance"].clone(), plain["entropy"].clone(), [g.clone() for g in plain["grads"]])
        rec = Recorder()
        rec.install(monkeypatch, ops)
        try:
            r = run(kind)
        finally:
            monkeypatch.undo()
        # the recorder changes nothing: bit-identical gradients; distance and entropy to the last bits of their fp64
        # sums (the Sinkhorn kernels add the per-wave partial statistics with fp64 atomics, in arrival order, once a
        # problem spans several workgroups: N = 256 in configs[4])
        assert len(r["grads"]) == len(plain[2])
        for g0, g1 in zip(plain[2], r["grads"]):
            assert torch.equal(g0, g1), kind
        for a, b in ((r["distance"], plain[0]), (r["entropy"], plain[1])):
            assert abs(float(a) - float(b)) <= 1e-13 * abs(float(b)), (kind, float(a), float(b))
        params = m.disc_params if kind == "disc" else m.gen_params
        steps[kind] = (rec.calls, {id(p): g for p, g in zip(params, r["grads"])}, params)
        del plain, r
    t_steps = time.perf_counter() - t0
    print(f"\n{case}: steps + recording {t_steps:.1f} s", flush=True)

    rows, failures = [], []

    def report(kind, label, tag, tkind, l2, worst):
        rows.append((case, kind, label, tag, l2, worst, tkind))
        bar_l2, bar_max = BARS[tkind]
        if not (l2 <= bar_l2 and worst <= bar_max):
            failures.append((case, kind, label, tag, l2, worst))

    for kind in ("disc", "gen"):
        calls, grads_by_id, params = steps[kind]
        # coverage: the recorded calls are the model's layers, in order, at the step's batch
        got = [(cl["op"], names[id(cl["params"][0])][:-2] if cl["params"] else None, cl["x"].shape[0]) for cl in calls]
        want = _expected_calls(c["model"], kind, nb)
        assert got == [w[:3] for w in want], (kind, got)
        for cl, w in zip(calls, want):
            for f, v in w[3].items():
                assert cl[f] == v, (kind, w[:3], f, cl[f], v)
            # every output that carries a gradient received it once; so did every input that requires one
            assert len(cl["dy"]) == int(cl["y_req"]) and len(cl["dx"]) == int(cl["x_req"]), (kind, w[:3])
            assert cl["y_req"] == cl["grad"], (kind, w[:3])
        # each variable of the differentiated network is used by exactly one differentiated call of the step
        used = [id(p) for cl in calls if cl["diff"] for p in cl["params"]]
        assert sorted(used) == sorted(id(p) for p in params), kind
        # the junction with the matching
        heads = [cl for cl in calls if cl["op"] == "feature_head"]
        if case != "configs4":
            if kind == "disc":
                f = heads[0]["y"]
                g_gen, g_dat = _injected(f[nb:], f[:nb], c["iters"])
                ref = torch.cat([g_dat, g_gen], 0)
            else:
                g_gen, _ = _injected(heads[1]["y"], heads[0]["y"], c["iters"])
                ref = g_gen
            acc = _Acc()
            acc.add(heads[-1]["dy"][0].cpu(), ref)
            report(kind, "matching>feature_head", "inj", "inj", *acc.result())
        # every call against its fp64 evaluation
        prev = None
        for i, cl in enumerate(calls):
            label = names[id(cl["params"][0])].rsplit("/", 1)[0] if cl["params"] else f"{prev}>{cl['op']}"
            prev = label
            for tag, tkind, l2, worst in _evaluate(cl, grads_by_id):
                tkind += "_pw" if cl["op"] in POINTWISE else ""
                report(kind, f"{i:02d} {label} @{cl['x'].shape[0]}", tag, tkind, l2, worst)
            cl.clear()
        torch.cuda.empty_cache()
        print(f"{case}: {kind} step references done at {time.perf_counter() - t0:.1f} s", flush=True)
    del steps
    m.close()
    gc.collect()
    torch.cuda.empty_cache()
    t_all = time.perf_counter() - t0

    print(f"\n{case}: {c}  steps + recording {t_steps:.1f} s, fp64 references {t_all - t_steps:.1f} s, total {t_all:.1f} s")
    print(f"{'config':9} {'step':4} {'call':52} {'tensor':10} {'rel L2':>9} {'max img/ch':>10}")
    for r in rows:
        print(f"{r[0]:9} {r[1]:4} {r[2]:52} {r[3]:10} {r[4]:9.2e} {r[5]:10.2e}")
    worst = {}
    for r in rows:
        k = r[6]
        worst[k] = (max(worst.get(k, (0, 0))[0], r[4]), max(worst.get(k, (0, 0))[1], r[5]))
    print(f"{case} worst per tensor kind: " + ", ".join(f"{k} {v[0]:.2e} / {v[1]:.2e}" for k, v in sorted(worst.items())))
    assert not failures, (len(failures), failures[:12])
