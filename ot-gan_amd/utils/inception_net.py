"""The reference's Inception network (the 2015 graph `classify_image_graph_def.pb`, reference utils/inception.py:55-93)
run on the library's gfx950 kernels (csrc/inception.hip).

`lower(nodes)` turns a GraphDef (utils/tfgraph.py) into an execution plan: the subgraph from the feed `ExpandDims:0`
to `pool_3:0` plus the weight matrix that is input 1 of `softmax/logits/MatMul` -- the only names the reference uses;
everything else is recognised by op type and attributes.  Rewrites, once at load (fp64):
  * every BatchNormWithGlobalNormalization folds into the preceding Conv2D's weights and bias, every Relu into the
    convolution's epilogue;
  * no Concat / ConcatV2 is executed: each producer writes at its channel offset of the concat's buffer;
  * the scalar Sub / Mul / Add / RealDiv around the ResizeBilinear fold into the resize kernel's affine.
The probabilities are the reference's: softmax(squeeze(pool_3) . W) WITHOUT the graph's softmax bias
(utils/inception.py:91-93), not the graph's own `softmax:0`.

`InceptionNet(plan_or_path, device)` runs a plan on CUDA tensors with a grow-only activation arena.
"""
import ctypes

import numpy as np

from .. import _lib
from .._lib_layers import IncepConvDesc, IncepPoolDesc, INCEP_POOL_MAX, INCEP_POOL_AVG

FEED, POOL3, LOGITS_MATMUL = "ExpandDims", "pool_3", "softmax/logits/MatMul"
_ALIAS = ("Identity", "CheckNumerics")
_AFFINE = ("Sub", "Mul", "Add", "RealDiv")


def _tname(ref):
    """'name:0' / 'name' -> node name; control inputs ('^name') -> None."""
    if ref.startswith("^"):
        return None
    return ref.split(":")[0]


def _out_size(n, k, s, same):
    return -(-n // s) if same else (n - k) // s + 1


class Tensor:
    """An activation [n, H, W, C] of the plan."""
    def __init__(self, H, W, C, name):
        self.H, self.W, self.C, self.name = H, W, C, name
        self.root, self.coff = self, 0      # buffer and channel offset (concat members write into the concat's buffer)
        self.step = None                    # producing step (None for a concat)
        self.parts = None                   # concat: [(Tensor, channel offset)]


class Plan:
    """Steps in execution order:
        ("resize", out, OH, OW, align_corners, a, b)      out = a * resize(input) + b (3 channels, dense)
        ("conv", x, out, w [KH,KW,C,Cout] f64, bias f64, (sh, sw), same, relu)
        ("pool", x, out, op 'max'/'avg', (KH, KW), (sh, sw), same)
        ("head", x, HW)                                    pool_3 = mean of the HW pixels; logits = pool_3 . W
    `weights`: [C, classes] of the logits MatMul."""
    def __init__(self):
        self.steps, self.buffers = [], []
        self.weights = None
        self.pool3_channels = 0

    def convs(self):
        return [s for s in self.steps if s[0] == "conv"]

    def flops_per_image(self):
        f = 0
        for s in self.steps:
            if s[0] == "conv":
                w, out = s[3], s[2]
                f += 2.0 * out.H * out.W * w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3]
        f += 2.0 * self.weights.shape[0] * self.weights.shape[1]
        return f


def _topo(nodes_by, targets):
    order, state = [], {}
    for t in targets:
        stack = [(t, False)]
        while stack:
            name, done = stack.pop()
            if done:
                if state.get(name) != 2:
                    state[name] = 2
                    order.append(name)
                continue
            if state.get(name):
                continue
            state[name] = 1
            stack.append((name, True))
            if name == FEED:
                continue
            if name not in nodes_by:
                raise ValueError("GraphDef: input %r of the plan is not a node of the graph" % name)
            for ref in nodes_by[name].inputs:
                dep = _tname(ref)
                if dep is not None and not state.get(dep):
                    stack.append((dep, False))
    return order


def _attr_list(node, key, default=None):
    v = node.attr.get(key, default)
    if v is None:
        raise ValueError("%s node %r: attribute %r missing" % (node.op, node.name, key))
    return list(v)


def _padding(node):
    p = node.attr.get("padding")
    p = p.decode() if isinstance(p, bytes) else p
    if p not in ("SAME", "VALID"):
        raise ValueError("%s node %r: padding %r (SAME or VALID)" % (node.op, node.name, p))
    return p == "SAME"


def _nhwc(node):
    fmt = node.attr.get("data_format")
    if fmt not in (None, b"NHWC", "NHWC"):
        raise ValueError("%s node %r: data_format %r (NHWC only)" % (node.op, node.name, fmt))


def lower(nodes):
    """GraphDef nodes -> Plan.  Fails loudly on any op on the path it does not implement."""
    by = {n.name: n for n in nodes}
    if POOL3 not in by:
        raise ValueError("GraphDef: no node %r (the reference reads pool_3:0)" % POOL3)
    if LOGITS_MATMUL not in by:
        raise ValueError("GraphDef: no node %r (the reference takes its input 1 as the logits weights)" % LOGITS_MATMUL)
    order = _topo(by, [POOL3])
    uses = {}
    for name in order:
        if name == FEED:
            continue
        for ref in by[name].inputs:
            d = _tname(ref)
            if d is not None:
                uses[d] = uses.get(d, 0) + 1

    plan = Plan()
    val = {}

    def const(name, what):
        v = val[name]
        if not isinstance(v, np.ndarray):
            raise ValueError("%s: input %r is not a constant" % (what, name))
        return v

    for name in order:
        if name == FEED:
            val[name] = ("input", 1.0, 0.0)
            continue
        node = by[name]
        op, ins = node.op, [d for d in (_tname(r) for r in node.inputs) if d is not None]
        what = "%s node %r" % (op, name)
        if op == "Const":
            val[name] = np.asarray(node.attr.get("value"))
        elif op in _ALIAS:
            val[name] = val[ins[0]]
        elif op in _AFFINE:
            a_, b_ = val[ins[0]], val[ins[1]]
            if isinstance(b_, np.ndarray) and b_.size == 1:
                x, c, const_first = a_, float(b_.reshape(())), False
            elif isinstance(a_, np.ndarray) and a_.size == 1:
                x, c, const_first = b_, float(a_.reshape(())), True
            else:
                raise ValueError("%s: only a scalar constant operand is supported" % what)
            if op == "RealDiv" and (const_first or c == 0.0):
                raise ValueError("%s: only a division by a non-zero constant is an affine map" % what)
            ma, mb = {"Sub": ((-1.0, c) if const_first else (1.0, -c)), "Mul": (c, 0.0), "Add": (1.0, c),
                      "RealDiv": (1.0 / c if c else 0.0, 0.0)}[op]
            if isinstance(x, tuple) and x[0] == "input":
                val[name] = ("input", ma * x[1], ma * x[2] + mb)
            elif isinstance(x, Tensor) and x.step is not None and x.step[0] == "resize" and uses.get(ins[1 if const_first else 0], 0) == 1:
                s = x.step
                x.step = (s[0], s[1], s[2], s[3], s[4], ma * s[5], ma * s[6] + mb)
                plan.steps[plan.steps.index(s)] = x.step
                val[name] = x
            else:
                raise ValueError("%s: a scalar affine map is supported only on the input and the resize" % what)
        elif op == "ResizeBilinear":
            x, size = val[ins[0]], const(ins[1], what).reshape(-1)
            if not (isinstance(x, tuple) and x[0] == "input"):
                raise ValueError("%s: the resize must read the input" % what)
            out = Tensor(int(size[0]), int(size[1]), 3, name)
            out.step = ("resize", out, out.H, out.W, bool(node.attr.get("align_corners") or False), x[1], x[2])
            plan.steps.append(out.step)
            val[name] = out
        elif op == "Conv2D":
            _nhwc(node)
            x, w = val[ins[0]], const(ins[1], what)
            if not isinstance(x, Tensor):
                raise ValueError("%s: input is not an activation after the resize" % what)
            st = _attr_list(node, "strides")
            dil = list(node.attr.get("dilations") or [1, 1, 1, 1])
            if len(st) != 4 or st[0] != 1 or st[3] != 1 or any(d != 1 for d in dil):
                raise ValueError("%s: strides %s / dilations %s not supported" % (what, st, dil))
            if w.ndim != 4 or w.shape[2] != x.C:
                raise ValueError("%s: filter %s for %d input channels" % (what, w.shape, x.C))
            same = _padding(node)
            out = Tensor(_out_size(x.H, w.shape[0], st[1], same), _out_size(x.W, w.shape[1], st[2], same), w.shape[3], name)
            out.step = ["conv", x, out, w.astype(np.float64), np.zeros(w.shape[3]), (st[1], st[2]), same, False]
            plan.steps.append(out.step)
            val[name] = out
        elif op == "BatchNormWithGlobalNormalization":
            t = val[ins[0]]
            if not (isinstance(t, Tensor) and t.step is not None and t.step[0] == "conv" and not t.step[7]
                    and uses.get(ins[0], 0) == 1):
                raise ValueError("%s: batch norm is folded only into a convolution it alone reads" % what)
            m, v, beta, gamma = (const(i, what).astype(np.float64).reshape(-1) for i in ins[1:5])
            eps = float(node.attr.get("variance_epsilon") or 0.0)
            scale = 1.0 / np.sqrt(v + eps)
            if node.attr.get("scale_after_normalization"):
                scale = scale * gamma
            s = t.step
            s[3] = s[3] * scale
            s[4] = (s[4] - m) * scale + beta
            val[name] = t
        elif op == "Relu":
            t = val[ins[0]]
            if not (isinstance(t, Tensor) and t.step is not None and t.step[0] == "conv" and uses.get(ins[0], 0) == 1):
                raise ValueError("%s: relu is fused only into a convolution it alone reads" % what)
            t.step[7] = True
            val[name] = t
        elif op in ("MaxPool", "AvgPool"):
            _nhwc(node)
            x = val[ins[0]]
            if not isinstance(x, Tensor):
                raise ValueError("%s: input is not an activation" % what)
            k, st = _attr_list(node, "ksize"), _attr_list(node, "strides")
            if len(k) != 4 or k[0] != 1 or k[3] != 1 or st[0] != 1 or st[3] != 1:
                raise ValueError("%s: ksize %s / strides %s not supported" % (what, k, st))
            same = _padding(node)
            out = Tensor(_out_size(x.H, k[1], st[1], same), _out_size(x.W, k[2], st[2], same), x.C, name)
            out.step = ("pool", x, out, "max" if op == "MaxPool" else "avg", (k[1], k[2]), (st[1], st[2]), same)
            plan.steps.append(out.step)
            val[name] = out
        elif op in ("Concat", "ConcatV2"):
            ax_name, parts = (ins[0], ins[1:]) if op == "Concat" else (ins[-1], ins[:-1])
            axis = int(const(ax_name, what).reshape(()))
            if axis not in (3, -1):
                raise ValueError("%s: concat along axis %d (channels only)" % (what, axis))
            ts = [val[p] for p in parts]
            if not all(isinstance(t, Tensor) and (t.parts or t.step is not None and t.step[0] in ("conv", "pool"))
                       for t in ts):
                raise ValueError("%s: every input must be a convolution, pool or concat output" % what)
            if len({(t.H, t.W) for t in ts}) != 1:
                raise ValueError("%s: spatial sizes differ" % what)
            out = Tensor(ts[0].H, ts[0].W, sum(t.C for t in ts), name)
            out.parts, off = [], 0
            for t in ts:
                out.parts.append((t, off))
                off += t.C
            val[name] = out
        elif op in ("Reshape", "Squeeze"):
            t = val[ins[0]]
            if not (isinstance(t, Tensor) and t.H == 1 and t.W == 1):
                raise ValueError("%s: only the pooled [n, 1, 1, C] tensor is reshaped" % what)
            val[name] = t
        else:
            raise ValueError("unsupported op %s at node %r on the path to pool_3" % (op, name))

    out = val[POOL3]
    if not (isinstance(out, Tensor) and out.H == 1 and out.W == 1):
        raise ValueError("pool_3 is not a [n, 1, 1, C] activation")
    w_name = _tname(by[LOGITS_MATMUL].inputs[1])
    while by[w_name].op in _ALIAS:
        w_name = _tname(by[w_name].inputs[0])
    if by[w_name].op != "Const":
        raise ValueError("input 1 of %s is not a constant" % LOGITS_MATMUL)
    W = np.asarray(by[w_name].attr["value"], np.float64)
    if W.ndim != 2 or W.shape[0] != out.C:
        raise ValueError("logits weights %s for pool_3 of %d channels" % (W.shape, out.C))
    plan.weights = W
    plan.pool3_channels = out.C

    # the last average pool over the whole grid runs inside the head kernel
    s = out.step
    if s is not None and s[0] == "pool" and s[3] == "avg" and not s[6] and s[4] == (s[1].H, s[1].W):
        plan.steps.remove(s)
        plan.steps.append(("head", s[1], s[1].H * s[1].W))
    else:
        plan.steps.append(("head", out, 1))

    # concats: members write into the outermost concat's buffer (outer concats first: nested offsets compose)
    concats = [v for v in dict.fromkeys(x for x in val.values() if isinstance(x, Tensor) and x.parts)]
    for c in reversed(sorted(concats, key=lambda t: order.index(t.name))):
        for t, off in c.parts:
            t.root, t.coff = c.root, c.coff + off
    _layout(plan)
    return plan


def _layout(plan):
    """Arena offsets (floats per image, multiples of 64) of every buffer, reusing memory of dead buffers."""
    first, last = {}, {}
    for i, s in enumerate(plan.steps):
        reads = [] if s[0] == "resize" else [s[1]]
        writes = [] if s[0] == "head" else [s[2] if s[0] != "resize" else s[1]]
        for t in writes:
            first.setdefault(id(t.root), (i, t.root))
            last[id(t.root)] = max(last.get(id(t.root), i), i)
        for t in reads:
            last[id(t.root)] = max(last.get(id(t.root), i), i)
    bufs = sorted(first.values(), key=lambda p: p[0])
    free, live, peak = [], [], 0          # free: [(offset, size)]

    def size_of(t):
        return -(-t.H * t.W * t.C // 64) * 64

    for i, t in bufs:
        for lt in [x for x in live if last[id(x)] < i]:
            live.remove(lt)
            free.append((lt.offset, size_of(lt)))
        free.sort()
        merged = []
        for o, sz in free:
            if merged and merged[-1][0] + merged[-1][1] == o:
                merged[-1] = (merged[-1][0], merged[-1][1] + sz)
            else:
                merged.append((o, sz))
        free = merged
        need = size_of(t)
        for j, (o, sz) in enumerate(free):
            if sz >= need:
                t.offset = o
                free[j] = (o + need, sz - need)
                break
        else:
            if free and free[-1][0] + free[-1][1] == peak:
                o, sz = free.pop()
                t.offset, peak = o, o + need
            else:
                t.offset, peak = peak, peak + need
        live.append(t)
    plan.buffers = [t for _, t in bufs]
    plan.arena_floats_per_image = peak


class InceptionNet:
    """The plan on one device.  probs(x) / pool3(x): x = CUDA float tensor [n, H, W, 3] in 0..255 (the contract of the
    reference's get_inception_score); probs_from_generator(x): generator output in [-1, 1] (the reference's
    127.5 (x + 1), train.py:260-261, folded into the resize).  Batches of `batch_size` images at a time; the activation
    arena grows to the largest batch seen and is reused."""

    def __init__(self, plan_or_path, device="cuda", batch_size=500):
        import torch
        if not isinstance(plan_or_path, Plan):
            from .tfgraph import load_graph
            plan_or_path = lower(load_graph(plan_or_path))
        self.plan, self.device, self.batch_size = plan_or_path, torch.device(device), int(batch_size)
        self._w = {}
        for s in self.plan.steps:
            if s[0] == "conv":
                w = torch.as_tensor(s[3], dtype=torch.float32).contiguous().to(self.device)
                self._w[id(s)] = (w, torch.as_tensor(s[4], dtype=torch.float32).to(self.device))
        self._W = torch.as_tensor(self.plan.weights, dtype=torch.float32).contiguous().to(self.device)
        self._arena = None
        self.classes = self.plan.weights.shape[1]
        self.flops_per_image = self.plan.flops_per_image()

    def _buf(self, n):
        import torch
        need = self.plan.arena_floats_per_image * n
        if self._arena is None or self._arena.numel() < need:
            self._arena = None
            self._arena = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._arena

    def _run(self, x, scale, shift):
        """-> (pool3 [n, C], logits [n, classes], probs [n, classes]) of one batch."""
        import torch
        n, H, W, C = x.shape
        x = x.to(self.device, torch.float32).contiguous()
        arena = self._buf(n)
        base = arena.data_ptr()
        L, st = _lib.lib(), _lib.stream_ptr()

        def addr(t):
            return base + 4 * (t.root.offset * n + t.coff)

        pool3 = torch.empty(n, self.plan.pool3_channels, device=self.device)
        logits = torch.empty(n, self.classes, device=self.device)
        probs = torch.empty(n, self.classes, device=self.device)
        for s in self.plan.steps:
            kind = s[0]
            if kind == "resize":
                out, a, b = s[1], s[5], s[6]
                _lib.check(L.otgan_incep_resize_f32(n, H, W, C, s[2], s[3], int(s[4]), a * scale, a * shift + b,
                                                    x.data_ptr(), addr(out), st), "incep_resize")
            elif kind == "conv":
                xt, out, w = s[1], s[2], s[3]
                d = IncepConvDesc(N=n, H=xt.H, W=xt.W, C=xt.C, ldx=xt.root.C, KH=w.shape[0], KW=w.shape[1],
                                  stride_h=s[5][0], stride_w=s[5][1], same=int(s[6]), Cout=out.C, ldy=out.root.C,
                                  y_coff=0, relu=int(s[7]))
                wt, bt = self._w[id(s)]
                _lib.check(L.otgan_incep_conv2d_f32(ctypes.byref(d), addr(xt), wt.data_ptr(), bt.data_ptr(), addr(out),
                                                    st), "incep_conv2d")
            elif kind == "pool":
                xt, out = s[1], s[2]
                d = IncepPoolDesc(N=n, H=xt.H, W=xt.W, C=xt.C, ldx=xt.root.C, KH=s[4][0], KW=s[4][1],
                                  stride_h=s[5][0], stride_w=s[5][1], same=int(s[6]),
                                  op=INCEP_POOL_MAX if s[3] == "max" else INCEP_POOL_AVG, ldy=out.root.C, y_coff=0)
                _lib.check(L.otgan_incep_pool_f32(ctypes.byref(d), addr(xt), addr(out), st), "incep_pool")
            else:
                xt, hw = s[1], s[2]
                _lib.check(L.otgan_incep_head_f32(n, hw, xt.C, xt.root.C, self.classes, addr(xt), self._W.data_ptr(),
                                                  pool3.data_ptr(), logits.data_ptr(), probs.data_ptr(), st),
                           "incep_head")
        return pool3, logits, probs

    def run(self, x, scale=1.0, shift=0.0):
        """(pool3, logits, probs) of every image, `batch_size` at a time; x: [n, H, W, 3] on the device."""
        import torch
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError("images must be [n, H, W, 3]")
        if not x.is_cuda:
            raise _lib.OtganError("InceptionNet runs on CUDA (MI355X) tensors; there is no CPU fallback")
        outs = [self._run(x[i:i + self.batch_size], scale, shift) for i in range(0, x.shape[0], self.batch_size)]
        return tuple(torch.cat(o, 0) if len(o) > 1 else o[0] for o in zip(*outs))

    def probs(self, x):
        return self.run(x)[2]

    def pool3(self, x):
        return self.run(x)[0]

    def probs_from_generator(self, x):
        """class probabilities of generator output x in [-1, 1]: the images 127.5 (x + 1)"""
        return self.run(x, 127.5, 127.5)[2]

    def probs_and_pool3_from_generator(self, x):
        """(class probabilities, pool_3) of generator output x in [-1, 1] from ONE forward pass: the Inception score
        reads the first, the Frechet distance (utils/fid.py) the second"""
        pool3, _, probs = self.run(x, 127.5, 127.5)
        return probs, pool3

    def __call__(self, images):
        """numpy [n, H, W, 3] in 0..255 -> numpy probabilities: the classifier callable of utils/inception.py"""
        import torch
        return self.probs(torch.as_tensor(np.ascontiguousarray(images, np.float32), device=self.device)).cpu().numpy()
