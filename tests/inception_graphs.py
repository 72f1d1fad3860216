"""Test helpers for the Inception evaluation network (utils/tfgraph.py, utils/inception_net.py):

* a GraphDef WRITER: protobuf wire-format bytes of an Inception-style graph with random weights, in the naming and op
  set of the 2015 `classify_image_graph_def.pb` (Conv2D -> BatchNormWithGlobalNormalization -> CheckNumerics ->
  Identity -> Relu, Concat joins, ExpandDims -> ResizeBilinear -> Sub 128 -> Mul 1/128, pool_3, softmax/logits/MatMul):
  `narrow_graph()` (few channels, 32 -> 75 resize) and `full_graph()` (the full 2015 topology, 94 convolutions);
* an fp64 INTERPRETER on torch CPU that walks the writer's node list op by op, with no folding and no fusion.  It
  reads neither the GraphDef bytes nor anything of the product's lowering.
"""
import functools
import struct

import numpy as np


# ---------------------------------------------------------------- protobuf wire format
def _varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(num, wt):
    return _varint((num << 3) | wt)


def f_varint(num, v):
    return _key(num, 0) + _varint(int(v))


def f_bytes(num, b):
    if isinstance(b, str):
        b = b.encode()
    return _key(num, 2) + _varint(len(b)) + bytes(b)


def f_float(num, v):
    return _key(num, 5) + struct.pack("<f", v)


def shape_proto(dims):
    return b"".join(f_bytes(2, f_varint(1, d)) for d in dims)


def tensor_proto(arr, use_content=True, fill=None):
    """TensorProto of a float32 / int32 array: tensor_content (little-endian) or float_val / int_val (packed);
    fill: write the single value `fill` for the whole shape (the broadcast form)."""
    arr = np.asarray(arr)
    is_f = arr.dtype.kind == "f"
    out = f_varint(1, 1 if is_f else 3) + f_bytes(2, shape_proto(arr.shape))
    if fill is not None:
        out += f_float(5, fill) if is_f else f_varint(7, fill)
    elif use_content:
        out += f_bytes(4, arr.astype("<f4" if is_f else "<i4").tobytes())
    elif is_f:
        out += f_bytes(5, arr.astype("<f4").tobytes())                      # packed float_val
    else:
        out += f_bytes(7, b"".join(_varint(int(x)) for x in arr.reshape(-1)))   # packed int_val
    return out


def attr_value(v):
    if isinstance(v, bool):
        return f_varint(5, v)
    if isinstance(v, int):
        return f_varint(3, v)
    if isinstance(v, float):
        return f_float(4, v)
    if isinstance(v, (bytes, str)):
        return f_bytes(2, v)
    if isinstance(v, tuple) and v[0] == "type":
        return f_varint(6, v[1])
    if isinstance(v, tuple) and v[0] == "shape":
        return f_bytes(7, shape_proto(v[1]))
    if isinstance(v, tuple) and v[0] == "tensor":
        return f_bytes(8, tensor_proto(*v[1:]))
    if isinstance(v, list):
        if all(isinstance(x, int) for x in v):
            body = f_bytes(3, b"".join(_varint(x) for x in v))                # packed ints
        elif all(isinstance(x, float) for x in v):
            body = b"".join(f_float(4, x) for x in v)                         # unpacked floats
        else:
            body = b"".join(f_bytes(2, x) for x in v)
        return f_bytes(1, body)
    raise TypeError(v)


def node_proto(n):
    out = f_bytes(1, n["name"]) + f_bytes(2, n["op"])
    for i in n["inputs"]:
        out += f_bytes(3, i)
    for k, v in sorted(n["attr"].items()):
        out += f_bytes(5, f_bytes(1, k) + f_bytes(2, attr_value(v)))
    return out


def graph_bytes(nodes):
    return b"".join(f_bytes(1, node_proto(n)) for n in nodes) + f_bytes(4, f_varint(1, 9))


# ---------------------------------------------------------------- graph builder
class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.nodes, self.values = [], {}
        self.n_conv = 0

    def node(self, name, op, inputs=(), **attr):
        self.nodes.append({"name": name, "op": op, "inputs": list(inputs), "attr": attr})
        return name

    def const(self, name, arr):
        arr = np.asarray(arr)
        self.values[name] = arr
        return self.node(name, "Const", value=("tensor", arr), dtype=("type", 1 if arr.dtype.kind == "f" else 3))

    def conv(self, name, x, cin, cout, kh, kw, stride=1, padding="SAME"):
        """Conv2D -> BatchNormWithGlobalNormalization -> CheckNumerics -> Identity -> Relu, 2015 naming."""
        self.n_conv += 1
        rng = self.rng
        w = (rng.standard_normal((kh, kw, cin, cout)) * np.sqrt(2.0 / (kh * kw * cin))).astype(np.float32)
        c = self.node(name + "/Conv2D", "Conv2D", [x, self.const(name + "/conv2d_params", w)],
                      strides=[1, stride, stride, 1], padding=padding, T=("type", 1))
        mean = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        var = rng.uniform(0.6, 1.4, cout).astype(np.float32)
        beta = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        gamma = rng.uniform(0.8, 1.2, cout).astype(np.float32)
        bn = self.node(name + "/batchnorm", "BatchNormWithGlobalNormalization",
                       [c, self.const(name + "/batchnorm/moving_mean", mean),
                        self.const(name + "/batchnorm/moving_variance", var),
                        self.const(name + "/batchnorm/beta", beta), self.const(name + "/batchnorm/gamma", gamma)],
                       variance_epsilon=0.001, scale_after_normalization=False, T=("type", 1))
        ck = self.node(name + "/CheckNumerics", "CheckNumerics", [bn], message="bn", T=("type", 1))
        ident = self.node(name + "/control_dependency", "Identity", [bn, "^" + ck], T=("type", 1))
        return self.node(name, "Relu", [ident], T=("type", 1))

    def pool(self, name, x, op, k, stride, padding):
        return self.node(name, op, [x], ksize=[1, k, k, 1], strides=[1, stride, stride, 1], padding=padding,
                         T=("type", 1))

    def concat(self, name, xs):
        ax = self.const(name + "/concat_dim", np.array(3, np.int32))
        return self.node(name, "Concat", [ax] + list(xs), N=len(xs), T=("type", 1))

    def input_chain(self, size):
        x = self.node("ExpandDims", "Placeholder", dtype=("type", 1))
        r = self.node("ResizeBilinear", "ResizeBilinear",
                      [x, self.const("ResizeBilinear/size", np.array([size, size], np.int32))], align_corners=False,
                      T=("type", 1))
        s = self.node("Sub", "Sub", [r, self.const("Sub/y", np.array(128.0, np.float32))], T=("type", 1))
        return self.node("Mul", "Mul", [s, self.const("Mul/y", np.array(1.0 / 128.0, np.float32))], T=("type", 1))

    def head(self, x, c, classes=1008):
        p = self.pool("pool_3", x, "AvgPool", 8, 1, "VALID")
        r = self.node("pool_3/_reshape", "Reshape", [p, self.const("pool_3/_reshape/shape", np.array([-1, c], np.int32))],
                      T=("type", 1))
        W = (self.rng.standard_normal((c, classes)) * (4.0 / np.sqrt(c))).astype(np.float32)
        m = self.node("softmax/logits/MatMul", "MatMul", [r, self.const("softmax/weights", W)], T=("type", 1))
        b = self.node("softmax/logits", "BiasAdd",
                      [m, self.const("softmax/biases", self.rng.standard_normal(classes).astype(np.float32))],
                      T=("type", 1))
        self.node("softmax", "Softmax", [b], T=("type", 1))


def _block_a(b, name, x, cin, pool_c):
    b1 = b.conv(name + "/conv", x, cin, 64, 1, 1)
    t = b.conv(name + "/tower/conv", x, cin, 48, 1, 1)
    b2 = b.conv(name + "/tower/conv_1", t, 48, 64, 5, 5)
    t = b.conv(name + "/tower_1/conv", x, cin, 64, 1, 1)
    t = b.conv(name + "/tower_1/conv_1", t, 64, 96, 3, 3)
    b3 = b.conv(name + "/tower_1/conv_2", t, 96, 96, 3, 3)
    p = b.pool(name + "/tower_2/pool", x, "AvgPool", 3, 1, "SAME")
    b4 = b.conv(name + "/tower_2/conv", p, cin, pool_c, 1, 1)
    return b.concat(name + "/join", [b1, b2, b3, b4]), 64 + 64 + 96 + pool_c


def _block_c(b, name, x, c7):
    b1 = b.conv(name + "/conv", x, 768, 192, 1, 1)
    t = b.conv(name + "/tower/conv", x, 768, c7, 1, 1)
    t = b.conv(name + "/tower/conv_1", t, c7, c7, 1, 7)
    b2 = b.conv(name + "/tower/conv_2", t, c7, 192, 7, 1)
    t = b.conv(name + "/tower_1/conv", x, 768, c7, 1, 1)
    t = b.conv(name + "/tower_1/conv_1", t, c7, c7, 7, 1)
    t = b.conv(name + "/tower_1/conv_2", t, c7, c7, 1, 7)
    t = b.conv(name + "/tower_1/conv_3", t, c7, c7, 7, 1)
    b3 = b.conv(name + "/tower_1/conv_4", t, c7, 192, 1, 7)
    p = b.pool(name + "/tower_2/pool", x, "AvgPool", 3, 1, "SAME")
    b4 = b.conv(name + "/tower_2/conv", p, 768, 192, 1, 1)
    return b.concat(name + "/join", [b1, b2, b3, b4])


def _block_e(b, name, x, cin, pool_op):
    b1 = b.conv(name + "/conv", x, cin, 320, 1, 1)
    t = b.conv(name + "/tower/conv", x, cin, 384, 1, 1)
    b2 = b.concat(name + "/tower/mixed", [b.conv(name + "/tower/mixed/conv", t, 384, 384, 1, 3),
                                          b.conv(name + "/tower/mixed/conv_1", t, 384, 384, 3, 1)])
    t = b.conv(name + "/tower_1/conv", x, cin, 448, 1, 1)
    t = b.conv(name + "/tower_1/conv_1", t, 448, 384, 3, 3)
    b3 = b.concat(name + "/tower_1/mixed", [b.conv(name + "/tower_1/mixed/conv", t, 384, 384, 1, 3),
                                            b.conv(name + "/tower_1/mixed/conv_1", t, 384, 384, 3, 1)])
    p = b.pool(name + "/tower_2/pool", x, pool_op, 3, 1, "SAME")
    b4 = b.conv(name + "/tower_2/conv", p, cin, 192, 1, 1)
    return b.concat(name + "/join", [b1, b2, b3, b4])


@functools.lru_cache(maxsize=None)
def full_graph(seed=0):
    """The 2015 topology: stem, 3 A blocks (256 / 288 / 288), B reduction (17 x 17 x 768), 4 C blocks, D reduction
    (8 x 8 x 1280), 2 E blocks (2048; avg pool, then stride-1 SAME max pool), pool_3, W [2048, 1008]."""
    b = Builder(seed)
    x = b.input_chain(299)
    x = b.conv("conv", x, 3, 32, 3, 3, 2, "VALID")
    x = b.conv("conv_1", x, 32, 32, 3, 3, 1, "VALID")
    x = b.conv("conv_2", x, 32, 64, 3, 3, 1, "SAME")
    x = b.pool("pool", x, "MaxPool", 3, 2, "VALID")
    x = b.conv("conv_3", x, 64, 80, 1, 1, 1, "VALID")
    x = b.conv("conv_4", x, 80, 192, 3, 3, 1, "VALID")
    x = b.pool("pool_1", x, "MaxPool", 3, 2, "VALID")
    c = 192
    for i, pc in enumerate((32, 64, 64)):
        x, c = _block_a(b, "mixed" + ("_%d" % i if i else ""), x, c, pc)
    # B: 288 -> 768 at 17 x 17
    b1 = b.conv("mixed_3/conv", x, 288, 384, 3, 3, 2, "VALID")
    t = b.conv("mixed_3/tower/conv", x, 288, 64, 1, 1)
    t = b.conv("mixed_3/tower/conv_1", t, 64, 96, 3, 3)
    b2 = b.conv("mixed_3/tower/conv_2", t, 96, 96, 3, 3, 2, "VALID")
    b3 = b.pool("mixed_3/pool", x, "MaxPool", 3, 2, "VALID")
    x = b.concat("mixed_3/join", [b1, b2, b3])
    for i, c7 in enumerate((128, 160, 160, 192)):
        x = _block_c(b, "mixed_%d" % (4 + i), x, c7)
    # D: 768 -> 1280 at 8 x 8
    t = b.conv("mixed_8/tower/conv", x, 768, 192, 1, 1)
    b1 = b.conv("mixed_8/tower/conv_1", t, 192, 320, 3, 3, 2, "VALID")
    t = b.conv("mixed_8/tower_1/conv", x, 768, 192, 1, 1)
    t = b.conv("mixed_8/tower_1/conv_1", t, 192, 192, 1, 7)
    t = b.conv("mixed_8/tower_1/conv_2", t, 192, 192, 7, 1)
    b2 = b.conv("mixed_8/tower_1/conv_3", t, 192, 192, 3, 3, 2, "VALID")
    b3 = b.pool("mixed_8/pool", x, "MaxPool", 3, 2, "VALID")
    x = b.concat("mixed_8/join", [b1, b2, b3])
    x = _block_e(b, "mixed_9", x, 1280, "AvgPool")
    x = _block_e(b, "mixed_10", x, 2048, "MaxPool")
    b.head(x, 2048)
    assert b.n_conv == 94
    return b.nodes, graph_bytes(b.nodes)


@functools.lru_cache(maxsize=None)
def narrow_graph(seed=1):
    """Every op and join form of the full graph at few channels: 32 x 32 -> 75 x 75, stem, one A-style block, a
    stride-2 reduction, a 1x7 / 7x1 block, an E-style block with nested concats and a stride-1 SAME max pool."""
    b = Builder(seed)
    x = b.input_chain(75)
    x = b.conv("conv", x, 3, 8, 3, 3, 2, "VALID")             # 37
    x = b.conv("conv_1", x, 8, 8, 3, 3, 1, "SAME")
    x = b.pool("pool", x, "MaxPool", 3, 2, "VALID")           # 18
    b1 = b.conv("mixed/conv", x, 8, 8, 1, 1)
    t = b.conv("mixed/tower/conv", x, 8, 12, 1, 1)
    b2 = b.conv("mixed/tower/conv_1", t, 12, 8, 5, 5)
    p = b.pool("mixed/tower_2/pool", x, "AvgPool", 3, 1, "SAME")
    b3 = b.conv("mixed/tower_2/conv", p, 8, 4, 1, 1)
    x = b.concat("mixed/join", [b1, b2, b3])                  # 20
    r1 = b.conv("mixed_1/conv", x, 20, 16, 3, 3, 2, "VALID")  # 8 ... (18 - 3) / 2 + 1 = 8
    r2 = b.pool("mixed_1/pool", x, "MaxPool", 3, 2, "VALID")
    x = b.concat("mixed_1/join", [r1, r2])                    # 36 at 8 x 8
    t = b.conv("mixed_2/tower/conv", x, 36, 12, 1, 1)
    t = b.conv("mixed_2/tower/conv_1", t, 12, 12, 1, 7)
    c1 = b.conv("mixed_2/tower/conv_2", t, 12, 16, 7, 1)
    t = b.conv("mixed_2/tower_1/conv", x, 36, 16, 1, 1)
    c2 = b.concat("mixed_2/tower_1/mixed", [b.conv("mixed_2/tower_1/mixed/conv", t, 16, 8, 1, 3),
                                            b.conv("mixed_2/tower_1/mixed/conv_1", t, 16, 8, 3, 1)])
    p = b.pool("mixed_2/tower_2/pool", x, "MaxPool", 3, 1, "SAME")
    c3 = b.conv("mixed_2/tower_2/conv", p, 36, 8, 1, 1)
    x = b.concat("mixed_2/join", [c1, c2, c3])                # 40
    b.head(x, 40, classes=24)
    return b.nodes, graph_bytes(b.nodes)


# ---------------------------------------------------------------- fp64 interpreter
def legacy_resize(x, oh, ow, align_corners=False):
    """TF's ResizeBilinear (legacy: src = dst * in / out, no half-pixel offset, upper neighbour clamped).
    x: float64 torch [n, H, W, C]."""
    import torch
    n, H, W, C = x.shape
    sy = (H - 1) / (oh - 1) if align_corners and oh > 1 else H / oh
    sx = (W - 1) / (ow - 1) if align_corners and ow > 1 else W / ow
    fy = torch.arange(oh, dtype=torch.float64) * sy
    fx = torch.arange(ow, dtype=torch.float64) * sx
    y0, x0 = fy.floor().long().clamp(max=H - 1), fx.floor().long().clamp(max=W - 1)
    y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
    ly, lx = (fy - y0)[None, :, None, None], (fx - x0)[None, None, :, None]
    tl, tr = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    bl, br = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    top, bot = tl + (tr - tl) * lx, bl + (br - bl) * lx
    return top + (bot - top) * ly


def _tf_pads(n, k, s, same):
    if not same:
        return (n - k) // s + 1, 0, 0
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return out, tot // 2, tot - tot // 2


def _nchw_pad(x, k, s, same, value=0.0):
    """(x NHWC f64) -> NCHW tensor padded for a TF window with `value`."""
    import torch.nn.functional as F
    _, H, W, _ = x.shape
    _, pt, pb = _tf_pads(H, k[0], s[0], same)
    _, pl, pr = _tf_pads(W, k[1], s[1], same)
    return F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb), value=value), (pt, pb, pl, pr)


def interpret(nodes, images, outputs=("pool_3", "softmax/logits/MatMul")):
    """Evaluate the node list in fp64 for images [n, H, W, 3] (numpy, 0..255) fed at ExpandDims; returns {name: numpy}."""
    import torch
    import torch.nn.functional as F
    by = {n["name"]: n for n in nodes}
    val = {"ExpandDims": torch.as_tensor(np.asarray(images, np.float64))}

    def get(ref):
        return ev(ref.split(":")[0])

    def ev(name):
        if name in val:
            return val[name]
        stack = [name]
        while stack:                      # iterative post-order (deep chains)
            top = stack[-1]
            pend = [i.split(":")[0] for i in by[top]["inputs"] if not i.startswith("^") and i.split(":")[0] not in val]
            if pend:
                stack.extend(pend)
                continue
            stack.pop()
            if top not in val:
                val[top] = compute(by[top])
        return val[name]

    def compute(nd):
        op, a = nd["op"], nd["attr"]
        ins = [val[i.split(":")[0]] for i in nd["inputs"] if not i.startswith("^")]
        if op == "Const":
            return torch.as_tensor(np.asarray(a["value"][1]).astype(np.float64))
        if op in ("Identity", "CheckNumerics"):
            return ins[0]
        if op == "ResizeBilinear":
            return legacy_resize(ins[0], int(ins[1][0]), int(ins[1][1]), a.get("align_corners", False))
        if op == "Sub":
            return ins[0] - ins[1]
        if op == "Mul":
            return ins[0] * ins[1]
        if op == "Add":
            return ins[0] + ins[1]
        if op == "RealDiv":
            return ins[0] / ins[1]
        if op == "Conv2D":
            w = ins[1]
            k, s = (w.shape[0], w.shape[1]), (a["strides"][1], a["strides"][2])
            xp, _ = _nchw_pad(ins[0], k, s, a["padding"] == "SAME")
            return F.conv2d(xp, w.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)
        if op == "BatchNormWithGlobalNormalization":
            x, m, v, beta, gamma = ins
            y = (x - m) / torch.sqrt(v + a["variance_epsilon"])
            if a["scale_after_normalization"]:
                y = y * gamma
            return y + beta
        if op == "Relu":
            return torch.clamp(ins[0], min=0)
        if op in ("MaxPool", "AvgPool"):
            k, s = (a["ksize"][1], a["ksize"][2]), (a["strides"][1], a["strides"][2])
            same = a["padding"] == "SAME"
            x = ins[0]
            if op == "MaxPool":
                xp, _ = _nchw_pad(x, k, s, same, value=-float("inf"))
                return F.max_pool2d(xp, k, s).permute(0, 2, 3, 1)
            xp, _ = _nchw_pad(x, k, s, same)
            ones, _ = _nchw_pad(torch.ones_like(x[..., :1]), k, s, same)
            return (F.avg_pool2d(xp, k, s) / F.avg_pool2d(ones, k, s)).permute(0, 2, 3, 1)
        if op == "Concat":
            return torch.cat(ins[1:], int(ins[0]))
        if op == "ConcatV2":
            return torch.cat(ins[:-1], int(ins[-1]))
        if op == "Reshape":
            return ins[0].reshape([int(d) for d in ins[1]])
        if op == "Squeeze":
            return ins[0].squeeze()
        if op == "MatMul":
            return ins[0] @ ins[1]
        if op == "BiasAdd":
            return ins[0] + ins[1]
        if op == "Softmax":
            return torch.softmax(ins[0], -1)
        raise ValueError("interpreter: op %s" % op)

    return {o: ev(o).numpy() for o in outputs}


def reference_outputs(nodes, images):
    """(pool_3 [n, C], bias-free logits, probabilities) in fp64 -- the reference's softmax(squeeze(pool_3) . W)."""
    out = interpret(nodes, images)
    pool3 = out["pool_3"].reshape(len(images), -1)
    logits = out["softmax/logits/MatMul"]
    e = np.exp(logits - logits.max(1, keepdims=True))
    return pool3, logits, e / e.sum(1, keepdims=True)


def images(n, size=32, seed=0):
    """Smooth random images [n, size, size, 3] in 0..255."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 255, (n, 4, 4, 3))
    import torch
    x = legacy_resize(torch.as_tensor(base), size, size).numpy()
    return np.clip(x + rng.normal(0, 20, x.shape), 0, 255).astype(np.float32)
