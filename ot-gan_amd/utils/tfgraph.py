"""Reader of TensorFlow GraphDef files -- the 2015 Inception graph `classify_image_graph_def.pb` of the reference's
evaluation (utils/inception.py:55-93) -- without TensorFlow and without the protobuf runtime: the wire format
(varints, length-delimited fields, packed and unpacked repeated scalars) decoded directly.

Field numbers are TensorFlow's public schema (graph.proto, node_def.proto, attr_value.proto, tensor.proto,
tensor_shape.proto, types.proto):
    GraphDef          node = 1, versions = 4
    NodeDef           name = 1, op = 2, input = 3 (repeated), device = 4, attr = 5 (map: key = 1, value = 2)
    AttrValue         list = 1, s = 2, i = 3, f = 4, b = 5, type = 6, shape = 7, tensor = 8
    AttrValue.List    s = 2, i = 3, f = 4, b = 5, type = 6, shape = 7, tensor = 8
    TensorProto       dtype = 1, tensor_shape = 2, tensor_content = 4, float_val = 5, int_val = 7
    TensorShapeProto  dim = 2; Dim: size = 1
    DataType          FLOAT = 1, INT32 = 3
"""
import os
import struct
import tarfile

import numpy as np

DT_FLOAT, DT_INT32 = 1, 3
GRAPH_FILE = "classify_image_graph_def.pb"


class Node:
    __slots__ = ("name", "op", "inputs", "device", "attr")

    def __init__(self):
        self.name, self.op, self.inputs, self.device, self.attr = "", "", [], "", {}

    def __repr__(self):
        return "Node(%r, %r, %r)" % (self.name, self.op, self.inputs)


def _varint(buf, pos):
    out = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        out |= (b & 0x7F) << shift
        if b < 0x80:
            return out, pos
        shift += 7


def _signed64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def fields(buf):
    """(field number, wire type, value) of every field of one message: value = int (varint, fixed32/64 as raw bits)
    or a memoryview (length-delimited)."""
    buf = memoryview(buf)
    pos, end = 0, len(buf)
    while pos < end:
        key, pos = _varint(buf, pos)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(buf, pos)
        elif wt == 1:
            v = struct.unpack_from("<Q", buf, pos)[0]
            pos += 8
        elif wt == 2:
            n, pos = _varint(buf, pos)
            v = buf[pos:pos + n]
            pos += n
        elif wt == 5:
            v = struct.unpack_from("<I", buf, pos)[0]
            pos += 4
        else:
            raise ValueError("GraphDef: unsupported wire type %d (field %d)" % (wt, num))
        yield num, wt, v


def _floats(wt, v):
    if wt == 5:
        return [struct.unpack("<f", struct.pack("<I", v))[0]]
    if wt == 2:
        return list(np.frombuffer(bytes(v), "<f4").astype(np.float64))
    raise ValueError("GraphDef: float field with wire type %d" % wt)


def _ints(wt, v):
    if wt == 0:
        return [_signed64(v)]
    if wt == 2:
        out, pos, b = [], 0, v
        while pos < len(b):
            x, pos = _varint(b, pos)
            out.append(_signed64(x))
        return out
    raise ValueError("GraphDef: integer field with wire type %d" % wt)


def parse_shape(buf):
    dims = []
    for num, _, v in fields(buf):
        if num == 2:
            size = 0
            for n2, w2, v2 in fields(v):
                if n2 == 1:
                    size = _signed64(v2)
            dims.append(size)
    return tuple(dims)


def parse_tensor(buf):
    """TensorProto -> numpy array (float32 / int32).  A single float_val / int_val with a larger shape fills the
    shape, as TensorFlow does."""
    dtype, shape, content, fv, iv = DT_FLOAT, (), None, [], []
    for num, wt, v in fields(buf):
        if num == 1:
            dtype = v
        elif num == 2:
            shape = parse_shape(v)
        elif num == 4:
            content = bytes(v)
        elif num == 5:
            fv += _floats(wt, v)
        elif num == 7:
            iv += _ints(wt, v)
    if dtype == DT_FLOAT:
        np_t, vals = np.float32, fv
    elif dtype == DT_INT32:
        np_t, vals = np.int32, iv
    else:
        raise ValueError("GraphDef: constant of dtype %d (only FLOAT = 1 and INT32 = 3 are read)" % dtype)
    count = int(np.prod(shape)) if shape else 1
    if content is not None:
        arr = np.frombuffer(content, np.dtype(np_t).newbyteorder("<")).astype(np_t)
    elif len(vals) == count:
        arr = np.asarray(vals, np_t)
    elif len(vals) == 1 or (not vals and count):
        arr = np.full(count, vals[0] if vals else 0, np_t)
    else:
        raise ValueError("GraphDef: constant with %d values for shape %s" % (len(vals), shape))
    if arr.size != count:
        raise ValueError("GraphDef: tensor_content of %d values for shape %s" % (arr.size, shape))
    return arr.reshape(shape)


def parse_attr(buf):
    """AttrValue -> python value: bytes / int / float / bool / ('type', n) / ('shape', dims) / ndarray / list."""
    for num, wt, v in fields(buf):
        if num == 1:
            return _parse_list(v)
        if num == 2:
            return bytes(v)
        if num == 3:
            return _signed64(v)
        if num == 4:
            return _floats(wt, v)[0]
        if num == 5:
            return bool(v)
        if num == 6:
            return ("type", v)
        if num == 7:
            return ("shape", parse_shape(v))
        if num == 8:
            return parse_tensor(v)
    return None


def _parse_list(buf):
    out = []
    for num, wt, v in fields(buf):
        if num == 2:
            out.append(bytes(v))
        elif num == 3:
            out += _ints(wt, v)
        elif num == 4:
            out += _floats(wt, v)
        elif num == 5:
            out += [bool(x) for x in _ints(wt, v)]
        elif num == 6:
            out += [("type", x) for x in _ints(wt, v)]
        elif num == 7:
            out.append(("shape", parse_shape(v)))
        elif num == 8:
            out.append(parse_tensor(v))
    return out


def parse_node(buf):
    n = Node()
    for num, wt, v in fields(buf):
        if num == 1:
            n.name = bytes(v).decode()
        elif num == 2:
            n.op = bytes(v).decode()
        elif num == 3:
            n.inputs.append(bytes(v).decode())
        elif num == 4:
            n.device = bytes(v).decode()
        elif num == 5:
            key, val = None, None
            for n2, w2, v2 in fields(v):
                if n2 == 1:
                    key = bytes(v2).decode()
                elif n2 == 2:
                    val = parse_attr(v2)
            n.attr[key] = val
    return n


def parse_graph(data):
    """GraphDef bytes -> list of Node in file order."""
    return [parse_node(v) for num, wt, v in fields(data) if num == 1]


def read_graph_bytes(path):
    """The graph file's bytes from the .pb itself, the reference's .tgz (inception-2015-12-05.tgz), or a directory
    holding the .pb (the reference unpacks into /tmp/imagenet)."""
    if os.path.isdir(path):
        return read_graph_bytes(os.path.join(path, GRAPH_FILE))
    with open(path, "rb") as f:
        head = f.read(2)
    if head == b"\x1f\x8b" or tarfile.is_tarfile(path):
        with tarfile.open(path, "r:*") as tf:
            for m in tf.getmembers():
                if os.path.basename(m.name) == GRAPH_FILE:
                    return tf.extractfile(m).read()
        raise ValueError("%s: archive without %s" % (path, GRAPH_FILE))
    with open(path, "rb") as f:
        return f.read()


def load_graph(path_or_bytes):
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else read_graph_bytes(path_or_bytes)
    return parse_graph(data)

