"""The Inception graph reader (utils/tfgraph.py) and its lowering (utils/inception_net.py) on the host: wire-format round
trip, the lowered plan of the full 2015 topology, the legacy resize of the fp64 interpreter, loud failures."""
import os

import numpy as np
import pytest

import inception_graphs as G
from otgan_amd.utils import inception_net, tfgraph


def test_reader_round_trip_nodes_inputs_and_attrs():
    nodes = [
        {"name": "a", "op": "Const", "inputs": [], "attr": {"value": ("tensor", np.arange(6, dtype=np.float32).reshape(2, 3)),
                                                            "dtype": ("type", 1)}},
        {"name": "b/c", "op": "Conv2D", "inputs": ["a", "a:0", "^ctl"],
         "attr": {"strides": [1, 2, 2, 1], "padding": "SAME", "f": 0.25, "flag": True, "neg": -3,
                  "shape": ("shape", (4, -1, 7)), "T": ("type", 3), "fl": [0.5, -1.5], "sl": [b"x", b"yz"]}},
    ]
    got = tfgraph.parse_graph(G.graph_bytes(nodes))
    assert [n.name for n in got] == ["a", "b/c"] and [n.op for n in got] == ["Const", "Conv2D"]
    assert got[1].inputs == ["a", "a:0", "^ctl"]
    at = got[1].attr
    assert at["strides"] == [1, 2, 2, 1] and at["padding"] == b"SAME" and at["f"] == 0.25 and at["flag"] is True
    assert at["neg"] == -3 and at["shape"] == ("shape", (4, -1, 7)) and at["T"] == ("type", 3)
    assert at["fl"] == [0.5, -1.5] and at["sl"] == [b"x", b"yz"]
    np.testing.assert_array_equal(got[0].attr["value"], np.arange(6, dtype=np.float32).reshape(2, 3))


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
def test_constants_content_values_and_broadcast_fill(dtype):
    arr = (np.arange(12).reshape(3, 4) * (0.5 if dtype == np.float32 else 1) - 3).astype(dtype)
    a = tfgraph.parse_tensor(G.tensor_proto(arr, use_content=True))
    b = tfgraph.parse_tensor(G.tensor_proto(arr, use_content=False))
    assert a.dtype == b.dtype == dtype
    np.testing.assert_array_equal(a, arr)
    np.testing.assert_array_equal(b, arr)
    fill = tfgraph.parse_tensor(G.tensor_proto(np.zeros((2, 5), dtype), fill=(1.25 if dtype == np.float32 else 7)))
    np.testing.assert_array_equal(fill, np.full((2, 5), 1.25 if dtype == np.float32 else 7, dtype))
    scalar = tfgraph.parse_tensor(G.tensor_proto(np.array(128.0, np.float32)))
    assert scalar.shape == () and scalar == 128.0


def test_reader_agrees_with_the_official_protobuf_runtime():
    """Messages of TensorFlow's schema, built from a hand-made descriptor, encoded by the official runtime."""
    pb = pytest.importorskip("google.protobuf")
    del pb
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="tfmini.proto", package="tfmini", syntax="proto3")

    def msg(name, fields, nested=()):
        m = fd.message_type.add(name=name)
        for fname, num, typ, label, tname in fields:
            f = m.field.add(name=fname, number=num, type=typ, label=label)
            if tname:
                f.type_name = tname
        for n in nested:
            m.nested_type.add().CopyFrom(n)
        return m
    OPT, REP = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    dim = descriptor_pb2.DescriptorProto(name="Dim")
    dim.field.add(name="size", number=1, type=F.TYPE_INT64, label=OPT)
    msg("TensorShapeProto", [("dim", 2, F.TYPE_MESSAGE, REP, ".tfmini.TensorShapeProto.Dim")], [dim])
    msg("TensorProto", [("dtype", 1, F.TYPE_INT32, OPT, None),
                        ("tensor_shape", 2, F.TYPE_MESSAGE, OPT, ".tfmini.TensorShapeProto"),
                        ("tensor_content", 4, F.TYPE_BYTES, OPT, None),
                        ("float_val", 5, F.TYPE_FLOAT, REP, None), ("int_val", 7, F.TYPE_INT32, REP, None)])
    lst = descriptor_pb2.DescriptorProto(name="ListValue")
    for fname, num, typ in (("s", 2, F.TYPE_BYTES), ("i", 3, F.TYPE_INT64), ("f", 4, F.TYPE_FLOAT), ("b", 5, F.TYPE_BOOL)):
        lst.field.add(name=fname, number=num, type=typ, label=REP)
    msg("AttrValue", [("list", 1, F.TYPE_MESSAGE, OPT, ".tfmini.AttrValue.ListValue"), ("s", 2, F.TYPE_BYTES, OPT, None),
                      ("i", 3, F.TYPE_INT64, OPT, None), ("f", 4, F.TYPE_FLOAT, OPT, None), ("b", 5, F.TYPE_BOOL, OPT, None),
                      ("type", 6, F.TYPE_INT32, OPT, None), ("shape", 7, F.TYPE_MESSAGE, OPT, ".tfmini.TensorShapeProto"),
                      ("tensor", 8, F.TYPE_MESSAGE, OPT, ".tfmini.TensorProto")], [lst])
    entry = descriptor_pb2.DescriptorProto(name="AttrEntry")
    entry.options.map_entry = True
    entry.field.add(name="key", number=1, type=F.TYPE_STRING, label=OPT)
    entry.field.add(name="value", number=2, type=F.TYPE_MESSAGE, label=OPT, type_name=".tfmini.AttrValue")
    msg("NodeDef", [("name", 1, F.TYPE_STRING, OPT, None), ("op", 2, F.TYPE_STRING, OPT, None),
                    ("input", 3, F.TYPE_STRING, REP, None), ("device", 4, F.TYPE_STRING, OPT, None),
                    ("attr", 5, F.TYPE_MESSAGE, REP, ".tfmini.NodeDef.AttrEntry")], [entry])
    msg("GraphDef", [("node", 1, F.TYPE_MESSAGE, REP, ".tfmini.NodeDef")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    get = message_factory.GetMessageClass if hasattr(message_factory, "GetMessageClass") else \
        (lambda d: message_factory.MessageFactory(pool).GetPrototype(d))
    GraphDef = get(pool.FindMessageTypeByName("tfmini.GraphDef"))
    g = GraphDef()
    n = g.node.add(name="conv/Conv2D", op="Conv2D", device="/cpu:0")
    n.input.extend(["x", "w:0"])
    n.attr["strides"].list.i.extend([1, 2, 2, 1])
    n.attr["padding"].s = b"VALID"
    n.attr["eps"].f = 0.001
    n.attr["flag"].b = True
    n.attr["T"].type = 1
    t = n.attr["value"].tensor
    t.dtype = 1
    t.tensor_shape.dim.add(size=2)
    t.tensor_shape.dim.add(size=3)
    t.float_val.extend([1.5, -2.0, 3.0, 0.25, 8.0, -1.0])
    t2 = g.node.add(name="k", op="Const").attr["value"].tensor
    t2.dtype = 3
    t2.tensor_shape.dim.add(size=4)
    t2.int_val.extend([7])
    got = tfgraph.parse_graph(g.SerializeToString())
    assert got[0].name == "conv/Conv2D" and got[0].device == "/cpu:0" and got[0].inputs == ["x", "w:0"]
    a = got[0].attr
    assert a["strides"] == [1, 2, 2, 1] and a["padding"] == b"VALID" and a["flag"] is True and a["T"] == ("type", 1)
    assert a["eps"] == pytest.approx(0.001, rel=1e-7)
    np.testing.assert_array_equal(a["value"], np.array([[1.5, -2.0, 3.0], [0.25, 8.0, -1.0]], np.float32))
    np.testing.assert_array_equal(got[1].attr["value"], np.full(4, 7, np.int32))


def test_lowering_of_the_full_2015_topology():
    nodes, data = G.full_graph()
    plan = inception_net.lower(tfgraph.parse_graph(data))
    convs = plan.convs()
    assert len(convs) == 94
    kinds = {s[0] for s in plan.steps}
    assert kinds == {"resize", "conv", "pool", "head"}        # no concat, no batch norm, no relu, no affine step left
    assert all(s[7] for s in convs)                           # every ReLU fused
    grids = {(s[2].H, s[2].C) for s in convs}
    assert {35, 17, 8} <= {h for h, _ in grids}
    roots = {(t.H, t.C) for t in plan.buffers}
    for g in [(35, 288), (17, 768), (8, 1280), (8, 2048)]:
        assert g in roots, g
    assert plan.steps[0][:5][2:4] == (299, 299)
    assert plan.steps[0][5] == pytest.approx(1 / 128) and plan.steps[0][6] == pytest.approx(-1.0)
    assert plan.steps[-1][0] == "head" and plan.steps[-1][2] == 64 and plan.steps[-1][1].C == 2048
    # bias-free logits: the MatMul's own weights, not the graph's softmax (bias) output
    by = {n["name"]: n for n in nodes}
    np.testing.assert_array_equal(plan.weights, by["softmax/weights"]["attr"]["value"][1].astype(np.float64))
    assert plan.flops_per_image() == pytest.approx(11.43e9, rel=0.01)       # ~5.7 GMAC per image


def test_lowering_folds_batch_norm_in_fp64():
    nodes, data = G.narrow_graph()
    plan = inception_net.lower(tfgraph.parse_graph(data))
    by = {n["name"]: n for n in nodes}
    w = by["conv/conv2d_params"]["attr"]["value"][1].astype(np.float64)
    m, v, beta = (by["conv/batchnorm/" + k]["attr"]["value"][1].astype(np.float64) for k in ("moving_mean", "moving_variance", "beta"))
    eps = float(np.float32(0.001))
    s = plan.convs()[0]
    np.testing.assert_allclose(s[3], w / np.sqrt(v + eps), rtol=1e-12)
    np.testing.assert_allclose(s[4], -m / np.sqrt(v + eps) + beta, rtol=1e-12)


def test_unknown_op_fails_loudly_with_its_name():
    nodes, _ = G.narrow_graph()
    bad = [dict(n) for n in nodes]
    for n in bad:
        if n["name"] == "conv_1":
            n["op"] = "Elu"
    with pytest.raises(ValueError, match=r"Elu.*conv_1"):
        inception_net.lower(tfgraph.parse_graph(G.graph_bytes(bad)))


def test_legacy_resize_by_hand():
    import torch
    x = torch.tensor([[0.0], [10.0]], dtype=torch.float64).reshape(1, 2, 1, 1).expand(1, 2, 2, 1).contiguous()
    # 2 -> 3: src = dst * 2/3 = 0, 2/3, 4/3 -> 0, 6.667, 10 (upper neighbour clamped)
    got = G.legacy_resize(x, 3, 2)[0, :, 0, 0].numpy()
    np.testing.assert_allclose(got, [0.0, 20.0 / 3.0, 10.0], rtol=1e-15)
    x = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64).reshape(1, 3, 1, 1)
    # 3 -> 5: src = 0, 0.6, 1.2, 1.8, 2.4 -> 1, 1.6, 2.4, 3.6, 4
    got = G.legacy_resize(x, 5, 1)[0, :, 0, 0].numpy()
    np.testing.assert_allclose(got, [1.0, 1.6, 2.4, 3.6, 4.0], rtol=1e-15)


def test_graph_file_forms_and_load_classifier_errors(tmp_path):
    import tarfile
    _, data = G.narrow_graph()
    pb = tmp_path / "d" / tfgraph.GRAPH_FILE
    pb.parent.mkdir()
    pb.write_bytes(data)
    tgz = tmp_path / "inception-2015-12-05.tgz"
    with tarfile.open(tgz, "w:gz") as tf:
        tf.add(pb, arcname="inception/" + tfgraph.GRAPH_FILE)
    for p in (pb, tgz, pb.parent):
        assert tfgraph.read_graph_bytes(str(p)) == data
    junk = tmp_path / "junk.bin"
    junk.write_bytes(b"\x07not a graph")
    from otgan_amd.utils.inception import load_classifier
    with pytest.raises(ValueError, match="TorchScript.*classify_image_graph_def"):
        load_classifier(str(junk))
    assert os.path.exists(pb)
