"""CPU: the definitions behind --health_every -- the numpy restatement's identities, `below` on hand-made histograms, the
report schedule `due` over every phase, flag validation, the record's JSON round trip and summary line, and that the new
entry points are declared in the header, the ctypes table and the Makefile."""
import math
import os
import re

import numpy as np
import pytest

import health_ref as R
from conftest import ROOT
from otgan_amd.utils import health


def _mixed(rng, n):
    x = rng.standard_normal(n).astype(np.float32) * np.float32(2.0) ** rng.integers(-30, 30, n).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -3e-45, np.finfo(np.float32).max], np.float32)
    at = rng.integers(0, n, min(n, 3 * len(special)))
    x[at] = special[np.arange(len(at)) % len(special)]
    return x


@pytest.mark.parametrize("n", [0, 1, 5, 257, 5000])
def test_reference_identities(n):
    rng = np.random.default_rng(n)
    x, ref = _mixed(rng, n), _mixed(rng, n)
    out, hist = R.tensor_health(x, ref)
    assert hist.sum() + out[4] + out[5] == n
    assert hist[255] == 0 and hist.shape == (256,)
    assert out[5] == np.count_nonzero(~np.isfinite(x)) and out[4] == np.count_nonzero(x == 0)
    fin = x[np.isfinite(x)].astype(np.float64)
    assert out[0] == pytest.approx(float((fin * fin).sum()), rel=1e-12) and out[1] == (np.abs(fin).max() if fin.size else 0.0)
    alone, hist2 = R.tensor_health(x)
    assert np.array_equal(alone[[0, 1, 4, 5]], out[[0, 1, 4, 5]]) and alone[2] == alone[3] == 0 and np.array_equal(hist, hist2)
    # the bucket is the biased exponent: 1.0 -> 127, the largest float -> 254, denormals -> 0
    assert R.tensor_health(np.float32([1.0, 1.5, np.finfo(np.float32).max, 1e-40]))[1].nonzero()[0].tolist() == [0, 127, 254]


def test_below_on_hand_made_histograms():
    h = np.zeros(256, np.int64)
    assert health.below(h, 11) == R.below(h, 11) == 0.0
    h[130] = 10
    assert health.below(h, 11) == 0.0 and health.below(h, 0) == 1.0
    h[119], h[120], h[108], h[0] = 3, 5, 2, 1          # 11, 10, 22 and 130 below the top
    assert health.below(h, 11) == R.below(h, 11) == 6 / 21
    assert health.below(h, 22) == R.below(h, 22) == 3 / 21
    assert health.below(h, 10) == 11 / 21 and health.below(h, 131) == 0.0
    rng = np.random.default_rng(0)
    for _ in range(50):
        h = rng.integers(0, 4, 256) * (rng.random(256) < 0.1)
        for bits in (1, 11, 22, 200):
            assert health.below(h, bits) == R.below(h, bits)
    assert (health.PIECE_BITS, health.OPERAND_BITS) == (11, 22)


@pytest.mark.parametrize("every", [1, 2, 7, 100])
@pytest.mark.parametrize("period", [2, 6])
def test_due_over_every_phase(every, period):
    steps = 4 * every * period + 3
    got = [s for s in range(steps) if health.due(s, every, period)]
    assert got == R.reported(steps, every, period)
    # every report window -- a multiple of `every` and its partner -- holds exactly one step of each kind, and the partner
    # is the FIRST later step of the other kind; the multiples land on every phase of the period
    phases = set()
    for a in range(0, steps - period, every):
        p = R.partner(a, period)
        phases.add(a % period)
        assert health.due(a, every, period) and health.due(p, every, period)
        assert sorted([R.kind(a, period), R.kind(p, period)]) == ["disc", "gen"]
        assert all(R.kind(s, period) == R.kind(a, period) for s in range(a, p))
    assert phases == {(k * every) % period for k in range(period)}
    # nothing else is reported: a reported step that is no multiple is the partner of the multiple before it
    for s in got:
        assert s % every == 0 or s == R.partner(s - s % every, period)
    assert not any(health.due(s, 0, period) for s in range(20))
    assert health.kind_of(0, period) == "disc" and health.kind_of(1, period) == "gen"


def test_flag_validation():
    from otgan_amd import train, trainer
    assert train.build_parser().parse_args([]).health_every == 0 == trainer.default_args().health_every
    assert train.build_parser().parse_args(["--health_every", "5"]).health_every == 5
    for bad in (-1, -100, 1.5):
        with pytest.raises(ValueError, match="health_every"):
            health.check_every(bad)
    assert health.check_every(0) == 0 and health.check_every(3) == 3
    # train.main refuses before it touches a device or the data
    with pytest.raises(ValueError, match="health_every"):
        train.main(["--health_every", "-2", "--synthetic", "--data_dir", "/nonexistent"])


def _record(kind, step, nonfinite=False):
    rng = np.random.default_rng(step)
    names = ["net/a/V", "net/a/g", "net/b"]
    grads = [rng.standard_normal(n).astype(np.float32) * np.float32(s) for n, s in ((40, 1.0), (3, 1e-9), (7, 1e3))]
    grads[1][0] = 0.0
    if nonfinite:
        grads[2][3] = np.nan
    before = [rng.standard_normal(g.size).astype(np.float32) for g in grads]
    after = [b - np.float32(1e-3) * np.sign(g) for b, g in zip(before, grads)]
    go = [R.tensor_health(g) for g in grads]
    po = None if nonfinite else np.stack([R.tensor_health(a, b)[0] for a, b in zip(after, before)])
    marg = np.array([[1e-16, 1e-17, 5e-2 / (p + 1), 1e-2 / (p + 1)] for p in range(6)])
    rec = health.collect(step, kind, names, np.stack([o for o, _ in go]), np.stack([h for _, h in go]), po, distance=0.25,
                         entropy=float("nan"), sinkhorn=health.sinkhorn_block(marg, 100, 500.0, health.TWO_BATCH_PROBLEMS), epoch=3)
    return rec, names, grads, before, after


def test_collect_against_the_restatement():
    rec, names, grads, before, after = _record("gen", 7)
    want = R.record(7, "gen", names, grads, before, after)
    assert set(rec) == {"step", "epoch", "kind", "distance", "entropy", "net", "grad_norm", "param_norm", "update_norm", "update_ratio",
                        "grad_nonfinite", "grad_below_11", "grad_below_22", "vars", "sinkhorn"}
    assert rec["net"] == "generator" and rec["kind"] == "gen" and rec["step"] == 7 and rec["epoch"] == 3
    for k in ("grad_norm", "param_norm", "update_norm", "update_ratio", "grad_below_11", "grad_below_22", "grad_nonfinite"):
        assert rec[k] == pytest.approx(want[k], rel=1e-15), k
    assert list(rec["vars"]) == names
    for name in names:
        v, w = rec["vars"][name], want["vars"][name]
        assert set(v) == {"n", "grad_norm", "grad_amax", "grad_zero", "grad_nonfinite", "grad_below_11", "grad_below_22",
                          "param_norm", "param_amax", "update_norm", "update_amax"}
        assert {k: v[k] for k in w} == w
    assert rec["vars"]["net/a/g"]["grad_zero"] == 1 and rec["vars"]["net/a/g"]["n"] == 3
    assert rec["update_ratio"] == rec["update_norm"] / rec["param_norm"]
    # the variables differ by 30 bits: the small one lies below the 22 bits of the large one only in its own histogram
    assert rec["grad_below_22"] == want["grad_below_22"]
    assert rec["sinkhorn"]["problems"] == list(health.TWO_BATCH_PROBLEMS) and rec["sinkhorn"]["iters"] == 100
    bad, *_ = _record("disc", 6, nonfinite=True)
    assert bad["net"] == "discriminator" and bad["grad_nonfinite"] == 1 and bad["param_norm"] is None and bad["update_ratio"] is None
    assert health.nonfinite_variables(bad) == ["net/b"] and math.isfinite(bad["grad_norm"])


def test_json_round_trip_and_summary_line(tmp_path):
    gen, disc = _record("gen", 7)[0], _record("disc", 6)[0]
    path = str(tmp_path / "health.jsonl")
    health.append(path, disc)
    health.append(path, gen)
    back = health.read(path)
    assert len(back) == 2 and open(path).read().count("\n") == 2
    for rec, got in zip((disc, gen), back):
        want = dict(rec, entropy=None)                 # NaN is written as null: the file is strict JSON
        assert got == want
    assert "NaN" not in open(path).read()
    line = health.summary_line({"gen": gen, "disc": disc})
    assert re.fullmatch(r"health: \|g\| gen \S+ disc \S+, update/param gen \S+ disc \S+, below 22 bits gen \S+ disc \S+, "
                        r"Sinkhorn column error max \S+ mean \S+ \(L = 100\)", line), line
    assert "%.3e" % gen["grad_norm"] in line and "%.3e" % disc["update_ratio"] in line and "max 5.000e-02" in line
    # one kind only (a run shorter than a pair), and no Sinkhorn
    alone = health.summary_line({"gen": dict(gen, sinkhorn=None), "disc": None})
    assert "disc n/a" in alone and alone.endswith("Sinkhorn column error n/a")


def test_symbols_are_declared():
    from otgan_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "otgan_layers.h")).read()
    names = ("otgan_tensor_health_f32", "otgan_tensor_health_workspace_bytes", "otgan_plan_marginals_f32",
             "otgan_plan_marginals_workspace_bytes")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    assert "health.hip" in open(os.path.join(ROOT, "ot-gan_amd", "csrc", "Makefile")).read()
    assert int(re.search(r"#define OTGAN_HEALTH_CHUNK (\d+)", header).group(1)) == ops.HEALTH_CHUNK
    assert int(re.search(r"#define OTGAN_HEALTH_MAX_SEGMENTS (\d+)", header).group(1)) == ops.HEALTH_MAX_SEGMENTS
    import torch
    with pytest.raises(_lib.OtganError):
        ops.tensor_health([torch.zeros(4)])
    with pytest.raises(_lib.OtganError):
        ops.plan_marginals(torch.ones(2, 3, 3))
