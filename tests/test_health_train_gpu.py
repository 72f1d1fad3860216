"""--health_every in training, on the GPU: training with the reports against training without them, bit for bit, eagerly and
under step graphs; the record of a step against tests/health_ref.py on the gradients of a gradient-only pass over the same data
and latents and on the parameters before and after; train.main's file and summary line; and non-finite gradients.

DCGAN and DenseNet at 32 x 32, batch_size 4, nr_gpu 2, 10 Sinkhorn sweeps, nr_gen_per_disc 2 (a period of 3 steps).

Schedules.  `health_every` 2 over 3 periods plus 2 steps reports every step but step 5: with step graphs on, the graphs' eager
warm-up never ends inside those 11 steps and every step is eager.  The second schedule, `health_every` 7 over 28 steps, is the
one under which all three graph kinds are captured (steps 10 - 12) and replayed after reported eager steps (14 / 15 and
21 / 22, replays 16 - 20 and 25 - 27); the test asserts that they were.

Bars.  Counts, maxima, histogram shares and n: equal.  A norm: its square within (n + 3) 2^-53 of the square of the
restatement's -- (n + 1) 2^-53 for an fp64 sum of n exact non-negative terms in any order (tests/test_health_gpu.py) and one
rounding each for the square root and for squaring it again here.  The Sinkhorn block: equal to the staged chain on the
features the step handed to its matching."""
import json
import os

import pytest
import torch

import health_ref as R
from test_step_graph_gpu import _same
from test_step_graph_interleave_gpu import Probe, _noise
from otgan_amd import ops
from otgan_amd.utils import health, matching

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NGD, ITERS, LAM = 2, 10, 100.0


def _model(model, graph, every):
    from otgan_amd.trainer import OTGAN, default_args
    args = default_args(model=model, batch_size=4, nr_gpu=2, sinkhorn_lambda=LAM, nr_sinkhorn_iter=ITERS, nr_gen_per_disc=NGD,
                        seed=3, step_graph=graph, health_every=every)
    return OTGAN(args, DEV)


def _data(m, k=4):
    g = torch.Generator().manual_seed(11)
    return [(torch.rand(m.nb, 32, 32, 3, generator=g) * 2 - 1).to(DEV) for _ in range(k)]


def _trajectory(model, graph, every, steps, probe=None):
    m = _model(model, graph, every)
    assert (m.graphs is not None) == bool(graph)
    xs = _data(m)
    torch.manual_seed(7)
    dists, kinds, reported = [], [], []
    for i in range(steps):
        if probe is not None:
            probe.i = i
        r = m.step(xs[i % len(xs)])
        dists.append(r["distance"].clone())
        kinds.append(r["kind"])
        if "health" in r:
            reported.append(i)
            assert r["health"]["step"] == i and r["health"]["kind"] == r["kind"]
    sd = m.state_dict(full=True)
    res = {"state": {k: v.clone() for k, v in sd.items() if torch.is_tensor(v)}, "opt": sd["__optim__"], "ema": sd["__ema__"],
           "dists": torch.stack(dists).cpu(), "kinds": kinds, "t": (m.gen_optimizer.t, m.disc_optimizer.t, m.step_counter),
           "reported": reported, "captured": sorted(m.graphs.graphs) if m.graphs is not None else [],
           "dead": m.graphs.dead if m.graphs is not None else None}
    m.close()
    return res


@pytest.mark.parametrize("every,steps", [(2, 3 * (NGD + 1) + 2), (7, 28)])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("model", ["dcgan", "densenet"])
def test_training_unchanged(model, graph, every, steps):
    plain = _trajectory(model, graph, 0, steps)
    probe = Probe()
    with pytest.MonkeyPatch.context() as mp:
        probe.install(mp, structure=False)
        with_health = _trajectory(model, graph, every, steps, probe)
    assert plain["reported"] == [] and with_health["reported"] == R.reported(steps, every, NGD + 1)
    assert plain["dead"] is None and with_health["dead"] is None
    if graph and every == 7:
        assert with_health["captured"] == ["disc", "gen", "gen1"]
        after = {k for i, k in probe.replays if i > 15}           # behind the reported eager steps 14 and 15
        assert after == {"disc", "gen", "gen1"}, probe.replays
        assert not any(i in with_health["reported"] for i, _ in probe.replays)        # a reported step is never a replay
    _same(plain, with_health)


def _staged_marginals(f_gen, f_dat):
    N = f_gen.shape[0] // 2
    a1, a2, b1, b2 = f_gen[:N], f_gen[N:], f_dat[:N], f_dat[N:]
    K = matching.cost_log_kernels([a1, b2, a1, a1, a2, a2], [a2, b1, b1, b2, b1, b2], LAM)      # a1a2 b2b1 a1b1 a1b2 a2b1 a2b2
    return ops.plan_marginals(matching.sinkhorn_plans(K, LAM, ITERS)).cpu().numpy()


@pytest.mark.parametrize("model", ["dcgan", "densenet"])
def test_the_record(model, monkeypatch):
    from otgan_amd import trainer
    # the networks' variables are module-level templates: two trainers of one model cannot live side by side, so the twin is
    # the same trainer, put back to the state in front of the step after its gradient-only pass
    a = _model(model, False, 1)
    xs = _data(a)
    seen = []
    real_match = trainer.OTGAN._match

    def match(self, f_gen, f_dat, *args, **kw):
        seen.append((f_gen.detach().clone(), f_dat.detach().clone()))
        return real_match(self, f_gen, f_dat, *args, **kw)
    monkeypatch.setattr(trainer.OTGAN, "_match", match)
    worst = 0.0
    for i in range(NGD + 1):                                 # a critic step and the two kinds of generator step
        z = _noise(model, a.nb, i)
        before = a.state_dict(full=True)
        grads = [g.cpu().numpy() for g in a.step(xs[i], noise=z, apply_updates=False)["grads"]]
        assert "health" not in a.last
        a.load_state_dict(before)
        r = a.step(xs[i], noise=z)
        after = a.state_dict(full=False)
        rec = r["health"]
        assert a.last["health"] is rec and rec["step"] == i and rec["kind"] == r["kind"] == ("disc" if i == 0 else "gen")
        assert rec["distance"] == float(r["distance"]) and rec["entropy"] == float(r["entropy"])
        net = a.discriminator if i == 0 else a.generator
        names = list(net.named_variables())
        assert list(rec["vars"]) == names and rec["net"] == names[0].split("/")[0]
        want = R.record(i, rec["kind"], names, grads, [before[n].numpy() for n in names], [after[n].numpy() for n in names])

        def norms_close(got, ref, n, what):
            nonlocal worst
            err, bar = abs(got * got - ref * ref), (n + 3) * 2.0 ** -53 * ref * ref
            worst = max(worst, err / bar if bar else 0.0)
            assert err <= bar, (what, got, ref)
        total = 0
        for name in names:
            v, w = rec["vars"][name], want["vars"][name]
            for k in ("n", "grad_amax", "grad_zero", "grad_nonfinite", "grad_below_11", "grad_below_22", "param_amax", "update_amax"):
                assert v[k] == w[k], (name, k, v[k], w[k])
            for k in ("grad_norm", "param_norm", "update_norm"):
                norms_close(v[k], w[k], v["n"], (name, k))
            total += v["n"]
            assert v["n"] == before[name].numel()
        for k in ("grad_nonfinite", "grad_below_11", "grad_below_22"):
            assert rec[k] == want[k], k
        for k in ("grad_norm", "param_norm", "update_norm"):
            norms_close(rec[k], want[k], total, k)
        assert rec["update_ratio"] == rec["update_norm"] / rec["param_norm"] and rec["grad_nonfinite"] == 0
        sk = rec["sinkhorn"]
        marg = _staged_marginals(*seen[-1])
        assert len(seen) == 2 * (i + 1) and sk["iters"] == ITERS and sk["lambda"] == LAM and sk["problems"] == list(health.TWO_BATCH_PROBLEMS)
        assert sk["row_err_max"] == marg[:, 0].tolist() and sk["col_err_max"] == marg[:, 2].tolist()
        assert sk["col_err_mean"] == marg[:, 3].tolist()
        print(model, "step", i, "|g|", rec["grad_norm"], "update/param", rec["update_ratio"], "below 22", rec["grad_below_22"],
              "column error", max(sk["col_err_max"]))
    print("worst norm error / bar", worst)
    a.close()


def test_single_batch_and_no_sinkhorn():
    from otgan_amd.trainer import OTGAN, default_args, assemble_single_log_kernels
    kw = dict(model="dcgan", batch_size=4, nr_gpu=2, sinkhorn_lambda=LAM, nr_sinkhorn_iter=ITERS, nr_gen_per_disc=NGD, seed=3,
              step_graph=False, health_every=1)
    m = OTGAN(default_args(no_sinkhorn=True, **kw), DEV)
    assert m.step(_data(m)[0])["health"]["sinkhorn"] is None
    m.close()
    m = OTGAN(default_args(single_batch=True, **kw), DEV)
    seen = []
    real = OTGAN._match

    def match(self, f_gen, f_dat, *a, **k):
        seen.append((f_gen.detach().clone(), f_dat.detach().clone()))
        return real(self, f_gen, f_dat, *a, **k)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(OTGAN, "_match", match)
        sk = m.step(_data(m)[0])["health"]["sinkhorn"]
    fa, fb = seen[0]
    K = assemble_single_log_kernels(matching.cost_log_kernels([fa, fb, fa], [fa, fb, fb], LAM).unsqueeze(0), LAM)   # 999 on a-a, b-b
    marg = ops.plan_marginals(matching.sinkhorn_plans(K, LAM, ITERS)).cpu().numpy()
    assert sk["problems"] == list(health.SINGLE_BATCH_PROBLEMS) and sk["col_err_max"] == marg[:, 2].tolist()
    assert sk["row_err_max"] == marg[:, 0].tolist() and sk["col_err_mean"] == marg[:, 3].tolist()
    m.close()


def _argv(save, extra=()):
    return ["--synthetic", "--synthetic_size", "24", "--nr_gpu", "2", "--batch_size", "4", "--nr_sinkhorn_iter", str(ITERS),
            "--sinkhorn_lambda", str(LAM), "--nr_gen_per_disc", str(NGD), "--save_dir", save, "--seed", "3", "--max_steps", "7",
            "--step_graph", "0"] + list(extra)


def test_train_main(tmp_path, capsys):
    from otgan_amd import train
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    m = train.main(_argv(on, ["--health_every", "2"]))
    sd_on = m.state_dict(full=True)
    m.close()
    out = capsys.readouterr().out
    path = os.path.join(on, "health.jsonl")
    assert os.path.exists(path)
    recs = [json.loads(line) for line in open(path)]
    assert [r["step"] for r in recs] == R.reported(7, 2, NGD + 1) == [0, 1, 2, 3, 4, 6]
    assert {r["kind"] for r in recs} == {"gen", "disc"} and [r["epoch"] for r in recs] == [0, 0, 0, 1, 1, 2]      # 3 steps an epoch
    for r in recs:
        assert r["kind"] == R.kind(r["step"], NGD + 1) and r["grad_nonfinite"] == 0 and r["update_ratio"] > 0
        assert len(r["sinkhorn"]["col_err_max"]) == 6 and r["sinkhorn"]["iters"] == ITERS
        assert all(set(v) >= {"n", "grad_norm", "grad_below_22", "update_norm"} for v in r["vars"].values())
    lines = [l for l in out.splitlines() if l.startswith("health: ")]
    assert len(lines) == 3 and all("(L = %d)" % ITERS in l and "|g| gen" in l for l in lines)
    assert lines[-1] == health.summary_line({"gen": recs[4], "disc": recs[5]})
    m = train.main(_argv(off))
    sd_off = m.state_dict(full=True)
    m.close()
    assert "health:" not in capsys.readouterr().out and not os.path.exists(os.path.join(off, "health.jsonl"))
    from test_probe_gpu import _same as same_tree
    same_tree(sd_on, sd_off)


def test_non_finite_gradients(tmp_path):
    m = _model("dcgan", False, 1)
    path = str(tmp_path / "health.jsonl")
    m.health_sink = lambda rec: health.append(path, rec)
    xs = _data(m)
    m.step(xs[0])                                                # a critic step, reported
    with torch.no_grad():
        m.gen_params[0].view(-1)[0] = float("nan")
    ops.bump_weights_epoch()
    before = m.state_dict(full=True)
    t = (m.gen_optimizer.t, m.disc_optimizer.t, m.step_counter)
    with pytest.raises(FloatingPointError) as e:
        m.step(xs[1])
    names = list(m.generator.named_variables())
    said = str(e.value)
    assert "generator" in said and any(n in said for n in names) and "discriminator/" not in said
    # the update was not applied: parameters, moments, step counts as before (bits: the poisoned weight is a NaN)
    after = m.state_dict(full=True)
    assert (m.gen_optimizer.t, m.disc_optimizer.t, m.step_counter) == t
    for k, v in before.items():
        if torch.is_tensor(v):
            assert torch.equal(v.view(torch.int32), after[k].view(torch.int32)), k
    for n in before["__ema__"]:
        assert torch.equal(before["__ema__"][n], after["__ema__"][n])
    # the line is in the file already
    recs = health.read(path)
    assert [r["step"] for r in recs] == [0, 1] and recs[1]["kind"] == "gen" and recs[1]["grad_nonfinite"] > 0
    assert recs[1]["param_norm"] is None and recs[1]["update_ratio"] is None
    bad = [n for n, v in recs[1]["vars"].items() if v["grad_nonfinite"]]
    assert bad and set(bad) <= set(names) and all(n in said for n in bad)
    assert m.last["health"]["step"] == 1
    m.close()
