"""GPU: replayed step graphs (trainer.GraphedSteps) against eager steps when the host does other work between steps.

A replayed graph keeps the device addresses it saw at capture time, and the host-side weight caches (ops.cached_weights,
ops._split_block_weights) decide AT CAPTURE TIME whether a graph recomputes the normalised weights and Winograd filters of a
network or reads tensors that already exist.  Whatever the host runs between steps -- `sample()` at every epoch end of
train.py, a step with an injected latent, a checkpoint reload -- can therefore decide what a graph reads for the rest of the
run.  Three kinds of test:

  1. interleaving: the same schedule twice from the same seed and data, eager throughout (`m.graphs is None`) and with
     graphs on, an EVENT before a chosen step in both: `sample` (m.sample(nb) or m.sample(100)), `sample_ema`, `eager`
     (that step with an injected latent), `reload` (load_state_dict(state_dict(full=True)), written in place)
     or `epoch_end` (sample + sample_ema + state_dict() before EVERY step: train.py with 1-step epochs).  With the period
     P = nr_gen_per_disc + 1 the single events go before every step P+1 ... 3P: before the "gen1" capture, between its
     replay and the "gen" capture, between the "gen" replay and the "disc" capture, and the same moments again between
     replays.  Parameters, EMA shadows, optimiser moments, step counts, per-step distances and the images the events
     returned must be bit-identical.  Each graph run asserts that the graphs are alive, that every step kind was captured
     and that each was replayed at least twice after the event (the run goes on until it was);
  2. what a capture reads: every lookup of the generator's (live or EMA) operands inside a capture is recomputed in that
     capture; the critic's are recomputed in the "gen1" capture, and read -- never recomputed, never eager -- from the
     tensors of the latest "gen1" graph in the "gen" and "disc" captures, their input-gradient filters included (the
     round-6 replay speed-up: the critic's filters are not rebuilt in every replay);
  3. the production entry points: train.main end to end (3-step epochs: a sample() falls between the "gen" replay and the
     first "disc" capture) with --step_graph 1 against --step_graph 0, and the benchmarked DenseNet batch (128 x 2, 200
     Sinkhorn iterations, nr_gen_per_disc 5) with one epoch-end sample before the first "disc" capture.

Measured on the parent commit of this test (graphs captured with whatever the host cache held), first diverging per-step
distance in brackets:
    dcgan 2:1   sample / sample100 before steps 5, 6: the "gen" / "disc" capture read the generator's operands that the
                sample had just made eagerly (a frozen generator from then on)                       [steps 8 / 9]
                eager before steps 5, 6: the "gen" / "disc" capture recomputed the critic's operands and filters in its
                own graph instead of reading the "gen1" graph's (values right, every replay rebuilds them)
    dcgan 1:1   sample / sample100 / epoch_end: the first "disc" capture read the sample's generator   [step 6]
                eager before step 4: the "disc" capture recomputed the critic's operands
    densenet    sample before every step 4 ... 9: the "disc" capture rebuilt the critic's dense-block operands (they were
                cached per batch size: n images in a generator step, 2 n in a critic step); before steps 5, 6 also the
                generator's operands as above                                                         [steps 8 / 9]
                sample100 before steps 4 ... 7: the same; the run then ended in a GPU memory-access fault in the schedule
                before step 8, so the later densenet schedules, the EMA-critic configuration, train.main and the
                benchmarked batch were not measured on the parent
    In the dcgan configurations sample_ema (plain critic) and reload passed there.  The parent also kept every trainer's
    parameter buffers (the FlatGroup registry) and, after close(), its cached weights (100+ MB of Winograd filters per
    wide layer): over a module of this size device memory ran out, a capture failed half-way and left its stream
    capturing, and every later launch of the process failed.  Both are released now, and a failed capture joins the
    second stream before it ends.
Wall time of this module on an MI355X: 128 s (136 s inside the whole GPU suite): 114 schedules, each a graph run and an
eager run of 7 - 22 steps with a fresh trainer, plus train.main and the benchmarked batch.  The reload schedules of a
configuration share one eager reference (a reload writes back the values the run holds, so the eager trajectory is the
same); the others cannot share one, as each event moves the RNG stream or the step that takes an injected latent.
"""
import collections
import gc
import os

import numpy as np
import pytest
import torch

from test_step_graph_gpu import _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    # every trainer of this module is closed; leave the process's scratch buffers as small as the next module expects
    from otgan_amd import ops
    from otgan_amd.utils import matching
    ops._ws.clear()
    matching._ws_cache.clear()
    ops.reset_amax_pool()
    gc.collect()
    torch.cuda.empty_cache()


CONFIGS = {
    # name: (model, nr_gen_per_disc, step_graph of the graph run, extra args)
    "dcgan_2to1": ("dcgan", 2, True, {}),
    "dcgan_1to1": ("dcgan", 1, True, {}),
    "densenet_2to1": ("densenet", 2, None, {}),          # graphs on by default: not forced
    "dcgan_2to1_ema_critic": ("dcgan", 2, True, {"train_disc_against_ema": True}),
}
EVENTS = ("sample", "sample100", "sample_ema", "eager", "reload")


def _kinds(ngd):
    return {"disc", "gen", "gen1"} if ngd > 1 else {"disc", "gen1"}


# ----------------------------------------------------------------------------------------------------------- probe
class Probe:
    """Wraps GraphedSteps.run / GraphedSteps._capture and the weight caches of ops (cached_weights, _split_block_weights,
    prepare_filters); every wrapper returns what the real function returns.  Records the replays (non-None returns of
    run), the captures, and for every cache lookup and filter preparation the capture it ran in (None: eager) and the
    capture that made the tensors it got.  The maker travels as an attribute of the value's first tensor (the probe holds
    no tensor: a wide layer's filters are 100+ MB)."""

    TAG = "_probe_made"

    def __init__(self):
        self.i = 0                 # index of the step being run (set by the caller)
        self.replays = []          # (step index, kind)
        self.captures = []         # (step index, kind); the position in the list is the capture's serial
        self.ctx = None            # serial of the capture under way
        self.lookups = []          # (ctx, storage of the parameter, serial of the value, "weights" | "block")
        self.filters = []          # (ctx, (storage of the parameter, serial) of the operand the filters were made from)
        self.pending = []          # filters made inside a lookup, before its value is returned: (ctx, operand)

    def _made(self, first, operands, V):
        """Serial of the capture that made a looked-up value (None: eager); tags its operands on first sight."""
        made = getattr(first, self.TAG, False)
        if made is False:
            made = self.ctx
            for t in operands:
                setattr(t, self.TAG, made)
                t._probe_param = V.untyped_storage().data_ptr()
        still = []
        for ctx, w in self.pending:
            if hasattr(w, "_probe_param"):
                self.filters.append((ctx, (w._probe_param, getattr(w, self.TAG))))
            else:
                still.append((ctx, w))
        self.pending = still
        return made

    def install(self, mp, structure=True):
        from otgan_amd import ops, trainer
        probe = self
        real_run, real_cap = trainer.GraphedSteps.run, trainer.GraphedSteps._capture

        def run(gs, x_data, phase):
            r = real_run(gs, x_data, phase)
            if r is not None:
                probe.replays.append((probe.i, gs._kind(phase)))
            return r

        def capture(gs, x_data, kind):
            probe.captures.append((probe.i, kind))
            probe.ctx = len(probe.captures) - 1
            try:
                return real_cap(gs, x_data, kind)
            finally:
                probe.ctx = None

        mp.setattr(trainer.GraphedSteps, "run", run)
        mp.setattr(trainer.GraphedSteps, "_capture", capture)
        if not structure:
            return
        real_cw, real_sb, real_pf = ops.cached_weights, ops._split_block_weights, ops.prepare_filters

        def cached_weights(V, g, compute):
            val = real_cw(V, g, compute)
            s = probe._made(val[0], val[:2], V)          # (w, wT, ...): the operands the filters are made from
            probe.lookups.append((probe.ctx, V.untyped_storage().data_ptr(), s, "weights"))
            return val

        def split_block_weights(Vs, per_layer, plan, F):
            val = real_sb(Vs, per_layer, plan, F)
            ops_ = [t for wd in val["wide"] for t in (wd["w"], wd["wT"])]
            s = probe._made(ops_[0], ops_, Vs[0])
            probe.lookups.append((probe.ctx, Vs[0].untyped_storage().data_ptr(), s, "block"))
            return val

        def prepare_filters(desc, which, w):
            if hasattr(w, "_probe_param"):
                probe.filters.append((probe.ctx, (w._probe_param, getattr(w, Probe.TAG))))
            else:
                probe.pending.append((probe.ctx, w))     # made by the lookup under way: resolved when it returns
            return real_pf(desc, which, w)

        mp.setattr(ops, "cached_weights", cached_weights)
        mp.setattr(ops, "_split_block_weights", split_block_weights)
        mp.setattr(ops, "prepare_filters", prepare_filters)

    def replayed_since(self, i0):
        c = collections.Counter(k for i, k in self.replays if i >= i0)
        return dict(c)

    def check_reads(self, m):
        """Section 2 of the module docstring, for every capture of the run; `m` is the run's model (its flat buffers tell
        the networks apart).  Returns a list of violations."""
        nets = {m.disc_params[0].untyped_storage().data_ptr(): "critic",
                m.gen_params[0].untyped_storage().data_ptr(): "generator",
                m.ema.average(m.gen_params[0]).untyped_storage().data_ptr(): "generator"}
        kind = [k for _, k in self.captures]
        at = [i for i, _ in self.captures]
        gen1, g1 = [], None
        for s, k in enumerate(kind):
            g1 = s if k == "gen1" else g1
            gen1.append(g1)
        name = lambda s: "an eager tensor" if s is None else f"capture {s} ('{kind[s]}' at step {at[s]})"
        bad, seen = [], collections.Counter()
        for ctx, V, s, what in self.lookups:
            if ctx is None:
                continue
            who = nets.get(V)
            if who is None:
                bad.append(f"capture {ctx}: a {what} lookup of an unknown parameter")
                continue
            seen[(ctx, who)] += 1
            want = ctx if (who == "generator" or kind[ctx] == "gen1") else gen1[ctx]
            if s != want or want is None:
                bad.append(f"{name(ctx)}: a {who} {what} lookup was served from {name(s)}, not from {name(want)}")
        for s in range(len(kind)):
            for who in ("generator", "critic"):
                if not seen[(s, who)]:
                    bad.append(f"{name(s)} made no {who} lookup")
        for ctx, _w in self.pending:
            bad.append(f"filters prepared ({'eager' if ctx is None else name(ctx)}) from an operand no cache lookup returned")
        for ctx, (V, s) in self.filters:
            who = nets.get(V)
            if who != "critic":
                continue
            if ctx is not None and kind[ctx] != "gen1":
                bad.append(f"{name(ctx)} prepared critic filters (from an operand of {name(s)})")
            elif s is not None and kind[s] == "gen1" and ctx != s:
                bad.append(f"critic filters of {name(s)}'s operands prepared {'eagerly' if ctx is None else 'in ' + name(ctx)}")
        return sorted(set(bad))


# ----------------------------------------------------------------------------------------------------------- runs
def _noise(model, nb, i):
    g = torch.Generator().manual_seed(100 + i)
    shapes = [(nb, 100)] if model == "dcgan" else [(nb, 100), (nb, 8, 8, 16), (nb, 16, 16, 16), (nb, 32, 32, 16)]
    u = [(torch.rand(s, generator=g) * 2 - 1).cuda() for s in shapes]
    return u[0] if model == "dcgan" else u


def _event(m, ev, outs):
    if ev == "sample":
        outs.append(m.sample(m.nb).cpu())
    elif ev == "sample100":
        outs.append(m.sample(100).cpu())
    elif ev == "sample_ema":
        outs.append(m.sample(100, ema=True).cpu())
    elif ev in ("epoch_end", "samples"):          # train.py:244-247
        outs.append(m.sample(100).cpu())
        outs.append(m.sample(100, ema=True).cpu())
        if ev == "epoch_end":
            m.state_dict()
    elif ev == "reload":
        m.load_state_dict(m.state_dict(full=True))
    elif ev not in ("eager", None):
        raise ValueError(ev)


def _trajectory(dev, model, ngd, graph, event, at, steps=None, probe=None, data=4, batch_size=4, iters=20, lam=100.0,
                snapshots=None, **kw):
    """One run: `event` before step `at` (a set of steps: before each of them; `epoch_end`: before every step).  `steps`
    None (graph runs): run until every kind is captured and each was replayed at least twice after the (last) event.
    -> the fields `_same` compares, plus the entropies, the events' outputs and the graph bookkeeping; with `snapshots`
    (step counts), {count: those fields after that many steps}."""
    from otgan_amd.trainer import OTGAN, default_args
    args = default_args(model=model, batch_size=batch_size, nr_gpu=2, sinkhorn_lambda=lam, nr_sinkhorn_iter=iters,
                        nr_gen_per_disc=ngd, seed=3, step_graph=graph, **kw)
    m = OTGAN(args, dev)
    if graph is False:
        assert m.graphs is None
    else:
        assert m.graphs is not None
    g = torch.Generator().manual_seed(11)
    xs = [(torch.rand(m.nb, 32, 32, 3, generator=g) * 2 - 1).to(dev) for _ in range(data)]
    torch.manual_seed(7)
    P = ngd + 1
    ats = at if isinstance(at, set) else {at}
    dists, ents, kinds, outs = [], [], [], []
    snaps = {}

    def result():
        sd = m.state_dict(full=True)
        return {"state": {k: v.clone() for k, v in sd.items() if torch.is_tensor(v)}, "opt": sd["__optim__"],
                "ema": sd["__ema__"], "dists": torch.stack(dists).cpu(), "ents": torch.stack(ents).cpu(), "kinds": list(kinds),
                "outs": list(outs), "t": (m.gen_optimizer.t, m.disc_optimizer.t, m.step_counter), "steps": len(kinds)}
    i = 0
    while True:
        if steps is not None and i >= steps:
            break
        if steps is None and i > at:
            since = 0 if event == "epoch_end" else at
            done = probe.replayed_since(since)
            if set(done) == _kinds(ngd) and min(done.values()) >= 2:
                break
            if i > at + 10 * P:
                break                       # the caller's condition check reports it
        if probe is not None:
            probe.i = i
        if event == "epoch_end" or i in ats:
            _event(m, event, outs)
        if event == "eager" and i in ats:
            r = m.step(xs[i % data], noise=_noise(model, m.nb, i))
        else:
            r = m.step(xs[i % data])
        dists.append(r["distance"].clone())
        ents.append(r["entropy"].clone())
        kinds.append(r["kind"])
        i += 1
        if snapshots is not None and i in snapshots:
            snaps[i] = result()
    if snapshots is not None:
        m.close()
        return snaps
    res = result()
    res["captured"] = set(m.graphs.graphs) if m.graphs is not None else set()
    res["dead"] = m.graphs.dead if m.graphs is not None else None
    if probe is not None:
        res["bad_reads"] = probe.check_reads(m)
    m.close()
    return res


def _first_divergence(a, b):
    n = min(len(a["dists"]), len(b["dists"]))
    diff = [i for i in range(n) if not torch.equal(a["dists"][i], b["dists"][i])]
    return diff[0] if diff else None


def _graph_run(dev, cfg, event, at):
    model, ngd, graph, kw = CONFIGS[cfg]
    probe = Probe()
    with pytest.MonkeyPatch.context() as mp:
        probe.install(mp)
        gr = _trajectory(dev, model, ngd, graph, event, at, probe=probe, **kw)
    return gr, probe


def _schedule(dev, cfg, event, at, ran=None, eg=None):
    """-> list of failure lines for one schedule (empty: it passed).  `ran`: its graph run (_graph_run), `eg`: its eager
    reference, when the caller has them."""
    model, ngd, graph, kw = CONFIGS[cfg]
    gr, probe = ran if ran is not None else _graph_run(dev, cfg, event, at)
    if eg is None:
        eg = _trajectory(dev, model, ngd, False, event, at, steps=gr["steps"], **kw)
    tag = f"{cfg} {event} before step {at}:"
    out = []
    since = 0 if event == "epoch_end" else at
    done = probe.replayed_since(since)
    if gr["dead"] is not None:
        out.append(f"{tag} graphs disabled: {gr['dead']}")
    if gr["captured"] != _kinds(ngd):
        out.append(f"{tag} captured {sorted(gr['captured'])}")
    if set(done) != _kinds(ngd) or min(done.values()) < 2:
        out.append(f"{tag} replays after the event {done} in {gr['steps']} steps")
    out += [f"{tag} {b}" for b in gr["bad_reads"]]
    try:
        _same(eg, gr)
        assert len(eg["outs"]) == len(gr["outs"]) and all(torch.equal(a, b) for a, b in zip(eg["outs"], gr["outs"])), \
            "event outputs differ"
    except AssertionError as e:
        k = _first_divergence(eg, gr)
        out.append(f"{tag} differs from the eager run (first diverging step distance: {k}; {str(e).splitlines()[0][:120]})")
    print(f"{tag} {gr['steps']} steps, captures {[k for _, k in probe.captures]} at {[i for i, _ in probe.captures]}, "
          f"replays after the event {done}: {'ok' if not out else 'FAIL'} ({torch.cuda.memory_allocated() / 2**30:.2f} GiB held)",
          flush=True)
    del gr, eg
    gc.collect()
    torch.cuda.empty_cache()
    return out


# ----------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("event", EVENTS + ("epoch_end",))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_events_between_replays(dev, cfg, event):
    """Section 1 and 2 of the module docstring: every position P+1 ... 3P (epoch_end: every step)."""
    model, ngd, graph, kw = CONFIGS[cfg]
    if graph is None:
        assert os.environ.get("OTGAN_STEP_GRAPH") is None     # the default must be what is tested
    P = ngd + 1
    positions = [0] if event == "epoch_end" else list(range(P + 1, 3 * P + 1))
    failures = []
    if event == "reload":
        # a reload writes the values the run already holds: the EAGER trajectory is the same whether it happens before one
        # of these steps or before each of them, so one eager run with a reload before every position, snapshotted at the
        # length of each graph run, is the reference of all six schedules
        ran = {at: _graph_run(dev, cfg, event, at) for at in positions}
        eg = _trajectory(dev, model, ngd, False, event, set(positions), steps=max(r[0]["steps"] for r in ran.values()),
                         snapshots={r[0]["steps"] for r in ran.values()}, **kw)
        for at in positions:
            failures += _schedule(dev, cfg, event, at, ran=ran[at], eg=eg[ran[at][0]["steps"]])
    else:
        for at in positions:
            failures += _schedule(dev, cfg, event, at)
    assert not failures, "\n".join(failures)


def test_train_main_graph_equals_eager(dev, tmp_path):
    """train.main with 3-step epochs (a sample() at every epoch end, between the "gen" replay and the first "disc" capture in
    the first window), --step_graph 1 against --step_graph 0: bit-identical models and distances.npz."""
    from otgan_amd import train
    failures = []
    for model in ("densenet", "dcgan"):
        res = {}
        for sg in ("1", "0"):
            save = str(tmp_path / f"{model}_{sg}")
            argv = ["--model", model, "--synthetic", "--synthetic_size", "48", "--nr_gpu", "2", "--batch_size", "8",
                    "--nr_sinkhorn_iter", "10", "--sinkhorn_lambda", "100", "--nr_gen_per_disc", "2", "--save_dir", save,
                    "--save_every", "1", "--seed", "3", "--max_steps", "15", "--step_graph", sg]
            probe = Probe()
            with pytest.MonkeyPatch.context() as mp:
                probe.install(mp)
                m = train.main(argv)
                if sg == "1":
                    assert m.graphs is not None and m.graphs.dead is None, model
                    assert set(m.graphs.graphs) == {"disc", "gen", "gen1"}, model
                    failures += [f"{model}: {b}" for b in probe.check_reads(m)]
                else:
                    assert m.graphs is None and not probe.replays
            res[sg] = ({k: (v.clone() if torch.is_tensor(v) else v) for k, v in m.state_dict(full=True).items()},
                       dict(np.load(os.path.join(save, "distances.npz"))), probe.replayed_since(0))
            m.close()
        done = res["1"][2]
        print(f"train.main {model}: captures, replays {done}", flush=True)
        assert set(done) == {"disc", "gen", "gen1"} and min(done.values()) >= 2, (model, done)
        a, b = res["1"][0], res["0"][0]
        assert a.keys() == b.keys()
        for k in a:
            if k == "__optim__":
                for net in ("gen", "disc"):
                    assert a[k][net]["t"] == b[k][net]["t"]
                    for sa, sb in zip(a[k][net]["slots"], b[k][net]["slots"]):
                        for s in sa:
                            assert (sa[s] is None and sb[s] is None) or torch.equal(sa[s], sb[s]), (model, net, s)
            elif k == "__ema__":
                for n in a[k]:
                    assert torch.equal(a[k][n], b[k][n]), (model, n)
            elif torch.is_tensor(a[k]):
                if not torch.equal(a[k], b[k]):
                    failures.append(f"{model}: {k} differs")
            else:
                assert a[k] == b[k], (model, k)
        da, db = res["1"][1], res["0"][1]
        assert da.keys() == db.keys()
        for k in da:
            if not np.array_equal(da[k], db[k]):
                failures.append(f"{model}: distances.npz {k} {da[k]} != {db[k]}")
    assert not failures, "\n".join(failures)


def test_benchmarked_batch_sample_before_first_disc_capture(dev):
    """configs[3] of test_full_batch_layers_gpu.py (densenet, 128 x 2, 200 Sinkhorn iterations) at the reference default
    nr_gen_per_disc = 5, graphs on by default: one epoch-end sample(100) + sample(100, ema=True) between the last "gen"
    replay and the first "disc" capture (step 2P), then until every kind was replayed twice after it.  Parameters, EMA and
    moments bit-identical; distances and entropies equal or within 1e-13 relative (the fp64 atomics of the Sinkhorn
    statistics add per-wave partial sums in arrival order once a problem spans several workgroups)."""
    assert os.environ.get("OTGAN_STEP_GRAPH") is None
    ngd = 5
    P = ngd + 1
    at = 2 * P
    kw = dict(batch_size=128, iters=200, lam=500.0)
    probe = Probe()
    with pytest.MonkeyPatch.context() as mp:
        probe.install(mp)
        gr = _trajectory(dev, "densenet", ngd, None, "samples", at, probe=probe, **kw)
    eg = _trajectory(dev, "densenet", ngd, False, "samples", at, steps=gr["steps"], **kw)
    done = probe.replayed_since(at)
    print(f"benchmarked batch: {gr['steps']} steps, captures {probe.captures}, replays after the event {done}", flush=True)
    assert gr["dead"] is None and gr["captured"] == _kinds(ngd)
    assert ("disc" not in {k for i, k in probe.captures if i < at}) and (at, "disc") in probe.captures, probe.captures
    assert set(done) == _kinds(ngd) and min(done.values()) >= 2, done
    assert not gr["bad_reads"], "\n".join(gr["bad_reads"])
    assert eg["kinds"] == gr["kinds"] and eg["t"] == gr["t"]
    assert len(eg["outs"]) == len(gr["outs"]) == 2 and all(torch.equal(a, b) for a, b in zip(eg["outs"], gr["outs"]))
    for name in ("dists", "ents"):
        for i, (a, b) in enumerate(zip(eg[name], gr[name])):
            assert torch.equal(a, b) or abs(float(a) - float(b)) <= 1e-13 * abs(float(a)), (name, i, float(a), float(b))
    for k in eg["state"]:
        assert torch.equal(eg["state"][k], gr["state"][k]), k
    for k in eg["ema"]:
        assert torch.equal(eg["ema"][k], gr["ema"][k]), k
    for net in ("gen", "disc"):
        assert eg["opt"][net]["t"] == gr["opt"][net]["t"]
        for sa, sb in zip(eg["opt"][net]["slots"], gr["opt"][net]["slots"]):
            for k in sa:
                assert (sa[k] is None and sb[k] is None) or torch.equal(sa[k], sb[k]), (net, k)
