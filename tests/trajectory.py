"""Teacher-forced, step-by-step check of a multi-step OT-GAN training trajectory against the fp64 oracle
(oracle/train_step_cpu.py) and the reference's update rule (oracle/nets_torch.py::adam_update).

Every step k of a schedule gets its own data batch and latent.  The step is run FOR REAL (updates applied, no
extra gradient-only step that would warm the caches under test); what it handed to its optimiser is recorded, and
the complete state -- variables, both optimisers' moments and step counters, EMA shadows -- is snapshotted before
and after.  The oracle is then evaluated at the BEFORE state, so a step that read anything older than that state
(a normalised weight, a Winograd filter, a dense-block operand or an EMA operand that survived an update) shows
up as a gradient error, and a wrong counter, sign, schedule or flat-buffer offset as a bookkeeping error.

The checker talks to a small adapter, so that it runs over the HIP trainer (HipTrainer below) and over a CPU
stand-in (tests/test_trajectory_cpu.py, which also feeds it deliberately faulty stand-ins) alike:

    adapter.model, .nonlinearity            "dcgan" | "densenet", the nets' --nonlinearity
    adapter.nr_gen_per_disc, .shards, .lam, .iters, .lr_disc, .lr_gen, .ema_critic
    adapter.names(scope)                    variable names of "discriminator" / "generator", in gradient-list order
    adapter.snapshot()                      -> {"vars": {name: t}, "ema": {name: t},
                                                "opt": {"gen" | "disc": {"t": float, "v": {name: t}, "mg": {name: t}}}}
                                               (CPU tensors in the dtype the trainer keeps them in)
    adapter.step(x, noise)                  -> {"kind", "distance", "entropy", "grads": [t, ...], "signs": [t, ...]}
                                               grads: what the step gave its optimiser; signs: the sign pattern of
                                               every feature-head call of the step, in call order

A violation raises TrajectoryError("step k [tag] ...") at the first check that fails; the tags are
schedule, step-counter, untouched, update-rule, ema, gradient, head-signs, distance, entropy, control."""
import torch

from oracle import nets_torch as NT
from oracle.train_step_cpu import CpuOTGAN

# bounds shared with tests/test_train_step_gpu.py / test_layers_gpu.py::test_optimiser_steps
UPDATE_TOL = 1e-6            # parameters, moments and EMA shadows against the fp64 update rule, relative L2 per variable
SCALAR_TOL = 1e-4            # distance (abs 1e-7) and entropy against the oracle
MAX_FLIPPED, MAX_FLIPPED_X = 8, 2e-5     # forced feature-head signs that differ from the oracle's own: units, |x| / sample RMS
FLIP_TENSOR_TOL, FLIP_MEDIAN_TOL = 3e-2, 5e-3      # un-forced CReLU steps (test_step_gradients_match_oracle)
CONTROL_FACTOR = 20.0        # stale-operand control: the project's `e_live > 20 * e_ema`
MOM1, MOM2, EMA_DECAY = 0.5, 0.999, 0.999          # reference train.py:63,142-143


class TrajectoryError(AssertionError):
    pass


def _fail(k, tag, msg):
    raise TrajectoryError(f"step {k} [{tag}] {msg}")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def expected_kind(k, nr_gen_per_disc):
    """reference train.py:214-226: a critic step iff the iteration is a multiple of nr_gen_per_disc + 1"""
    return "disc" if k % (nr_gen_per_disc + 1) == 0 else "gen"


def make_inputs(model, nb, steps, seed, size=32):
    """Distinct (x_k, noise_k) per step from a seeded CPU generator."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=gen) * 2 - 1
    xs, noises = [], []
    for _ in range(steps):
        xs.append(u(nb, size, size, 3))
        noises.append(u(nb, 100) if model == "dcgan" else [u(nb, 100), u(nb, 8, 8, 16), u(nb, 16, 16, 16), u(nb, 32, 32, 16)])
    return xs, noises


def _to64(z):
    return [t.double() for t in z] if isinstance(z, list) else z.double()


def _scope_vars(snap, scope):
    return {n: t for n, t in snap["vars"].items() if n.startswith(scope + "/")}


class _Oracle:
    def __init__(self, ad):
        self.ad = ad
        self.o = CpuOTGAN(ad.model, ad.nonlinearity, dtype=torch.float64, use_c_matching=False)

    def grads(self, named, kind, x, noise, ema=None, signs=None):
        """-> ({name: gradient}, distance, entropy, forced-sign report) of the oracle step at the variables `named`."""
        ad, o = self.ad, self.o
        o.load(named)
        ema_P = o.ema_params(ema) if (ema is not None and kind == "disc") else None
        NT.FORCED_HEAD_SIGNS = [s.clone() for s in signs] if signs is not None else None      # (the oracle pops them)
        del NT.FORCED_HEAD_REPORT[:]
        try:
            gr, dist, ent = o.grads(kind, x.double(), _to64(noise), ad.shards, ad.lam, ad.iters, ema_P=ema_P)
        finally:
            NT.FORCED_HEAD_SIGNS = None
        report = list(NT.FORCED_HEAD_REPORT)
        del NT.FORCED_HEAD_REPORT[:]
        names = ad.names("generator" if kind == "gen" else "discriminator")
        assert len(names) == len(gr)
        return dict(zip(names, gr)), dist, ent, report


def _check_bookkeeping(ad, k, kind, before, after, grads):
    """Everything that needs no oracle: counters, the network that must not move, the update rule, the EMA."""
    me, other = ("disc", "gen") if kind == "disc" else ("gen", "disc")
    scope, other_scope = ("discriminator", "generator") if kind == "disc" else ("generator", "discriminator")
    t0, t1 = before["opt"][me]["t"], after["opt"][me]["t"]
    if t1 != t0 + 1:
        _fail(k, "step-counter", f"the {me} optimiser's t went {t0} -> {t1} in its own step (must advance by exactly 1)")
    if after["opt"][other]["t"] != before["opt"][other]["t"]:
        _fail(k, "step-counter", f"the {other} optimiser's t moved {before['opt'][other]['t']} -> {after['opt'][other]['t']} "
                                 f"in a {me} step (train.py:142-143: one counter per optimiser)")
    for n, t in _scope_vars(before, other_scope).items():
        if not torch.equal(t, after["vars"][n]):
            _fail(k, "untouched", f"{n} changed in a {me} step")
    for slot in ("v", "mg"):
        for n, t in before["opt"][other][slot].items():
            if not torch.equal(t, after["opt"][other][slot][n]):
                _fail(k, "untouched", f"the {other} optimiser's {slot} of {n} changed in a {me} step")
    # the reference update in fp64 on the BEFORE state and the recorded gradient
    lr = -ad.lr_disc if kind == "disc" else ad.lr_gen             # train.py:142-143
    names = ad.names(scope)
    assert len(names) == len(grads), (len(names), len(grads))
    for n, g in zip(names, grads):
        st = {"t": t0, "v": before["opt"][me]["v"][n].double(), "mg": before["opt"][me]["mg"][n].double()}
        ref = NT.adam_update(before["vars"][n].double(), g.double().cpu(), st, lr, MOM1, MOM2)
        for what, got, want in (("parameter", after["vars"][n], ref), ("v", after["opt"][me]["v"][n], st["v"]),
                                ("mg", after["opt"][me]["mg"][n], st["mg"])):
            e = rel(got, want)
            if not e < UPDATE_TOL:
                _fail(k, "update-rule", f"{what} of {n} is {e:.2e} from adam_update(before, recorded gradient, lr = {lr:g}, "
                                        f"t = {t0:g}) (bound {UPDATE_TOL:g})")
    for n, sh0 in before["ema"].items():
        sh1 = after["ema"][n]
        if kind == "disc":
            if not torch.equal(sh0, sh1):
                _fail(k, "ema", f"the shadow of {n} changed in a critic step")
        else:
            want = EMA_DECAY * sh0.double() + (1.0 - EMA_DECAY) * after["vars"][n].double()       # train.py:63-64, 223
            e = rel(sh1, want)
            if not e < UPDATE_TOL:
                _fail(k, "ema", f"the shadow of {n} is {e:.2e} from {EMA_DECAY} * before + {1 - EMA_DECAY:.3f} * updated "
                                f"weights (bound {UPDATE_TOL:g})")


def run(ad, xs, noises, grad_tol=None, force_signs=True, oracle=True, control=True, log=print):
    """Run and check the trajectory.  grad_tol: per-tensor relative-L2 bound of the gradients with forced head signs;
    None = the flip-tolerant bounds of an un-forced CReLU step (every tensor FLIP_TENSOR_TOL, median FLIP_MEDIAN_TOL).
    oracle=False: schedule and bookkeeping only.  -> per-step report (list of dicts)."""
    orc = _Oracle(ad) if oracle else None
    period = ad.nr_gen_per_disc + 1
    # the control must separate a stale operand from the tightest bound the step is held to
    control_floor = CONTROL_FACTOR * (grad_tol if grad_tol is not None else FLIP_MEDIAN_TOL)
    snaps, report = [], []
    for k, (x, noise) in enumerate(zip(xs, noises)):
        kind = expected_kind(k, ad.nr_gen_per_disc)
        before = ad.snapshot()
        snaps.append(before)
        r = ad.step(x, noise)
        after = ad.snapshot()
        if r["kind"] != kind:
            _fail(k, "schedule", f"ran a {r['kind']} step, the reference runs a {kind} step (k % {period} == {k % period})")
        grads = [g.detach().cpu() for g in r["grads"]]
        _check_bookkeeping(ad, k, kind, before, after, grads)
        row = {"step": k, "kind": kind}
        report.append(row)
        if orc is None:
            log(f"  step {k:2d} {kind:4s} schedule / counters / update rule / EMA ok")
            continue
        ema = before["ema"] if ad.ema_critic else None
        signs = r["signs"] if force_signs else None
        if force_signs and len(r["signs"]) != (1 if kind == "disc" else 2):
            _fail(k, "head-signs", f"{len(r['signs'])} feature-head calls recorded in a {kind} step")
        gr, dist, ent, rep = orc.grads(before["vars"], kind, x, noise, ema=ema, signs=signs)
        names = list(gr)
        errs = sorted((rel(a, gr[n]), n) for n, a in zip(names, grads))
        worst, median = errs[-1], errs[len(errs) // 2][0]
        flipped = sum(c for c, _ in rep)
        biggest = max([v for _, v in rep] + [0.0])
        row.update(worst=worst[0], worst_name=worst[1], median=median, flipped=flipped, biggest=biggest)
        log(f"  step {k:2d} {kind:4s} worst {worst[0]:.2e} ({worst[1]})  median {median:.2e}  distance {float(r['distance']):.6f} "
            f"(oracle {dist:.6f})  forced signs differing {flipped} (|x| <= {biggest:.1e} RMS)")
        if grad_tol is not None:
            if not worst[0] < grad_tol:
                _fail(k, "gradient", f"{worst[1]} is {worst[0]:.2e} from the oracle evaluated at the pre-step state (bound "
                                     f"{grad_tol:g}; median {median:.2e}; forced signs differing {flipped}, |x| <= {biggest:.1e})")
        else:
            if not worst[0] < FLIP_TENSOR_TOL:
                _fail(k, "gradient", f"{worst[1]} is {worst[0]:.2e} from the oracle evaluated at the pre-step state (bound "
                                     f"{FLIP_TENSOR_TOL:g})")
            if not median < FLIP_MEDIAN_TOL:
                _fail(k, "gradient", f"the median tensor is {median:.2e} from the oracle evaluated at the pre-step state "
                                     f"(bound {FLIP_MEDIAN_TOL:g})")
        if force_signs:
            if len(rep) != len(signs) or flipped > MAX_FLIPPED or biggest > MAX_FLIPPED_X:
                _fail(k, "head-signs", f"{flipped} forced units differ from the oracle's own signs, largest |x| {biggest:.2e} of "
                                       f"the sample's RMS (bounds {MAX_FLIPPED}, {MAX_FLIPPED_X:g}); {len(rep)} head calls")
        d = float(r["distance"])
        if not abs(d - dist) <= SCALAR_TOL * abs(dist) + 1e-7:
            _fail(k, "distance", f"{d!r} against the oracle's {dist!r}")
        e = float(r["entropy"])
        if not abs(e - ent) <= SCALAR_TOL * abs(ent):
            _fail(k, "entropy", f"{e!r} against the oracle's {ent!r}")
        # sensitivity control: would this step's check have seen operands that are one update old?
        if control and k >= 1 and k in (1, period):
            if kind == "gen":
                what = "critic one update old"
                stale = dict(before["vars"])
                stale.update(_scope_vars(snaps[k - 1], "discriminator"))
                gs, _, _, _ = orc.grads(stale, kind, x, noise)
            elif ad.ema_critic:
                # this critic step reads the shadows, not the live generator: the wrong operand here is the live generator
                what = "live generator instead of the EMA generator"
                gs, _, _, _ = orc.grads(before["vars"], kind, x, noise)
            else:
                what = "generator one update old"
                stale = dict(before["vars"])
                stale.update(_scope_vars(snaps[k - 1], "generator"))
                gs, _, _, _ = orc.grads(stale, kind, x, noise)
            e_stale = min(rel(a, gs[n]) for n, a in zip(names, grads))
            row.update(control=e_stale, control_what=what)
            log(f"          control ({what}): closest tensor {e_stale:.2e} (must be >= {control_floor:.1e})")
            if not e_stale >= control_floor:
                _fail(k, "control", f"an oracle with the {what} is only {e_stale:.2e} away on its closest tensor: the gradient "
                                    f"bound would not separate it (needs {control_floor:.1e})")
    return report


def summary(report):
    """(worst gradient error over all steps, smallest control error or None)"""
    worst = max((r["worst"] for r in report if "worst" in r), default=None)
    ctl = min((r["control"] for r in report if "control" in r), default=None)
    return worst, ctl


# ------------------------------------------------------------------------------------------------- the HIP trainer
class HipTrainer:
    """Adapter over otgan_amd.trainer.OTGAN.  Nothing is added to the launches of a step: the gradient list is cloned on
    its way into OTGAN._optimise (wrapped on the instance) and the feature head's input signs are copied out as
    tests/test_train_step_gpu.py does."""

    def __init__(self, device, **over):
        from otgan_amd.trainer import OTGAN, default_args
        over.setdefault("step_graph", False)
        self.args = a = default_args(**over)
        self.device = device
        self.m = m = OTGAN(a, device)
        assert m.graphs is None
        self.model, self.nonlinearity = a.model, a.nonlinearity
        self.nr_gen_per_disc, self.shards = a.nr_gen_per_disc, m.shards
        self.lam, self.iters = a.sinkhorn_lambda, a.nr_sinkhorn_iter
        self.lr_disc, self.lr_gen, self.ema_critic = a.learning_rate_disc, a.learning_rate_gen, a.train_disc_against_ema
        self.nb = m.nb
        self._names = {"discriminator": list(m.discriminator.named_variables()), "generator": list(m.generator.named_variables())}
        self._recorded = None
        real = m._optimise

        def recording_optimise(opt, grads, lr, critic):
            self._recorded = [g.detach().clone() for g in grads]
            return real(opt, grads, lr, critic)
        m._optimise = recording_optimise

    def names(self, scope):
        return self._names[scope]

    def _moments(self, opt, saved, scope):
        """The flat moment buffers of a saved optimiser state as {name: tensor}: every parameter sits at its own offset inside
        the group's flat buffer (no order assumed)."""
        flat = opt.group.flat
        slot = saved["slots"][0]
        out = {"t": float(saved["t"]), "v": {}, "mg": {}}
        for n, p in zip(self._names[scope], opt.params):
            off = (p.data_ptr() - flat.data_ptr()) // 4
            assert 0 <= off and off + p.numel() <= flat.numel()
            for key in ("v", "mg"):
                buf = slot.get(key)
                out[key][n] = (torch.zeros(p.shape) if buf is None           # (allocated by the optimiser's first step)
                               else buf[off:off + p.numel()].view(p.shape).clone())
        return out

    def snapshot(self):
        m = self.m
        sd = m.state_dict(full=True)
        assert len(m.gen_optimizer.state) == 1 and len(m.disc_optimizer.state) == 1 and len(sd["__optim__"]["gen"]["slots"]) == 1
        return {"vars": {n: t.clone() for n, t in sd.items() if "/" in n},
                "ema": {n: t.clone() for n, t in sd["__ema__"].items()},
                "opt": {"gen": self._moments(m.gen_optimizer, sd["__optim__"]["gen"], "generator"),
                        "disc": self._moments(m.disc_optimizer, sd["__optim__"]["disc"], "discriminator")}}

    def step(self, x, noise):
        from otgan_amd.utils import nn as hip_nn
        dev = self.device
        signs = []
        real_head = hip_nn.feature_head

        def recording_head(z):
            signs.append(torch.sign(z.detach()).cpu())
            return real_head(z)
        self._recorded = None
        noise = [t.to(dev) for t in noise] if isinstance(noise, list) else noise.to(dev)
        hip_nn.feature_head = recording_head
        try:
            r = self.m.step(x.to(dev), noise=noise)
        finally:
            hip_nn.feature_head = real_head
        assert self._recorded is not None, "the step never reached its optimiser"
        return {"kind": r["kind"], "distance": float(r["distance"]), "entropy": float(r["entropy"]),
                "grads": [g.cpu() for g in self._recorded], "signs": signs}

    def close(self):
        self.m.close()
