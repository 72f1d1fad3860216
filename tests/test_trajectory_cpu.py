"""CPU: the trajectory harness (tests/trajectory.py) proves itself.  An fp32 stand-in of the trainer -- the oracle's
own nets in fp32, NT.adam_update, an EMA in plain torch -- passes it; each deliberately faulty stand-in (the faults a
cached operand, a shared counter or a wrong sign would cause in the HIP trainer) is rejected with its own message.
The faults live in this stand-in only: nothing faulty ever runs on a GPU."""
import pytest
import torch

from oracle import nets_torch as NT
from oracle.train_step_cpu import CpuOTGAN
from tests import trajectory as TJ

LAM, ITERS, SHARDS, BATCH = 20.0, 10, 2, 2

# Gradient bound of the fp32 stand-in against the fp64 oracle with shared head signs.  Not a measurement of the
# stand-in: it is the ceiling tests/test_trajectory_gpu.py allows any forced-sign case (an order below the smallest
# effect of a one-update-old operand, >= 0.2 at these learning rates), and fp32 round-off through these nets sits two
# orders below it (PyTorch-CPU fp32 reaches ~5e-6 on such gradients, tests/test_train_step_gpu.py).
GRAD_TOL = 1e-4


class StandIn:
    """The trainer's adapter interface (tests/trajectory.py) over CpuOTGAN in fp32.  `fault` plants one mistake."""

    def __init__(self, nr_gen_per_disc, ema_critic=False, lr_disc=1e-3, lr_gen=1e-3, fault=None, seed=1):
        self.model, self.nonlinearity = "dcgan", "elu"
        self.nr_gen_per_disc, self.shards, self.lam, self.iters = nr_gen_per_disc, SHARDS, LAM, ITERS
        self.lr_disc, self.lr_gen, self.ema_critic, self.fault = lr_disc, lr_gen, ema_critic, fault
        self.nb = SHARDS * BATCH
        self.net = CpuOTGAN("dcgan", "elu", seed=seed, dtype=torch.float32, use_c_matching=False)
        self._names = {s: [f"{lay}/{leaf}" for lay in self.net.P if lay.startswith(s) for leaf in ("V", "g", "b")]
                       for s in ("discriminator", "generator")}
        z = lambda s: {n: torch.zeros_like(self._var(n)) for n in self._names[s]}
        self.opt = {"gen": {"t": 1.0, "v": z("generator"), "mg": z("generator")},
                    "disc": {"t": 1.0, "v": z("discriminator"), "mg": z("discriminator")}}
        self.ema = {n: self._var(n).detach().clone() for n in self._names["generator"]}
        self.step_counter = 0
        self.old = {"discriminator": None, "generator": None, "ema": None}      # the state one update earlier (for the faults)

    def _var(self, name):
        lay, leaf = name.rsplit("/", 1)
        return self.net.P[lay][leaf]

    def names(self, scope):
        return self._names[scope]

    def _vars(self, scope):
        return {n: self._var(n).detach().clone() for n in self._names[scope]}

    def snapshot(self):
        named = self._vars("discriminator")
        named.update(self._vars("generator"))
        return {"vars": named, "ema": {n: t.clone() for n, t in self.ema.items()},
                "opt": {k: {"t": o["t"], "v": {n: t.clone() for n, t in o["v"].items()},
                            "mg": {n: t.clone() for n, t in o["mg"].items()}} for k, o in self.opt.items()}}

    def step(self, x, noise):
        period = self.nr_gen_per_disc + 1
        phase = (self.step_counter + (1 if self.fault == "schedule_off_by_one" else 0)) % period
        kind = "disc" if phase == 0 else "gen"
        scope, me = ("discriminator", "disc") if kind == "disc" else ("generator", "gen")
        # forward / backward, possibly on operands that are one update old
        live = None
        if self.fault == "stale_critic_in_gen_step" and kind == "gen" and self.old["discriminator"] is not None:
            live = self._vars("discriminator")
            self.net.load(self.old["discriminator"])
        if self.fault == "stale_generator_in_critic_step" and kind == "disc" and self.old["generator"] is not None:
            live = self._vars("generator")
            self.net.load(self.old["generator"])
        shadows = self.ema
        if self.fault == "stale_ema_in_critic_step" and self.old["ema"] is not None:
            shadows = self.old["ema"]
        ema_P = self.net.ema_params(shadows) if (self.ema_critic and kind == "disc") else None
        signs = []
        real_head = NT.feature_head

        def recording_head(z):
            signs.append(torch.sign(z.detach()))
            return real_head(z)
        NT.feature_head = recording_head
        try:
            gr, dist, ent = self.net.grads(kind, x, noise, SHARDS, LAM, ITERS, ema_P=ema_P)
        finally:
            NT.feature_head = real_head
            if live is not None:
                self.net.load(live)
        grads = [g.detach().clone() for g in gr]
        # update (reference train.py:142-143: the critic ascends)
        self.old[scope] = self._vars(scope)
        lr = self.lr_gen if kind == "gen" else (self.lr_disc if self.fault == "critic_lr_not_negated" else -self.lr_disc)
        o = self.opt[me]
        if self.fault == "moments_reset_each_period" and kind == "disc":
            for slot in ("v", "mg"):
                for t in o[slot].values():
                    t.zero_()
        with torch.no_grad():
            for n, g in zip(self._names[scope], grads):
                st = {"t": o["t"], "v": o["v"][n], "mg": o["mg"][n]}
                self._var(n).copy_(NT.adam_update(self._var(n).detach(), g, st, lr, TJ.MOM1, TJ.MOM2))
                o["v"][n], o["mg"][n] = st["v"], st["mg"]
        o["t"] += 1.0
        if self.fault == "shared_t":
            self.opt["gen" if me == "disc" else "disc"]["t"] = o["t"]
        if kind == "gen" or self.fault == "ema_on_critic_steps":
            self.old["ema"] = {n: t.clone() for n, t in self.ema.items()}
            for n in self._names["generator"]:
                self.ema[n] = TJ.EMA_DECAY * self.ema[n] + (1.0 - TJ.EMA_DECAY) * self._var(n).detach()
        self.step_counter += 1
        return {"kind": kind, "distance": dist, "entropy": ent, "grads": grads, "signs": signs}


def _run(steps, seed=3, **kw):
    ad = StandIn(**kw)
    xs, noises = TJ.make_inputs("dcgan", ad.nb, steps, seed)
    return TJ.run(ad, xs, noises, grad_tol=GRAD_TOL, force_signs=True)


def test_clean_stand_in_passes():
    """d g g d g g d at both learning rates 1e-3, head signs forced from the fp32 run: every check holds at every step, and
    the control finds a one-update-old critic / generator at least 20 x the gradient bound away."""
    print()
    rep = _run(7, nr_gen_per_disc=2)
    assert [r["kind"] for r in rep] == ["disc", "gen", "gen", "disc", "gen", "gen", "disc"]
    worst, ctl = TJ.summary(rep)
    print(f"clean stand-in: worst gradient tensor over 7 steps {worst:.2e}, closest stale-operand control {ctl:.2e}")
    assert sum("control" in r for r in rep) == 2


def test_clean_stand_in_passes_with_ema_critic():
    """The EMA-critic branch of the harness (shadows taken from the BEFORE state; control against the live generator)."""
    print()
    rep = _run(3, nr_gen_per_disc=1, ema_critic=True)
    assert "live generator" in rep[2]["control_what"]


# fault -> (stand-in options, steps needed to reach the step at which it differs, the message it must be rejected with)
MUTANTS = {
    "stale_critic_in_gen_step": (dict(nr_gen_per_disc=2), 2, r"step 1 \[gradient\]"),
    "stale_generator_in_critic_step": (dict(nr_gen_per_disc=1), 3, r"step 2 \[gradient\]"),
    # one EMA update moves a shadow by 1e-3 of the weight update: a generator step large enough for a one-update-old shadow to
    # be far from the current one (as test_ema_critic_step_matches_oracle does)
    "stale_ema_in_critic_step": (dict(nr_gen_per_disc=1, ema_critic=True, lr_gen=0.05), 3, r"step 2 \[gradient\]"),
    "ema_on_critic_steps": (dict(nr_gen_per_disc=1), 3, r"step [02] \[ema\] the shadow of .* changed in a critic step"),
    "shared_t": (dict(nr_gen_per_disc=2), 1, r"step 0 \[step-counter\] the gen optimiser's t moved"),
    "critic_lr_not_negated": (dict(nr_gen_per_disc=2), 1, r"step 0 \[update-rule\] parameter of discriminator/"),
    "schedule_off_by_one": (dict(nr_gen_per_disc=2), 1, r"step 0 \[schedule\] ran a gen step"),
    "moments_reset_each_period": (dict(nr_gen_per_disc=1), 3, r"step 2 \[update-rule\] parameter of discriminator/"),
}


@pytest.mark.parametrize("fault", sorted(MUTANTS))
def test_faulty_stand_in_is_rejected(fault):
    kw, steps, message = MUTANTS[fault]
    print()
    with pytest.raises(TJ.TrajectoryError, match=message) as info:
        _run(steps, fault=fault, **kw)
    print(f"{fault}: {info.value}")
