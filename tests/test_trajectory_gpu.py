"""GPU: multi-step training trajectories of the HIP trainer pinned to the fp64 oracle step by step
(tests/trajectory.py; the harness is itself tested, with faulty stand-ins, in tests/test_trajectory_cpu.py).

What carries state from one step to the next -- the normalised-weight / folded-weight / Winograd-filter cache and its
storage epochs, the dense-block operand cache, the critic operands kept across the generator steps of a period, the EMA
generator's cached weights, the two optimisers' counters, the critic's negated learning rate, the schedule with more than
one generator step per period, and the DenseNet optimiser path (flatten_like + flat Adam + separate EMA launch) -- is held
against an independent reference here: every step runs for real, and the oracle is evaluated at the state the step
started from.  Replayed step graphs are tied to these eager steps through the bit-identity tests
(tests/test_step_graph_gpu.py, tests/test_step_graph_interleave_gpu.py)."""
import pytest
import torch

from tests import trajectory as TJ

pytestmark = pytest.mark.gpu

LAM, ITERS = 20.0, 10
LR = 1e-3       # one update moves the gradients far beyond the bounds below (the control of every case verifies it)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# Gradient bounds of the forced-sign (ELU) cases: worst tensor over ALL steps of the case against the fp64 oracle, measured
# on the MI355X (pytest -s prints every step), times 3 -- the margin of test_train_step_gpu.py::_WELL_TOL, for the same reason
# (a compiler or summation-order change moves these errors by tens of per cent).  Whatever is measured, no bound may exceed
# CEILING: an order below the smallest effect of a one-update-old operand.
#   case   worst tensor per step (d g g d g g d; c: d g g d g)                                 maximum    bound
#   a      6.49e-6  5.12e-6  3.61e-6  4.25e-6  3.71e-6  3.65e-6  6.54e-6                      6.54e-6    2.0e-5
#   b      6.49e-6  5.12e-6  3.61e-6  4.88e-6  3.53e-6  4.97e-6  7.28e-6                      7.28e-6    2.2e-5
#   c      5.13e-6  1.84e-6  3.94e-6  2.08e-6  2.44e-6                                        5.13e-6    1.5e-5
# (forced signs differing from the oracle's own: 0 - 1 unit per step, |x| <= 5.0e-6 of the sample's RMS.)
# Closest tensor of the stale-operand control, which must stay 20 x the bound away (4.0e-4 / 4.4e-4 / 3.0e-4):
#   a      critic one update old 9.84e-1, generator one update old 5.43e-1
#   b      critic one update old 9.84e-1, live instead of EMA generator 1.29
#   c      critic one update old 1.48,    generator one update old 6.47e-2
#   d      (CReLU, un-forced; worst / median per step 2.1e-3 / 1.4e-3, 5.8e-6 / 3.3e-6, 3.0e-4 / 2.3e-4, 6.2e-5 / 4.4e-5)
#          critic one update old 9.09e-1, generator one update old 6.22e-1 (must be >= 1e-1 = 20 x the median bound)
CEILING = 1e-4
GRAD_TOL = {"a": 2.0e-5, "b": 2.2e-5, "c": 1.5e-5}
assert all(v <= CEILING for v in GRAD_TOL.values())

CASES = {
    "a": dict(over=dict(model="dcgan", nonlinearity="elu", nr_gen_per_disc=2), steps=7),
    "b": dict(over=dict(model="dcgan", nonlinearity="elu", nr_gen_per_disc=2, train_disc_against_ema=True), steps=7),
    "c": dict(over=dict(model="densenet", nonlinearity="elu", nr_gen_per_disc=2), steps=5),
}


def _trainer(dev, seed, **over):
    free, total = torch.cuda.mem_get_info(dev)
    print(f"\ndevice memory: {torch.cuda.memory_allocated(dev) / 2 ** 30:.1f} GiB held by this process' tensors, "
          f"{free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB free")
    return TJ.HipTrainer(dev, batch_size=3, nr_gpu=2, sinkhorn_lambda=LAM, nr_sinkhorn_iter=ITERS, learning_rate_disc=LR,
                         learning_rate_gen=LR, seed=seed, step_graph=False, **over)


@pytest.mark.parametrize("case", sorted(CASES))
def test_trajectory_matches_oracle_step_by_step(dev, case):
    """Cases a (DCGAN, two generator steps per period), b (a + --train_disc_against_ema: the oracle's critic step reads
    the BEFORE shadows) and c (DenseNet: more variables than the gathered Adam step takes, the unfused EMA, the dense-block
    operand cache across updates).  ELU, head signs shared with the oracle: arithmetic-only comparisons."""
    spec = CASES[case]
    ad = _trainer(dev, seed=5, **spec["over"])
    try:
        assert ad.nb == 6
        xs, noises = TJ.make_inputs(ad.model, ad.nb, spec["steps"], seed=21)
        print(f"\ntrajectory case {case}:")
        rep = TJ.run(ad, xs, noises, grad_tol=GRAD_TOL[case], force_signs=True)
    finally:
        ad.close()
    worst, ctl = TJ.summary(rep)
    print(f"case {case}: worst tensor over {len(rep)} steps {worst:.2e} (bound {GRAD_TOL[case]:.1e}), closest control {ctl:.2e}")
    assert sum("control" in r for r in rep) == 2


def test_trajectory_production_nonlinearity(dev):
    """Case d: DCGAN with the default CReLU, d g d g, signs not forced.  A unit of any CReLU layer may legitimately fall on
    the other side of zero than in fp64, so the bounds are those of test_step_gradients_match_oracle (every tensor 3e-2, the
    median tensor of each step 5e-3); the control holds a one-update-old operand 20 x the median bound away."""
    ad = _trainer(dev, seed=5, model="dcgan", nr_gen_per_disc=1)
    try:
        assert ad.nonlinearity == "crelu"
        xs, noises = TJ.make_inputs(ad.model, ad.nb, 4, seed=22)
        print("\ntrajectory case d:")
        rep = TJ.run(ad, xs, noises, grad_tol=None, force_signs=False)
    finally:
        ad.close()
    assert [r["kind"] for r in rep] == ["disc", "gen", "disc", "gen"]
    assert sum("control" in r for r in rep) == 2


def test_trajectory_reference_schedule_bookkeeping(dev):
    """Case e: the reference's default nr_gen_per_disc = 5 over 13 steps (d 5g d 5g d), no oracle: which step kind runs,
    which optimiser's t moves, which network and moments move (the other bit for bit untouched), the update rule on the
    recorded gradients and the EMA rule."""
    ad = _trainer(dev, seed=6, model="dcgan", nonlinearity="elu")
    try:
        assert ad.nr_gen_per_disc == 5
        xs, noises = TJ.make_inputs(ad.model, ad.nb, 13, seed=23)
        print("\ntrajectory case e:")
        rep = TJ.run(ad, xs, noises, oracle=False)
    finally:
        ad.close()
    assert [r["kind"] for r in rep] == ["disc"] + ["gen"] * 5 + ["disc"] + ["gen"] * 5 + ["disc"]
