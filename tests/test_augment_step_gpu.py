"""GPU: --augment in the training step (trainer.OTGAN with args.augment): the step's gradients against the fp64 oracle step with
T (tests/augment_ref.py) in front of every critic pass, the wiring with an identity T, replayed step graphs, the paths that are
never augmented, and train.main end to end."""
import math
import re

import pytest
import torch

import augment_ref as R
from oracle.train_step_cpu import CpuOTGAN

pytestmark = pytest.mark.gpu

POLICY = "color,translation,cutout"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _oracle_grads(o, kind, x, noise, u, policy, S, lam, iters):
    """CpuOTGAN.grads with T inserted: D(T(cat[x, G(z)])) in the critic step; D(T(x)) without grad and D(T(G(z))) with the
    gradient through T in the generator step.  Rows [0, nb) of u belong to the real batch, [nb, 2 nb) to the generated one."""
    nb = x.shape[0]
    if kind == "gen":
        x_gen = o.gen(noise)
        with torch.no_grad():
            f_dat = o.disc(R.apply(x, u[:nb], policy))
        f_gen = o.disc(R.apply(x_gen, u[nb:], policy))
        g_gen, _, dist, ent = o.match(f_gen, f_dat, S, lam, iters)
        return torch.autograd.grad(f_gen, o.params("generator"), g_gen), dist, ent
    with torch.no_grad():
        x_gen = o.gen(noise)
    f_all = o.disc(R.apply(torch.cat([x, x_gen], 0), u, policy))
    g_gen, g_dat, dist, ent = o.match(f_all[nb:], f_all[:nb], S, lam, iters)
    return torch.autograd.grad(f_all, o.params("discriminator"), torch.cat([g_dat, g_gen], 0)), dist, ent


@pytest.mark.parametrize("kind", ["disc", "gen"])
def test_step_gradients_match_oracle_with_augmentation(dev, kind):
    """The configuration and acceptance rule of tests/test_train_step_gpu.py::test_step_gradients_match_oracle (dcgan): each
    tensor < max(3e-2, 3 x the fp32 oracle's error), median < 5e-3, distance and entropy to 2e-4 relative.

    The critic's biases are given non-zero values first (the same in the step and in both oracles).  Cutout and translation
    fill whole regions of the critic's input with zeros; with the biases at their initial 0 every pre-activation inside such a
    region is EXACTLY zero in the oracle, on the kink of CReLU, where the derivative does not exist: autograd takes 0 for both
    halves, while a Winograd convolution leaves +-1e-8 there and opens one half.  The bias gradients of the first three critic
    layers move by 5 - 27 % when the oracle's zero regions are replaced by 1e-9 noise (nothing else moves, and nothing moves
    once the biases are non-zero: 3e-10), and the step's conv2d_1/b sat 7.7e-2 from the oracle for that reason alone.  A
    critic after its first update has no such ties."""
    from otgan_amd import ops
    from otgan_amd.trainer import OTGAN, default_args
    lam, iters = 100.0, 20
    args = default_args(model="dcgan", batch_size=3, nr_gpu=2, sinkhorn_lambda=lam, nr_sinkhorn_iter=iters,
                        nr_gen_per_disc=1, seed=7, augment=POLICY)
    m = OTGAN(args, dev)
    assert m.aug_policy == 7
    if kind == "gen":
        m.step_counter = 1
    gen = torch.Generator().manual_seed(11)
    x = torch.rand(m.nb, 32, 32, 3, generator=gen) * 2 - 1
    noise = torch.rand(m.nb, 100, generator=gen) * 2 - 1
    u = torch.rand(2 * m.nb, 8, generator=gen)
    with torch.no_grad():
        for k, v in m.discriminator.named_variables().items():
            if k.endswith("/b"):
                v.copy_((0.1 * torch.randn(v.shape, generator=gen)).to(dev))
    ops.bump_weights_epoch()
    r = m.step(x.to(dev), noise=noise.to(dev), aug=u.to(dev), apply_updates=False)
    assert r["kind"] == kind
    named = {}
    named.update(m.discriminator.named_variables())
    named.update(m.generator.named_variables())
    o = CpuOTGAN("dcgan", "crelu", dtype=torch.float64, use_c_matching=False)
    o.load(named)
    gr, dist, ent = _oracle_grads(o, kind, x.double(), noise.double(), u, 7, 2, lam, iters)
    o32 = CpuOTGAN("dcgan", "crelu", dtype=torch.float32, use_c_matching=False)
    o32.load(named)
    gr32, _, _ = _oracle_grads(o32, kind, x.float(), noise.float(), u, 7, 2, lam, iters)
    # T is far from the identity at these uniforms, on both halves (a step that skipped it would be an O(1) distance away)
    assert _rel(R.apply(x, u[:m.nb], 7), x) > 0.3 and _rel(R.apply(x, u[m.nb:], 7), x) > 0.3
    assert float(r["distance"]) == pytest.approx(dist, rel=2e-4, abs=1e-7)
    assert float(r["entropy"]) == pytest.approx(ent, rel=2e-4)
    names = list((m.generator if kind == "gen" else m.discriminator).named_variables())
    errs = []
    for n, a, b, c in zip(names, r["grads"], gr, gr32):
        e_hip, e_32 = _rel(a, b), _rel(c, b)
        errs.append(e_hip)
        assert e_hip < max(3e-2, 3 * e_32), (n, e_hip, e_32)
    print("%s step with augmentation: worst tensor %.3g, median %.3g" % (kind, max(errs), sorted(errs)[len(errs) // 2]))
    assert sorted(errs)[len(errs) // 2] < 5e-3, sorted(errs)[len(errs) // 2]
    m.close()


def _one_step(dev, kind, augment, aug, **kw):
    from otgan_amd.trainer import OTGAN, default_args
    args = default_args(model="dcgan", batch_size=3, nr_gpu=2, sinkhorn_lambda=100.0, nr_sinkhorn_iter=20, nr_gen_per_disc=1,
                        seed=7, augment=augment, **kw)
    m = OTGAN(args, dev)
    m.step_counter = 1 if kind == "gen" else 0
    gen = torch.Generator().manual_seed(11)
    x = (torch.rand(m.nb, 32, 32, 3, generator=gen) * 2 - 1).to(dev)
    noise = (torch.rand(m.nb, 100, generator=gen) * 2 - 1).to(dev)
    r = m.step(x, noise=noise, aug=aug(m.nb) if aug else None, apply_updates=False)
    out = (r["distance"].clone(), r["entropy"].clone(), [t.clone() for t in r["grads"]])
    m.close()
    return out


@pytest.mark.parametrize("ema_critic", [False, True], ids=["live", "ema"])
@pytest.mark.parametrize("kind", ["disc", "gen"])
def test_identity_transform_changes_nothing(dev, kind, ema_critic):
    """Translation only with a supplied zero shift (u3 = u4 = 0.5): T copies, and the step -- distance, entropy and every
    gradient -- has the bits of the step without --augment.  The wiring adds nothing but T."""
    def zero_shift(nb):
        u = torch.rand(2 * nb, 8, generator=torch.Generator().manual_seed(3))
        u[:, 3:5] = 0.5
        return u.to(dev)
    off = _one_step(dev, kind, "", None, train_disc_against_ema=ema_critic)
    on = _one_step(dev, kind, "translation", zero_shift, train_disc_against_ema=ema_critic)
    assert torch.equal(off[0], on[0]) and torch.equal(off[1], on[1])
    assert len(off[2]) == len(on[2]) and all(torch.equal(a, b) for a, b in zip(off[2], on[2]))


def _run(dev, graph, steps, ngd):
    """The small configuration of tests/test_step_graph_gpu.py with augmentation on."""
    from otgan_amd.trainer import OTGAN, default_args
    args = default_args(model="dcgan", batch_size=4, nr_gpu=2, sinkhorn_lambda=100.0, nr_sinkhorn_iter=20,
                        nr_gen_per_disc=ngd, seed=3, step_graph=graph, augment=POLICY)
    m = OTGAN(args, dev)
    g = torch.Generator().manual_seed(11)
    xs = [(torch.rand(m.nb, 32, 32, 3, generator=g) * 2 - 1).to(dev) for _ in range(4)]
    torch.manual_seed(7)
    dists = [m.step(xs[i % 4])["distance"].clone() for i in range(steps)]
    sd = m.state_dict(full=True)
    state = {k: v.clone() for k, v in sd.items() if torch.is_tensor(v)}
    state.update({"ema/" + k: v.clone() for k, v in sd["__ema__"].items()})
    captured = sorted(m.graphs.graphs) if m.graphs is not None else []
    dead = m.graphs.dead if m.graphs is not None else None
    m.close()
    return state, torch.stack(dists).cpu(), captured, dead


def test_replayed_steps_equal_eager_steps_with_augmentation(dev):
    """The draw of the uniforms happens inside the captured step, like the generator's latent: three periods and two steps,
    two of the periods replayed, end with the eager run's bits."""
    ngd = 2
    steps = 3 * (ngd + 1) + 2
    s0, d0, c0, _ = _run(dev, False, steps, ngd)
    s1, d1, c1, dead = _run(dev, True, steps, ngd)
    assert c0 == [] and dead is None and c1 == ["disc", "gen", "gen1"]
    assert torch.equal(d0, d1), (d0, d1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


def test_paths_outside_the_step_are_not_augmented(dev):
    """sample(), sample(ema=True) and critic_features() of models of the same seed with augmentation on and off, no step taken:
    identical bits, and nothing is drawn beyond what they draw today (the device's random stream ends at the same place)."""
    from otgan_amd.trainer import OTGAN, default_args
    x = (torch.rand(8, 32, 32, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev)
    got = []
    for augment in ("", POLICY):
        m = OTGAN(default_args(model="dcgan", batch_size=4, nr_gpu=2, nr_sinkhorn_iter=10, seed=5, augment=augment), dev)
        torch.manual_seed(9)
        got.append((m.sample(8).clone(), m.sample(8, ema=True).clone(), m.critic_features(x).clone(), torch.rand(4, device=dev)))
        m.close()
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_train_main_with_augmentation(tmp_path, capsys):
    from otgan_amd import train
    m = train.main(["--synthetic", "--synthetic_size", "64", "--batch_size", "4", "--nr_gpu", "2", "--nr_sinkhorn_iter", "10",
                    "--augment", POLICY, "--max_steps", "7", "--save_dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert m.step_counter == 7 and m.aug_policy == 7
    m.close()
    assert out.count("augmentation of the critic's inputs: color,translation,cutout (policy 7)") == 1
    line = [l for l in out.splitlines() if l.startswith("Iteration 0")]
    assert len(line) == 1
    vals = [float(v) for v in re.findall(r"= (-?[0-9.]+(?:e-?[0-9]+)?|nan|inf)", line[0].split("time")[1])][1:]
    assert len(vals) == 3 and all(math.isfinite(v) for v in vals), line
