"""Command-line training driver with the reference's flag set (reference train.py:14-33:
same names, types and defaults), one process per GPU:

    python train.py --model dcgan --nr_gpu 2 --batch_size 128 --data_dir /data ...
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 train.py --nr_gpu 16 --batch_size 128

`--nr_gpu` keeps the reference's meaning -- the number of equal feature shards of the
matching problem (it must be even, train.py:34) -- and is decoupled from the number of
physical GPUs (= torch.distributed world size): every rank owns nr_gpu / world shards.

Added flags (not in the reference): --synthetic (random CIFAR-shaped data instead of the
pickled dataset), --synthetic_size, --matching_scope global|local, --max_steps, --image_size (32 | 64, both models; the
reference is 32 x 32 only), --save_every,
--data_dependent_init, --eval_every / --eval_samples / --inception_model (the reference's Inception-score hook,
train.py:245-272: --inception_model takes the reference's own 2015 graph file, or a TorchScript classifier),
--fid_stats / --fid_real_samples (the Frechet Inception Distance beside every score, utils/fid.py),
--kid_subsets / --kid_subset_size / --kid_real_samples (the Kernel Inception Distance beside them, utils/kid.py),
--pr_neighbours / --pr_real_samples (precision, recall, density and coverage beside them, utils/pr.py),
--probe_every / --probe_neighbours / --probe_train_samples / --probe_test_samples (the critic's score: k-NN classification of
held-out labelled images in the critic's own features, utils/probe.py -- the measurement the reference loads its labels and
test set for, train.py:199, and leaves empty),
--dataset cifar10|imagenet64|npy and --data_on_device (utils/data.py): the training set lives on the device as uint8 and
one kernel launch per step gathers, flips and converts the step's batch; 64 x 64 data (the downsampled-ImageNet pickles, a
.npy of one's own images) comes in this way only.  Guarantee: `--dataset cifar10 --data_on_device` feeds `model.step` the
same bits as the default host path, step for step (same host and device random streams, same conversion table),
--augment color,translation,cutout (utils/augment.py, ops.augment: differentiable augmentation, Zhao et al. 2020 -- one random
colour / translation / cutout transform per image in front of every critic pass of a training step, real and generated, with
the generator's gradient taken through it; the lever against a critic that memorises a small training set.  Samples, metrics,
the probe and the initialisation pass are never augmented; '' = off, and the step is then the reference's bit for bit),
--swd_samples / --swd_patches / --swd_dirs / --swd_repeats (utils/swd.py: the sliced Wasserstein distance x 1e3 per
Laplacian-pyramid level between generated and training images, Karras et al. 2018 -- the one sample metric that needs no
--inception_model; at the --eval_every cadence, for the live and the EMA generator, without moving the training run),
--authenticity_samples / --authenticity_neighbours / --authenticity_train_samples (utils/authenticity.py: is the generator
copying the training set?  Exact pixel-space nearest training images of generated samples on the int8 matrix pipe, the
authenticity score of Alaa et al. 2022 beside a held-out baseline, and nn_sample<epoch>.png: the samples nearest to the
training set, each beside its nearest training images; same cadence, same fixed samples as --swd_samples),
--health_every N (utils/health.py: every N steps, and at the first later step of the other kind, one JSON line in
<save_dir>/health.jsonl -- gradient, parameter and update norms per variable, the share of every gradient below the 11 and 22
bits of the split-precision engine, the marginal residuals of the step's Sinkhorn plans -- and one `health:` line per epoch;
training is the same bit for bit; non-finite gradients are written and then raised before the optimiser runs).

Checkpoints (`<save_dir>/med_gan_params-<epoch>`, the reference's naming, train.py:275-277) are torch pickles
of {variable name: tensor} plus optimiser moments / step count and EMA shadows (which the reference's
Saver omits); they are not TensorFlow checkpoints.
"""
import argparse
import os
import pickle
import sys
import time

import numpy as np
import torch


def build_parser():
    p = argparse.ArgumentParser()
    # ---- reference flags (train.py:15-32), same defaults
    p.add_argument('--seed', type=int, default=1)
    p.add_argument('--batch_size', type=int, default=625)
    p.add_argument('--learning_rate_disc', type=float, default=0.0003)
    p.add_argument('--learning_rate_gen', type=float, default=0.0003)
    p.add_argument('--data_dir', type=str, default='/home/tim/data')
    p.add_argument('--save_dir', type=str, default='/local_home/tim/med_gan')
    p.add_argument('--optimizer', type=str, default='adam')
    p.add_argument('--nonlinearity', type=str, default='crelu')
    p.add_argument('--nr_gpu', type=int, default=8, help='How many equal shards (reference: GPUs) to split each step across?')
    p.add_argument('--nr_gen_per_disc', type=int, default=5, help='How many times to update the generator for each update of the discriminator?')
    p.add_argument('--sinkhorn_lambda', type=float, default=500.)
    p.add_argument('--nr_sinkhorn_iter', type=int, default=500)
    p.add_argument('--single_batch', dest='single_batch', action='store_true', help='Use simplified batching using a single batch instead of 2')
    p.add_argument('--train_disc_against_ema', dest='train_disc_against_ema', action='store_true', help='Should discriminator be trained against samples of EMA generator?')
    p.add_argument('--model', type=str, default='dcgan')
    p.add_argument('--load_params', dest='load_params', action='store_true')
    p.add_argument('--model_name', type=str, default='med_gan_params-2399')
    p.add_argument('--no_sinkhorn', dest='no_sinkhorn', action='store_true')
    # ---- additions
    p.add_argument('--synthetic', action='store_true', help='uniform random image_size x image_size x 3 data instead of CIFAR-10')
    p.add_argument('--matching_scope', type=str, default='global', choices=['global', 'local'])
    p.add_argument('--max_steps', type=int, default=0, help='stop after this many steps (0 = run like the reference)')
    p.add_argument('--image_size', type=int, default=32,
                   help='side of the generated / critic images: 32 (the reference) or 64 for --model dcgan and --model densenet; '
                        '64 needs data of 64, 128 or 256 pixels a side (--dataset imagenet64 | npy, or --synthetic: CIFAR-10 is 32x32)')
    p.add_argument('--save_every', type=int, default=200, help='checkpoint every this many epochs (reference: 200, train.py:275)')
    p.add_argument('--synthetic_size', type=int, default=50000, help='number of synthetic images with --synthetic')
    p.add_argument('--data_dependent_init', action='store_true',
                   help="run the reference's intended (never executed, SURVEY F7) data-dependent initialisation pass "
                        "on the first batch: g <- init_scale / std, b <- -mean * g per layer (utils/nn.py:133-162)")
    p.add_argument('--ranks', type=int, default=0,
                   help='processes (= GPUs) to run on when started plainly, without torchrun; 0 = as many of the visible '
                        'GPUs as divide --nr_gpu (the reference drives nr_gpu devices from one command, train.py:72-85)')
    p.add_argument('--eval_every', type=int, default=100, help='Inception score every this many epochs (reference: 100, train.py:245)')
    p.add_argument('--eval_samples', type=int, default=50000, help='samples per score (reference: 50000, train.py:262)')
    p.add_argument('--inception_model', type=str, default='',
                   help="the reference's 2015 Inception graph (classify_image_graph_def.pb, inception-2015-12-05.tgz or the "
                        'directory holding the .pb; runs on the GPU kernels) or a TorchScript classifier (float32 images '
                        '[n,H,W,3] in 0..255 -> class probabilities); without it the Inception-score hook is skipped')
    p.add_argument('--fid_stats', type=str, default='',
                   help="report the Frechet Inception Distance beside every Inception score, against the pool_3 statistics in "
                        "this .npz (keys mu, sigma: the circulated fid_stats_*.npz files load as they are); a missing file is "
                        "computed from the training set before the first step and saved there.  Needs the 2015 graph as "
                        "--inception_model.  '' = off")
    p.add_argument('--fid_real_samples', type=int, default=0,
                   help='training images behind a computed --fid_stats file: the first N (0 = all)')
    p.add_argument('--kid_subsets', type=int, default=0,
                   help='report the Kernel Inception Distance (utils/kid.py: unbiased, so comparable across --eval_samples) beside '
                        'every Inception score as the mean and std of the MMD^2 of this many random subsets of the generated and '
                        'the real pool_3 features (papers use 100).  Needs the 2015 graph as --inception_model.  0 = off')
    p.add_argument('--kid_subset_size', type=int, default=1000,
                   help='rows per KID subset and side; cut to the rows the smallest rank holds')
    p.add_argument('--kid_real_samples', type=int, default=0,
                   help='training images behind the real side of KID: the first N (0 = min(eval_samples, training images))')
    p.add_argument('--pr_neighbours', type=int, default=0,
                   help='report precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of '
                        'the generated against the real pool_3 features beside every Inception score (utils/pr.py), with balls '
                        'reaching to the K-th nearest neighbour (the papers use 3; at most 8).  Needs the 2015 graph as '
                        '--inception_model.  0 = off')
    p.add_argument('--pr_real_samples', type=int, default=0,
                   help='training images behind the real side of precision and recall: the first N (0 = min(eval_samples, '
                        'training images))')
    p.add_argument('--probe_every', type=int, default=0,
                   help="score the critic's features every this many epochs by k-NN classification of held-out labelled images "
                        "against training images in the critic's own cosine geometry (utils/probe.py; the reference's comment "
                        "says 50, train.py:199).  Needs a dataset with labels; 0 = off")
    p.add_argument('--probe_neighbours', type=int, default=5, help='neighbours that vote in the probe (1 ... 8)')
    p.add_argument('--probe_train_samples', type=int, default=5000, help='training images the probe searches: the first N')
    p.add_argument('--probe_test_samples', type=int, default=1000,
                   help='held-out images the probe classifies: the first N of test_batch / val_data (an .npz has no held-out '
                        'subset: its training images are classified leave-one-out)')
    p.add_argument('--step_graph', type=int, nargs='?', const=1, default=None, choices=(0, 1),
                   help='replay whole steps as hipGraphs after the first period (single-process runs; bit-identical to the '
                        'eager steps).  Default: on for --model densenet (launch-bound: replay 25.5 ms against 27.6 - 29.6 ms), '
                        'off for dcgan (8.60 against 8.52 - 8.56 ms); --step_graph / --step_graph 1 forces it on, --step_graph 0 off')
    p.add_argument('--dataset', type=str, default='cifar10', choices=['cifar10', 'imagenet64', 'npy'],
                   help='what --data_dir holds (utils/data.py): the CIFAR-10 python batches (the reference), the downsampled-ImageNet '
                        "64x64 batches train_data_batch_1 ... 10 (pickles or .npz), or one .npy / .npz file of uint8 [n, H, W, 3] images; "
                        'data whose side is 2x or 4x --image_size is box-downsampled on the device')
    p.add_argument('--data_on_device', action='store_true',
                   help='keep the training set on the device as uint8 and make every batch there in one launch (gather, flip, '
                        'uint8 -> [-1, 1]) instead of the per-step host gather and copy; the same batches bit for bit.  Implied by '
                        '--dataset imagenet64 | npy, which have no host-float path; with --synthetic: a random uint8 set')
    p.add_argument('--augment', type=str, default='',
                   help="differentiable augmentation of everything the critic sees in a training step (DiffAugment, Zhao et al. "
                        "2020): a comma-separated subset of color,translation,cutout in any order, e.g. "
                        "'color,translation,cutout'; the generator's gradient flows through the transform.  For small training "
                        "sets.  '' = off (the reference's step)")
    p.add_argument('--swd_samples', type=int, default=0,
                   help='report the sliced Wasserstein distance x 1e3 per Laplacian-pyramid level (Karras et al. 2018; '
                        'utils/swd.py) between this many generated and as many training images at the --eval_every cadence, for '
                        'the live and the EMA generator.  Needs no --inception_model.  The paper uses 16384; cut, with a notice, '
                        'to the number of training images.  0 = off')
    p.add_argument('--swd_patches', type=int, default=128, help='7 x 7 patches per image and pyramid level (the paper: 128)')
    p.add_argument('--swd_dirs', type=int, default=128, help='random directions per repeat (the paper: 128)')
    p.add_argument('--swd_repeats', type=int, default=4, help='repeats, each with fresh directions (the paper: 4)')
    p.add_argument('--authenticity_samples', type=int, default=0,
                   help='report the authenticity score (Alaa et al. 2022; utils/authenticity.py) of this many generated images '
                        'from their exact nearest training images in pixel space, at the --eval_every cadence, for the live and '
                        'the EMA generator, and write nn_sample<epoch>.png: the samples nearest to the training set beside their '
                        'nearest training images.  Needs no --inception_model.  0 = off')
    p.add_argument('--authenticity_neighbours', type=int, default=3,
                   help='nearest training images shown per sample on the sheet (1 ... 8); the score uses the first')
    p.add_argument('--authenticity_train_samples', type=int, default=50000,
                   help='training images that are searched: the first N')
    p.add_argument('--health_every', type=int, default=0,
                   help='every this many steps (and at the first later step of the other kind) append one JSON line to '
                        '<save_dir>/health.jsonl: gradient, parameter and update norms per variable, the share of every gradient '
                        'below the 11 and 22 bits of the split-precision engine, and the marginal residuals of the Sinkhorn plans '
                        '(utils/health.py); one summary line per epoch.  Training is the same bit for bit.  0 = off')
    return p


def uses_device_data(args):
    """The device-resident uint8 path (utils/data.py)?  --data_on_device, or a dataset that has no host-float loader."""
    return bool(args.data_on_device) or args.dataset != 'cifar10'


def inception_hook(model, args, classifier, state, rank=0, world=1):
    """train.py:245-272: scores of `eval_samples` samples of the generator and of its EMA copy, running maximum.
    Every rank takes part: it draws and classifies its share of the samples (its own latent stream, seed + rank) and
    the class probabilities are gathered, so no rank waits at the next epoch's first collective while rank 0 alone
    samples and scores 2 x 50 000 images.  All ranks get the same scores; rank 0 prints them.

    With the device classifier the same forward pass also feeds the metrics on pool_3 (utils.features.HookMetric), each
    on pool_3 of exactly the `eval_samples` samples the score covers -- this rank's `mine` rows that survive the cut:
    the Frechet Inception Distance with `state["fid_real"]` = (mu, sigma) (--fid_stats; fid.FidMetric), the Kernel
    Inception Distance with --kid_subsets > 0 and `state["kid_real"]` (real_kid_state; kid.KidMetric), and precision,
    recall, density and coverage with --pr_neighbours > 0 and `state["pr_real"]` / `state["pr_real_radii"]`
    (real_pr_state; pr.PrMetric).  The last two read the rows from one device feature bank, `state["kid_gen"]`, which
    is filled when either is on: allocated once per run, cleared per model."""
    from .utils.inception import class_probabilities, inception_score_from_probs
    from .utils import features
    from . import parallel
    on_device = hasattr(classifier, "probs_from_generator")    # utils.inception_net.InceptionNet: samples stay on the GPU
    share = features.share(args.eval_samples, 0, world)[1]     # every rank draws as many as rank 0 holds
    # the gather below is cut to eval_samples rows: of this rank's share the first `mine` survive
    lo, hi = features.share(args.eval_samples, rank, world)
    mine = hi - lo
    metrics = []
    if on_device:       # each metric is on with its flag and what its real_*_state left in `state`
        from .utils import fid, kid, pr
        for cls, flag in ((fid.FidMetric, True), (kid.KidMetric, getattr(args, "kid_subsets", 0) > 0),
                          (pr.PrMetric, getattr(args, "pr_neighbours", 0) > 0)):
            if flag and state.get(cls.key + "_real") is not None:
                metrics.append(cls(state[cls.key + "_real"], args, classifier, state, rank, world))
    bank = None
    if any(m.uses_bank for m in metrics):
        if "kid_gen" not in state or state["kid_gen"].buf.shape[0] < mine:      # one buffer for every evaluation of the run
            state["kid_gen"] = features.FeatureBank(mine, classifier.plan.pool3_channels, classifier.device, total=args.eval_samples)
        bank = state["kid_gen"]
    out = {}
    for tag, ema in (("", False), ("EMA ", True)):
        probs, have = [], 0
        for m in metrics:
            m.begin()
        if bank is not None:
            bank.clear()
        while have < share:
            x = model.sample(min(1000, share - have), ema=ema)
            if metrics:
                p, pool3 = classifier.probs_and_pool3_from_generator(x.float())
                probs.append(p)
                kept = pool3[:min(max(mine - have, 0), x.shape[0])]
                for m in metrics:
                    m.take(kept)
                if bank is not None:
                    bank.append(kept)
            elif on_device:
                probs.append(classifier.probs_from_generator(x.float()))                      # 127.5 (x + 1) folded in
            else:
                x = x.float().cpu().numpy()
                probs.append(class_probabilities([127.5 * (im + 1.) for im in x], classifier))   # train.py:260-262
            have += x.shape[0]
        if on_device:
            p = torch.cat(probs)[:share].float().to(model.device)
        else:
            p = torch.from_numpy(np.concatenate(probs)[:share].astype(np.float32)).to(model.device)
        p = parallel.all_gather_rows(p)[:args.eval_samples].cpu().numpy()
        score = inception_score_from_probs(p, splits=10)
        if rank == 0:
            print('%sinception score was %.6f, std was %.3f' % (tag, score[0], score[1]))
        if score[0] > state["max"]:
            state["max"], state["iter"] = score[0], state["epoch"]
        out[tag.strip() or "live"] = score
        for m in metrics:
            out[m.key + "_" + (tag.strip() or "live")] = m.finish(tag, bank)
    if rank == 0:
        print('max inception score was %.6f, iter was %d' % (state["max"], state["iter"]))
    for m in metrics:
        m.close()
    return out


def real_fid_stats(args, classifier, trainx, rank=0, world=1):
    """--fid_stats: (mu, sigma) of the real data's pool_3, loaded from the file or -- when rank 0 does not find it --
    computed by all ranks from the first --fid_real_samples training images and saved by rank 0.  None (said once) when
    the classifier is not the device network of the 2015 graph: FID is defined on its pool_3."""
    from . import parallel
    from .utils import fid
    if not _has_pool3(classifier, rank, '--fid_stats: FID needs', 'it is'):
        return None
    C = classifier.plan.pool3_channels
    there = torch.tensor([1.0 if os.path.exists(args.fid_stats) else 0.0], device=classifier.device)
    if float(parallel.broadcast_(there)):          # rank 0 decides: every rank takes the same branch
        mu, sigma, n = fid.load_stats(args.fid_stats, C)
        if rank == 0:
            print('FID statistics of the real data: loaded %s (%s)' % (args.fid_stats, '%d images' % n if n else 'n not recorded'))
        return mu, sigma
    x = _head(trainx, args.fid_real_samples) if args.fid_real_samples else trainx
    mu, sigma, n = fid.dataset_stats(classifier, x, rank, world)
    if rank == 0:
        fid.save_stats(args.fid_stats, mu, sigma, n)
        print('FID statistics of the real data: computed from %d training images, saved to %s' % (n, args.fid_stats))
    return mu, sigma


def _has_pool3(classifier, rank, needs, they_are):
    """Is the classifier the device network of the 2015 graph, whose pool_3 the metrics are defined on?  If not, rank 0
    says so once."""
    ok = hasattr(classifier, "probs_and_pool3_from_generator")
    if not ok and rank == 0:
        print('%s the 2015 Inception graph as --inception_model (%s defined on its pool_3); skipped' % (needs, they_are))
    return ok


def _head(trainx, n):
    """the first n training images (a utils.data.DeviceDataset has no slices: `head` shares its store)"""
    return trainx.head(n) if hasattr(trainx, "head") else trainx[:n]


def _real_features(args, classifier, trainx, rank, world, needs, they_are, samples, check, what, reuse=None):
    """The real side of a metric on feature banks: (pool_3 of the first `samples or eval_samples` training images as this
    rank's share of a device feature bank -- `reuse` when that bank holds the same images --, check(images)), or None
    when the classifier has no pool_3.  `check` raises, and says what it has to say, before anything is classified."""
    from .utils import features
    if not _has_pool3(classifier, rank, needs, they_are):
        return None
    n = min(samples or args.eval_samples, trainx.shape[0])
    checked = check(n)
    shared = reuse is not None and reuse.total == n
    bank = reuse if shared else features.real_bank(classifier, _head(trainx, n), n, rank, world)
    if rank == 0:
        print('%s features of the real data: pool_3 of the first %d training images, %s (%.1f MB per rank)'
              % (what, n, 'the bank KID keeps' if shared else 'kept on the device', bank.buf.numel() * 4 / 1e6))
    return bank, checked


def real_kid_state(args, classifier, trainx, rank=0, world=1):
    """--kid_subsets: what the hook keeps in its state for the Kernel Inception Distance -- {"kid_real": the pool_3 of the
    first --kid_real_samples training images as a device feature bank (this rank's share), "kid_m": the subset size in
    effect}.  Empty (said once) when the classifier is not the device network of the 2015 graph.  A subset size below 2
    is a ValueError before anything is classified."""
    from .utils import kid

    def subset_size(n):
        m = kid.effective_subset_size(args.kid_subset_size, args.eval_samples, n, world)
        if rank == 0 and m < args.kid_subset_size:
            print('KID subsets hold %d rows, not --kid_subset_size %d: the smallest rank has no more generated or real rows'
                  % (m, args.kid_subset_size))
        return m
    made = _real_features(args, classifier, trainx, rank, world, '--kid_subsets: KID needs', 'it is', args.kid_real_samples,
                          subset_size, 'KID')
    return {"kid_real": made[0], "kid_m": made[1]} if made else {}


def real_pr_state(args, classifier, trainx, rank=0, world=1, kid_bank=None):
    """--pr_neighbours: what the hook keeps in its state for precision, recall, density and coverage -- {"pr_real": the
    pool_3 of the first --pr_real_samples training images as a device feature bank (this rank's share; `kid_bank`, the
    bank KID keeps, when that holds the same images), "pr_real_radii": the K-th neighbour radius of every real row over
    all ranks, computed once}.  Empty (said once) when the classifier is not the device network of the 2015 graph.  A
    side with no more than K rows is a ValueError before anything is classified."""
    from .utils import pr
    made = _real_features(args, classifier, trainx, rank, world, '--pr_neighbours: precision and recall need', 'they are',
                          args.pr_real_samples, lambda n: pr.check_neighbours(args.pr_neighbours, args.eval_samples, n),
                          'precision / recall', kid_bank)
    return {"pr_real": made[0], "pr_real_radii": pr.radii(made[0].rows, made[1], rank, world)} if made else {}


def probe_state(args, trainx, dev, rank=0, world=1):
    """--probe_every: what the probe keeps for the run -- {"bank": the training set (the probe reads its first "n_bank"
    images), "bank_labels" / "query_labels": int64 on the device, "queries": the first --probe_test_samples held-out images
    as a uint8 device store (None: leave-one-out on the bank, an .npz has no held-out subset), "max" / "iter": the running
    best}.  None, said once by rank 0, for data without labels and for --synthetic: the run trains as without the flag.
    A bank with no more than K rows is a ValueError here, before the first step."""
    from .utils import data as udata, probe
    say = print if rank == 0 else (lambda *a: None)
    if args.synthetic:
        say('--probe_every: --synthetic data has no labels; the critic k-NN probe is skipped')
        return None
    labels = udata.load_labels(args.dataset, args.data_dir)
    if labels is None:
        say('--probe_every: %s carries no labels; the critic k-NN probe is skipped' % args.data_dir)
        return None
    n_bank = min(args.probe_train_samples, trainx.shape[0])
    probe.check_neighbours(args.probe_neighbours, n_bank)
    state = {"bank": trainx, "n_bank": n_bank, "bank_labels": torch.from_numpy(labels[:n_bank]).to(dev), "queries": None,
             "query_labels": None, "max": -1.0, "iter": 0}
    if args.dataset == 'npy':
        say('--probe_every: an .npz has no held-out subset; the first %d training images are classified leave-one-out' % n_bank)
        return state
    held_labels = udata.load_labels(args.dataset, args.data_dir, 'test')
    if held_labels is None:
        say('--probe_every: the held-out subset under %s carries no labels; the critic k-NN probe is skipped' % args.data_dir)
        return None
    held = udata.load_u8(args.dataset, args.data_dir, 'test')[:max(args.probe_test_samples, 0)]
    if held.shape[0] == 0:
        raise ValueError("--probe_test_samples %d: the probe needs at least one held-out image" % args.probe_test_samples)
    state["queries"] = udata.DeviceDataset(held, dev, args.image_size)
    state["query_labels"] = torch.from_numpy(held_labels[:held.shape[0]]).to(dev)
    return state


def probe_hook(model, args, state, rank=0, world=1):
    """The critic's score (utils/probe.py): k-NN classification of the held-out images against the first training images in
    the critic's features of this moment.  Every rank takes part: it runs the critic over its share of both sets
    (OTGAN.critic_features, in batches of at most OTGAN.PROBE_BATCH rows of its share, unflipped, in storage order), the
    bank is gathered and the counts are summed; rank 0 prints.  Training is untouched: no random draw, no parameter
    written."""
    from .utils import features, probe

    def feats(images, lo, hi):
        out = [torch.empty(0, model.num_features, device=model.device)]
        for i in range(lo, hi, model.PROBE_BATCH):
            j = min(i + model.PROBE_BATCH, hi)
            if hasattr(images, "rows"):
                x = images.rows(i, j)
            else:
                x = torch.from_numpy(np.ascontiguousarray(images[i:j], np.float32)).to(model.device)
            out.append(model.critic_features(x))
        return torch.cat(out)

    k = args.probe_neighbours
    lo, hi = features.share(state["n_bank"], rank, world)
    bank, bank_labels = feats(state["bank"], lo, hi), state["bank_labels"][lo:hi]
    if state["queries"] is None:
        right_k, right_1, n = probe.accuracy(bank, bank_labels, None, None, k, rank, world, leave_one_out=True)
    else:
        qlo, qhi = features.share(state["queries"].shape[0], rank, world)
        right_k, right_1, n = probe.accuracy(bank, bank_labels, feats(state["queries"], qlo, qhi),
                                             state["query_labels"][qlo:qhi], k, rank, world)
    acc = right_k / n
    if rank == 0:
        print('critic k-NN accuracy was %.4f (K = %d), 1-NN was %.4f, %d held-out against %d training images'
              % (acc, k, right_1 / n, n, state["n_bank"]))
    if acc > state["max"]:
        state["max"], state["iter"] = acc, state["epoch"]
        if rank == 0:
            print('max critic k-NN accuracy was %.4f, iter was %d' % (state["max"], state["iter"]))
    return acc, right_1 / n


def swd_state(args, trainx, dev, rank=0, world=1):
    """--swd_samples: what the sliced Wasserstein hook keeps for the run -- {"real": utils.swd.SwdReal, the sorted projections
    of the first n training images on this rank's contiguous share of the --swd_repeats x --swd_dirs directions, "n",
    "swd_min" / "swd_iter"}.  Positions (separate draws for the real and the generated side) and directions come ONCE per run
    from a private host generator seeded with --seed, the same on every rank, so evaluations are comparable across epochs; no
    draw touches the run's own random streams.  An image size without a pyramid is a ValueError here, before the first step."""
    from .utils import features, swd
    swd.levels(args.image_size)
    n = min(args.swd_samples, trainx.shape[0])
    if rank == 0 and n < args.swd_samples:
        print('--swd_samples %d: cut to the %d training images' % (args.swd_samples, n))
    if hasattr(trainx, "rows"):      # the stored uint8 where the store is what the model sees, the quantised rows otherwise
        real = trainx.store[:n] if trainx.factor == 1 else torch.cat(
            [swd.quantise(trainx.rows(i, min(i + 1000, n))) for i in range(0, n, 1000)])
    else:
        real = torch.from_numpy(swd.quantise(trainx[:n])).to(dev)
    g = torch.Generator().manual_seed(args.seed)
    pos_real = swd.positions(n, args.image_size, args.swd_patches, g)
    pos_gen = swd.positions(n, args.image_size, args.swd_patches, g)
    dirs = swd.directions(args.swd_repeats, args.swd_dirs, g)
    made = swd.SwdReal(real, pos_real, dirs, pos_gen=pos_gen, dir_range=features.share(dirs.shape[0], rank, world))
    if rank == 0:
        print('sliced Wasserstein distance: %d generated against %d training images, %d patches per image and level, %d '
              'directions, %d levels; sorted projections of the real side kept on the device (%.1f MB per rank)'
              % (n, n, args.swd_patches, dirs.shape[0], made.L, made.nbytes / 1e6))
    return {"real": made, "n": n}


def swd_hook(model, args, state, rank=0, world=1):
    """The sliced Wasserstein distance of the live and the EMA generator against the training images (utils/swd.py), whether or
    not there is an --inception_model.  Every rank takes part: it samples its share of the images (swd.sample_images: fixed
    latents, the device generator's state saved and restored, so the training run does not move), the uint8 images are
    gathered, each rank computes its share of the directions and the table is gathered; all ranks get the same numbers, rank 0
    prints them."""
    from .utils import swd
    metric = swd.SwdMetric(state["real"], args, state, rank, world)
    out = {}
    for tag, ema in (("", False), ("EMA ", True)):
        images = swd.sample_images(model, state["n"], args.seed, ema=ema, rank=rank, world=world)
        out[tag.strip() or "live"] = metric.evaluate(images, tag)
    metric.close()
    return out


def _u8_at_model_size(trainx, n, dev):
    """The first n training images as the model sees them, uint8 on the device: the stored uint8 where the store is what the
    model sees, the quantised rows otherwise (as swd_state)."""
    from .utils import swd
    if hasattr(trainx, "rows"):
        return trainx.store[:n] if trainx.factor == 1 else torch.cat(
            [swd.quantise(trainx.rows(i, min(i + 1000, n))) for i in range(0, n, 1000)])
    return torch.from_numpy(swd.quantise(trainx[:n])).to(dev)


def authenticity_state(args, trainx, dev, rank=0, world=1):
    """--authenticity_samples: what the authenticity hook keeps for the run -- {"bank": the first
    --authenticity_train_samples training images as uint8 on the device, "radii": each one's squared distance to its nearest
    other bank image (computed once, every rank its share), "held": the score of the first held-out images (cifar10 /
    imagenet64; None for npy and --synthetic, said once), "n"}.  A bank of fewer than 2 images is a ValueError here, before
    the first step."""
    from .utils import authenticity, data as udata
    n_bank = min(args.authenticity_train_samples, trainx.shape[0])
    if n_bank < 2:
        raise ValueError("--authenticity_samples needs a bank of at least 2 training images: it has %d" % n_bank)
    bank = _u8_at_model_size(trainx, n_bank, dev)
    radii = authenticity.radii(bank, rank, world)
    state = {"bank": bank, "radii": radii, "n": args.authenticity_samples, "held": None}
    if rank == 0:
        print('authenticity: %d generated against %d training images, %d of which have an exact duplicate among them'
              % (args.authenticity_samples, n_bank, int((radii == 0).sum())))
    if args.synthetic or args.dataset == 'npy':
        if rank == 0:
            print('--authenticity_samples: %s has no held-out subset; the authenticity score is printed without a held-out '
                  'baseline' % ('--synthetic data' if args.synthetic else args.data_dir))
        return state
    held = udata.load_u8(args.dataset, args.data_dir, 'test')[:args.authenticity_samples]
    held = _u8_at_model_size(udata.DeviceDataset(np.ascontiguousarray(held), dev, args.image_size), held.shape[0], dev)
    metric = authenticity.AuthenticityMetric(bank, radii, {}, rank, world)
    state["held"] = m = metric.measure(held)
    if rank == 0:
        print('held-out authenticity was %.4f, median nearest distance was %.2f, exact copies %d, %d held-out against %d '
              'training images' % (m["authentic"] / m["n"], authenticity.rms(m["median"], metric.D), m["copies"], m["n"], n_bank))
    return state


def authenticity_hook(model, args, state, rank=0, world=1):
    """The authenticity of the live and the EMA generator against the training images (utils/authenticity.py), whether or not
    there is an --inception_model.  The samples are swd.sample_images' (fixed latents, the device generator's state saved and
    restored: the training run does not move); each rank searches its share of them, all ranks get the same numbers, rank 0
    prints them and writes the nearest-neighbour sheets."""
    from .utils import authenticity, swd
    metric = authenticity.AuthenticityMetric(state["bank"], state["radii"], state, rank, world, held=state["held"])
    out = {}
    for tag, ema in (("", False), ("EMA ", True)):
        images = swd.sample_images(model, state["n"], args.seed, ema=ema, rank=rank, world=world)
        out[tag.strip() or "live"] = m = metric.evaluate(images, tag, k=args.authenticity_neighbours)
        if rank == 0:
            authenticity.save_png(authenticity.sheet(images, state["bank"], m["index"], m["dist"]),
                                  os.path.join(args.save_dir, '%snn_sample%d.png' % ('ema_' if ema else '', state["epoch"])))
    metric.close()
    return out


def load_cifar(data_dir, subset='train'):
    """Pickled CIFAR-10 python batches under <data_dir>/cifar-10-python/cifar-10-batches-py
    (the layout the reference's data/cifar10_data.py:40-53 reads; no download here)."""
    d = os.path.join(data_dir, 'cifar-10-python', 'cifar-10-batches-py')
    files = ['data_batch_%d' % i for i in range(1, 6)] if subset == 'train' else ['test_batch']
    xs = []
    for f in files:
        with open(os.path.join(d, f), 'rb') as fo:
            e = pickle.load(fo, encoding='latin1')
        xs.append(np.asarray(e['data']).reshape(-1, 3, 32, 32))
    x = np.concatenate(xs, 0)
    return np.transpose(x, (0, 2, 3, 1)).astype(np.float32) / 127.5 - 1.     # train.py:158


def maybe_flip(x):
    """Random horizontal flip per image (train.py:163-170), on the device."""
    flip = torch.rand(x.shape[0], device=x.device) < 0.5
    return torch.where(flip[:, None, None, None], x.flip(2), x)


def save_tile_png(x, path, n=100):
    """10x10 sample sheet (the role of utils/plotting.py:9-13,29-74)."""
    try:
        from PIL import Image
    except ImportError:
        return
    x = x[:n].clamp(-1, 1).add(1).mul(127.5).byte().cpu().numpy()
    k = int(np.ceil(np.sqrt(x.shape[0])))
    H, W = x.shape[1:3]
    sheet = np.full((k * (H + 1) + 1, k * (W + 1) + 1, 3), 255, np.uint8)
    for i, im in enumerate(x):
        r, c = divmod(i, k)
        sheet[1 + r * (H + 1):1 + r * (H + 1) + H, 1 + c * (W + 1):1 + c * (W + 1) + W] = im
    Image.fromarray(sheet).save(path)


def auto_ranks(nr_gpu, devices, scope='global'):
    """Largest rank count <= devices that divides the nr_gpu logical shards (and is even or 1 in the global matching
    scope, where a rank's rows must lie inside one mini-batch half; an even shard count per rank in the local one)."""
    for r in range(min(devices, nr_gpu), 0, -1):
        if nr_gpu % r == 0 and ((r == 1 or r % 2 == 0) if scope == 'global' else (nr_gpu // r) % 2 == 0):
            return r
    return 1


def main(argv=None, self_launch=False):
    """`self_launch`: set by the command-line entry points (train.py at the repository root, `python -m`): the plain
    invocation drives every visible device.  An in-process caller (a test, a notebook) gets a single-rank run in its
    own process unless it passes --ranks explicitly -- never a surprise SystemExit."""
    args = build_parser().parse_args(argv)
    assert args.nr_gpu % 2 == 0                                   # train.py:34
    from .utils import probe
    try:
        probe.check_neighbours(args.probe_neighbours)
    except ValueError as e:
        raise ValueError("--probe_neighbours: %s" % e) from None
    from .utils import augment
    try:
        policy = augment.parse_policy(args.augment)
    except ValueError as e:
        raise ValueError("--augment: %s" % e) from None
    if args.authenticity_samples > 0:
        from .utils import authenticity
        try:
            authenticity.check_neighbours(args.authenticity_neighbours)
        except ValueError as e:
            raise ValueError("--authenticity_neighbours: %s" % e) from None
    from .utils import health
    health.check_every(args.health_every)
    from . import parallel
    from .trainer import OTGAN
    if not parallel.launched() and (self_launch or args.ranks):
        # one command drives every device, like the reference's tower loop (train.py:72-85): a rank is a process
        # here, so the plain invocation re-executes itself under torch.distributed.run
        want = args.ranks or auto_ranks(args.nr_gpu, torch.cuda.device_count() if torch.cuda.is_available() else 0,
                                        args.matching_scope)
        if want > 1:
            script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'train.py')
            try:
                sys.exit(parallel.self_launch(script, sys.argv[1:] if argv is None else list(argv), want))
            except parallel.LaunchError as e:
                sys.exit('train.py --ranks %d: %s' % (want, e))
    rank, world, local = parallel.init_from_env()
    if not torch.cuda.is_available():
        raise RuntimeError("training needs MI355X GPUs: there is no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if rank == 0:
        print(args)
    np.random.seed(args.seed)                                      # train.py:48
    torch.manual_seed(args.seed + rank)
    on_device = uses_device_data(args)
    if on_device:
        # the set as uint8 on the device (every rank holds all of it); an --image_size the data cannot feed is a ValueError here
        from .utils import data as udata
        if args.synthetic:
            u8 = np.random.randint(0, 256, (args.synthetic_size, args.image_size, args.image_size, 3), dtype=np.uint8)
        else:
            u8 = udata.load_u8(args.dataset, args.data_dir)
        trainx = udata.DeviceDataset(u8, dev, args.image_size)
        del u8
        init_batch = trainx.rows(0, min(args.batch_size, trainx.shape[0])) if args.data_dependent_init else None
    else:
        if args.synthetic:
            trainx = np.random.rand(args.synthetic_size, args.image_size, args.image_size, 3).astype(np.float32) * 2 - 1
        else:
            trainx = load_cifar(args.data_dir)
        init_batch = torch.from_numpy(trainx[:args.batch_size]) if args.data_dependent_init else None
    model = OTGAN(args, dev, init_batch=init_batch)
    if rank == 0:
        print("model has a hidden representation with %d features" % model.num_features)   # train.py:56
        print("augmentation of the critic's inputs: %s (policy %d)" % (",".join(augment.policy_names(policy)) or "off", policy))

    per_step = args.nr_gpu * args.batch_size
    nr_batches = trainx.shape[0] // per_step                        # train.py:159
    if rank == 0:
        os.makedirs(args.save_dir, exist_ok=True)
    current_epoch = 0
    if args.load_params:                                           # train.py:190-193
        sd = torch.load(os.path.join(args.save_dir, args.model_name), map_location='cpu')
        model.load_state_dict(sd)
        current_epoch = int(args.model_name[args.model_name.rfind('-') + 1:])
    health_state = {"epoch": current_epoch, "gen": None, "disc": None}      # the last reported pair of steps
    if args.health_every > 0:
        def health_sink(record):
            record["epoch"] = health_state["epoch"]
            health_state[record["kind"]] = record
            if rank == 0:
                health.append(os.path.join(args.save_dir, 'health.jsonl'), record)
        model.health_sink = health_sink
    if rank == 0:
        print('starting training')
    mean_dist_gen, mean_dist_disc = [], []
    classifier, score_state = None, {"max": 0.0, "iter": 0, "epoch": 0}
    if args.inception_model:      # on every rank: each classifies its share of the samples
        from .utils.inception import load_classifier
        classifier = load_classifier(args.inception_model, dev)
    elif rank == 0:
        print('no --inception_model: the Inception-score hook (reference train.py:245-272) is skipped')
    if args.fid_stats:
        score_state["fid_real"] = real_fid_stats(args, classifier, trainx, rank, world)
    if args.kid_subsets > 0:
        score_state.update(real_kid_state(args, classifier, trainx, rank, world))
    if args.pr_neighbours > 0:
        score_state.update(real_pr_state(args, classifier, trainx, rank, world, score_state.get("kid_real")))
    probe_st = probe_state(args, trainx, dev, rank, world) if args.probe_every > 0 else None
    swd_st = swd_state(args, trainx, dev, rank, world) if args.swd_samples > 0 else None
    auth_st = authenticity_state(args, trainx, dev, rank, world) if args.authenticity_samples > 0 else None
    start_time = time.time()
    total = 0
    for epoch in range(current_epoch, 1000000):
        begin = time.time()
        health_state["epoch"] = epoch
        inds = np.random.permutation(trainx.shape[0])              # same seed on every rank
        if on_device:
            trainx.set_permutation(inds)
        dg, dd, ent = [], [], []
        for t in range(nr_batches):
            # shard s of this step reads rows (t + s*nr_batches)*B ... (train.py:209-211)
            if on_device:
                # the draw of maybe_flip (same device stream position), applied inside the gather
                flip = torch.rand(model.shards * args.batch_size, device=dev) < 0.5
                offs = [(t + (rank * model.shards + j) * nr_batches) * args.batch_size for j in range(model.shards)]
                r = model.step(trainx.batch(offs, args.batch_size, flip))
            else:
                rows = []
                for j in range(model.shards):
                    s = rank * model.shards + j
                    td = t + s * nr_batches
                    rows.append(inds[td * args.batch_size:(td + 1) * args.batch_size])
                xb = torch.from_numpy(trainx[np.concatenate(rows)]).to(dev, non_blocking=True)
                r = model.step(maybe_flip(xb))
            (dd if r["kind"] == "disc" else dg).append(r["distance"])
            ent.append(r["entropy"])
            total += 1
            if args.max_steps and total >= args.max_steps:
                break
        model.check_finite()        # one sync per logging interval (a failed Sinkhorn launch poisons the scalars)
        f = lambda lst: float(torch.stack([z.double() for z in lst]).mean()) if lst else float('nan')
        mean_dist_gen.append(f(dg))
        mean_dist_disc.append(f(dd))
        if classifier is not None and (epoch + 1) % args.eval_every == 0 and epoch != current_epoch:   # train.py:245
            score_state["epoch"] = epoch
            inception_hook(model, args, classifier, score_state, rank, world)
        if probe_st is not None and (epoch + 1) % args.probe_every == 0 and epoch != current_epoch:
            probe_st["epoch"] = epoch
            probe_hook(model, args, probe_st, rank, world)
        if swd_st is not None and (epoch + 1) % args.eval_every == 0 and epoch != current_epoch:
            swd_st["epoch"] = epoch
            swd_hook(model, args, swd_st, rank, world)
        if auth_st is not None and (epoch + 1) % args.eval_every == 0 and epoch != current_epoch:
            auth_st["epoch"] = epoch
            authenticity_hook(model, args, auth_st, rank, world)
        if rank == 0:
            print("Iteration %d, time = %ds, train distance before gen = %.6f, train distance before disc = %.6f, "
                  "avg matching entropy = %.6f" % (epoch, time.time() - begin, mean_dist_gen[-1],
                                                   mean_dist_disc[-1], f(ent)))          # train.py:231
            if args.health_every > 0 and (health_state["gen"] or health_state["disc"]):
                print(health.summary_line(health_state))
            save_tile_png(model.sample(100), os.path.join(args.save_dir, 'sample%d.png' % epoch))
            save_tile_png(model.sample(100, ema=True), os.path.join(args.save_dir, 'ema_sample%d.png' % epoch))
            if (epoch + 1) % args.save_every == 0 and epoch != current_epoch:                          # train.py:275-277
                torch.save(model.state_dict(), os.path.join(args.save_dir, 'med_gan_params-%d' % epoch))
                np.savez(os.path.join(args.save_dir, 'distances.npz'), mean_dist_gen=np.array(mean_dist_gen),
                         mean_dist_disc=np.array(mean_dist_disc))
                print('current epoch %d, elapsed hours from start epoch %.3f, total updates %d' % (
                    epoch, (time.time() - start_time) / 3600, model.step_counter))
            sys.stdout.flush()
        if args.max_steps and total >= args.max_steps:
            break
    return model


if __name__ == '__main__':
    main(self_launch=True)
