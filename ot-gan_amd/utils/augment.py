"""Differentiable augmentation of the critic's inputs (Zhao et al. 2020, "Differentiable Augmentation for Data-Efficient GAN
Training"): the policy string of `--augment` and the per-image uniforms the kernels of csrc/augment.hip derive their
parameters from (include/otgan_layers.h states the formulas; ops.augment is the autograd op)."""
import torch

POLICIES = {"color": 1, "translation": 2, "cutout": 4}      # ops.AUG_*; the names are DiffAugment's own
SLOTS = 8           # floats per image: b, ks, kc | tx, ty | ox, oy | unused


def parse_policy(text):
    """'color,translation,cutout' (any order, any subset, '' = off) -> the kernels' bit mask."""
    mask = 0
    for name in (text or "").split(","):
        name = name.strip()
        if not name:
            continue
        if name not in POLICIES:
            raise ValueError("unknown augmentation %r in %r: the valid names are %s"
                             % (name, text, ", ".join(sorted(POLICIES, key=POLICIES.get))))
        mask |= POLICIES[name]
    return mask


def policy_names(mask):
    """The names of the groups in `mask`, in the order they are applied."""
    return [n for n, bit in sorted(POLICIES.items(), key=lambda kv: kv[1]) if mask & bit]


def draw(rows, device):
    """[rows, 8] uniforms in [0, 1) from the device's default random stream (train.py seeds it with seed + rank): one row
    per image."""
    return torch.rand(rows, SLOTS, device=device)
