"""Hand-offs (ops.leave / take / forget): values that ride on a tensor from the autograd node that produced it to the one
that consumes it, valid for as long as the tensor's version counter stands still.  Host logic only: CPU tensors, no
library call."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from otgan_amd import ops  # noqa: E402


def test_a_left_value_is_returned_until_torch_writes_the_tensor():
    t, rec = torch.zeros(4, 8), torch.ones(3)
    assert ops.take(t, "amax") is None and ops.amax_of(t) is None and ops.colsum_of(t) is None
    assert ops.leave(t, "amax", rec) is t
    assert ops.take(t, "amax") is rec and ops.amax_of(t) is rec
    assert ops.take(t, "amax") is rec                      # reading does not remove
    t.add_(1.0)                                            # a torch in-place op: everything left on the tensor is stale
    assert ops.take(t, "amax") is None and ops.amax_of(t) is None


def test_kinds_of_one_version_live_together_and_a_newer_version_drops_the_older():
    t, rec, cs, rec2 = torch.zeros(4, 8), torch.ones(3), torch.ones(8), torch.full((3,), 2.0)
    ops.tag_amax(t, rec)
    ops.leave(t, "colsum", cs)                             # same version: the first kind stays
    assert ops.amax_of(t) is rec and ops.colsum_of(t) is cs
    t.mul_(2.0)
    ops.tag_amax(t, rec2)                                  # left at a newer version: the older kinds are gone
    assert ops.amax_of(t) is rec2
    assert ops.colsum_of(t) is None and ops.take(t, "colsum") is None


def test_the_removing_form_removes_one_kind_and_forget_drops_all():
    t, rec, cs = torch.zeros(4, 8), torch.ones(3), torch.ones(8)
    ops.tag_amax(t, rec)
    ops.leave(t, "colsum", cs)
    assert ops.take(t, "colsum", remove=True) is cs
    assert ops.take(t, "colsum") is None and ops.take(t, "colsum", remove=True) is None
    assert ops.amax_of(t) is rec                           # the other kind is untouched
    ops.leave(t, "glu", cs)
    ops.forget(t)
    assert ops.amax_of(t) is None and ops.take(t, "glu") is None
    ops.forget(t)                                          # nothing left: still fine


def test_views_carry_nothing_unless_told_and_share_the_counter_of_their_base():
    base, rec = torch.zeros(4, 8), torch.ones(3)
    ops.tag_amax(base, rec)
    v = base.view(2, 16)
    assert ops.amax_of(v) is None                          # a view is another tensor object
    assert ops.carry_amax(v, base) is v and ops.amax_of(v) is rec
    base.add_(1.0)                                         # the base is written in place afterwards
    assert ops.amax_of(v) is None and ops.amax_of(base) is None
    ops.tag_amax(base, rec)
    w = base[:, :4]
    assert ops.amax_of(ops.carry_amax(w, base)) is rec
    base[:, 4:].fill_(1.0)                                 # ... or a sibling view is (ExtendChannelsFunction's copies)
    assert ops.amax_of(w) is None and ops.amax_of(base) is None
    # nothing to carry: the destination stays without a record
    assert ops.amax_of(ops.carry_amax(torch.zeros(2), torch.zeros(2))) is None
