"""CPU restatement (torch, fp16) of the gate-sparsity hook and its counts, the checker of tests/test_sparsity_host.py
(pinned there to the reference's own receiver through the tests/golden/sparsity_* fixtures) and of
tests/test_gpu_sparsity.py.

  hook           SparsityMeasure.hook_fn: proj -> chunk -> act(gate); returns (value * act(gate), act(gate), the
                 pre-activation gate)
  counts         (elements with |gate| <= threshold in fp32, elements with gate < 0) of an activated gate
  ratio_fp32     the reference driver's formula (sparsity/check_sparsity.py:41-45): exact zeros per row / F in fp32,
                 then the fp32 mean over the tokens
  group_counts   the port's prompt batches: per group of images, per-neuron and total counts
Shared helpers (fixtures, tokens, weights) come from tests/neuron_ref.py: the sparsity fixtures use the same seeding.
"""
import torch
import torch.nn.functional as F

from neuron_ref import act_fn, golden, synth, tokens, weights  # noqa: F401


def hook(x, w, b, act):
    value, pre = F.linear(x, w, b).chunk(2, dim=-1)
    gate = act_fn(act)(pre)
    return value * gate, gate, pre


def counts(gate, threshold=0.0):
    g = gate.float()
    return int((g.abs() <= torch.tensor(threshold, dtype=torch.float32)).sum()), int((g < 0).sum())


def ratio_fp32(gate):
    mask = gate == 0.0
    return (mask.int().sum(-1).float() / gate.shape[-1]).mean().item()


def group_counts(gate, img_group, ngroups, threshold=0.0):
    """gate [nimg, N, F] -> (zero [ngroups, F], neg [ngroups, F], totals [ngroups, 2]) as int64 tensors."""
    g = gate.float()
    thr = torch.tensor(threshold, dtype=torch.float32, device=gate.device)
    zero, neg = [], []
    for k in range(ngroups):
        imgs = [i for i, gi in enumerate(img_group) if gi == k]
        sel = g[imgs].reshape(-1, g.shape[-1])
        zero.append((sel.abs() <= thr).sum(0))
        neg.append((sel < 0).sum(0))
    zero, neg = torch.stack(zero), torch.stack(neg)
    return zero, neg, torch.stack([zero.sum(1), neg.sum(1)], 1)
