"""CPU restatement (torch, fp16) of the neuron-level hooks, the checker of tests/test_neuron_host.py (pinned there to
the reference's own hooks through the tests/golden/neuron_* fixtures) and of tests/test_gpu_neurons.py.

  pred_hook      NeuronPredictivity / NeuronPredictivityBB.hook_fn: proj -> chunk -> act(gate); the column maximum of
                 the activated gate over every token (or the bounding-box positions of every image); value * gate
  remove_hook    RemoveNeurons.hook_fn: gate[..., mask == 1] = -0.17 before the product
  group_max      the port's prompt batches: the maximum per group of images (and positions)
Shared helpers regenerate the fixtures' modules and tokens from their seeds (tests/golden/synth.py).
"""
import glob
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLD not in sys.path:
    sys.path.insert(0, GOLD)
import synth  # noqa: E402

OVERRIDE = -0.17


def golden(kind):
    out = []
    for f in sorted(glob.glob(os.path.join(GOLD, "*.npz"))):
        with np.load(f, allow_pickle=False) as z:
            if str(z["kind"]) == kind:
                out.append((os.path.basename(f)[:-4], {k: z[k] for k in z.files}))
    return out


def x_seed(seed, prompt, kind, call):
    """Seed of the tokens of hooked call `call` of prompt `prompt` (kind 0 = base, 1 = adj) in the fixtures."""
    return seed + 1000 + (prompt * 2 + kind) * 100 + call


def tokens(c, prompt, kind, call, nimg=2):
    return torch.from_numpy(synth.tokens((nimg, int(c["N"]), int(c["C"])), x_seed(int(c["seed"]), prompt, kind,
                                                                                    call))).half()


def weights(c, l):
    """fp16 (w [8C, C], b [8C]) of the fixture's module l."""
    w, b = synth.geglu_weights(int(c["C"]), int(c["seed"]) + l, float(c["gate_bias"]))
    return torch.from_numpy(w).half(), torch.from_numpy(b).half()


def act_fn(act):
    return F.relu if act == "relu" else F.gelu


def valid_box(bb, seq_len):
    """The positions a bounding box selects, or None where the receivers fall back to all tokens."""
    if bb is None:
        return None
    idx = [int(i) for i in bb]
    if not idx or any(i < -seq_len or i >= seq_len for i in idx):
        return None
    return [i % seq_len for i in idx]


def pred_hook(x, w, b, act, bb=None):
    """(value * act(gate), column maximum of act(gate) over all tokens / the box positions of every image)."""
    value, gate = F.linear(x, w, b).chunk(2, dim=-1)
    gate = act_fn(act)(gate)
    box = valid_box(bb, x.shape[1])
    sel = gate if box is None else gate[:, box, :]
    return value * gate, torch.max(sel.reshape(-1, gate.shape[-1]), dim=0)[0]


def remove_hook(x, w, b, act, mask):
    """(value * gate', gate') with gate' = act(gate), -0.17 where mask == 1 (an empty mask: no override)."""
    value, gate = F.linear(x, w, b).chunk(2, dim=-1)
    gate = act_fn(act)(gate)
    mask = np.asarray(mask).reshape(-1)
    if mask.size:
        gate[..., torch.from_numpy(np.flatnonzero(mask != 0))] = OVERRIDE
    return value * gate, gate


def group_max(gate, img_group, ngroups, positions=None):
    """gate [nimg, N, F] -> [ngroups, F]: the maximum over the images of each group (positions: only those tokens)."""
    sel = gate if positions is None else gate[:, positions, :]
    out = []
    for g in range(ngroups):
        imgs = [i for i, gi in enumerate(img_group) if gi == g]
        out.append(sel[imgs].reshape(-1, gate.shape[-1]).max(0)[0])
    return torch.stack(out)
