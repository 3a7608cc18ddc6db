"""CPU restatement (torch, fp16) of AddExperts.hook_fn (neuron_receivers/add_skilled_experts.py:35-71), the checker of
tests/test_add_experts_host.py (pinned there bit for bit to the reference's own hook through the
tests/golden/add_experts_* fixtures) and of tests/test_gpu_add_experts.py.

  bias_vector    the per-expert bias as the hook forms it: scale * tensor(std).to(fp16), at the SET of listed ids
  biased         score + bias on the listed columns only (an indexed assignment: a duplicate id is applied once)
  k_selected     int(0.8 * k), Python float arithmetic
  route          top-k' of a score matrix -> (value * masked gate, masked gate, indices)
  add_hook       the whole hook from x: (out, masked gate, biased score [rows, E], top-k' indices [rows, k'])
  route_from_y   the same from a projection output y = [value | gate] (the GPU tests hand it the device's own y)
  topk_lowest    top-k with ties toward the lowest expert id as a bool [rows, E] matrix (the device's tie rule)
Shared helpers regenerate the fixtures' modules and tokens from their seeds (expert_ref.py, tests/golden/synth.py).
"""
import numpy as np
import torch

from expert_ref import act_fn, golden, patterns, scores, synth, unpack_sel, weights  # noqa: F401


def tokens(c, call, nimg=2):
    """The tokens [nimg, N, C] of hooked call `call` of a fixture: one searched seed per token row."""
    N, C = int(c["N"]), int(c["C"])
    rows = np.stack([synth.tokens((C,), int(s)) for s in c["x_seeds"][call]])
    return torch.from_numpy(rows.reshape(nimg, N, C)).half()


def bias_vector(ids, std, E, scale=5.0):
    full = scale * torch.tensor([float(v) for v in std]).to(torch.float16)
    out = torch.zeros(E, dtype=torch.float16)
    ids = [int(e) for e in ids]
    if ids:
        out[ids] = full[ids]
    return out


def biased(score, ids, std, scale=5.0):
    ids = [int(e) for e in ids]
    score = score.clone()
    if ids:
        add = scale * torch.tensor([float(v) for v in std]).to(score.dtype)
        score[:, ids] = score[:, ids] + add[ids]
    return score


def k_selected(k):
    return int(0.8 * k)


def route(value, gate, score, pat, kk):
    """value, gate [..., F]; score [rows, E]: keep the neurons of each row's top-kk experts."""
    labels = torch.topk(score, k=kk, dim=-1)[1]
    mask = torch.nn.functional.embedding(labels, pat).sum(-2).view(gate.shape)
    gate = gate.clone()
    gate[mask == 0] = 0
    return value * gate, gate, labels


def add_hook(x, w, b, act, pat, k, ids, std):
    value, gate, score = scores(x, w, b, act, pat)
    score = biased(score, ids, std)
    out, gate, labels = route(value, gate, score, pat, k_selected(k))
    return out, gate, score, labels


def route_from_y(y, act, pat, k, ids, std):
    """y [rows, 2F] fp16 -> (out, masked gate, biased score, top-k' indices), the hook's arithmetic after the projection."""
    value, gate = y.chunk(2, dim=-1)
    gate = act_fn(act)(gate)
    score = biased(torch.matmul(gate, pat.transpose(0, 1)), ids, std)
    out, gate, labels = route(value, gate, score, pat, k_selected(k))
    return out, gate, score, labels


def topk_lowest(score, k):
    """bool [rows, E]: the k largest of each row of `score` (numpy, any float dtype; -0 == +0), ties at the k-th value
    toward the lowest column -- a stable descending argsort."""
    s = np.asarray(score).astype(np.float32) + 0.0
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    on = np.zeros(s.shape, dtype=bool)
    np.put_along_axis(on, order, True, axis=1)
    return on


def expand_keep(on, esize):
    """bool [rows, E] selection -> bool [rows, E * esize] over the expert-major neurons."""
    return np.repeat(on, esize, axis=1)


def unpack_keep(keep):
    """keep words int64 [F / 64, M] (numpy) -> bool [M, F]."""
    kb = np.ascontiguousarray(keep).view(np.uint64)
    bits = ((kb[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return np.ascontiguousarray(bits.transpose(1, 0, 2).reshape(kb.shape[1], -1))
