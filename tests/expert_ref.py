"""CPU restatement (torch, fp16) of the expert-level discovery hooks, the checker of tests/test_expert_host.py (pinned
there to the reference's own hooks through the tests/golden/expert_* fixtures) and of tests/test_gpu_expert_stats.py.

  scores         proj -> chunk -> act(gate) -> gate @ patterns.T: (value, activated gate, per-token expert scores)
  pred_hook      ExpertPredictivity.hook_fn: the dense value * gate and torch.max(score, dim=0)
  freq_hook      FrequencyMeasure.hook_fn: the top-k masked value * gate and how often image 0 selected each expert,
                 accumulated as the reference does (one += 1 / seq_len per token)
  unpack_sel     the routing kernels' sel words -> a bool [rows, E] matrix
Shared helpers regenerate the fixtures' modules and tokens from their seeds (tests/golden/synth.py, neuron_ref.py).
"""
import numpy as np
import torch

from neuron_ref import act_fn, golden, group_max, synth, weights, x_seed  # noqa: F401


def patterns(c):
    """The [E, 4C] 0/1 fp16 matrix moefication/helper.py:48-62 builds from the fixture's labels."""
    labels = torch.from_numpy(np.asarray(c["labels"]).astype(np.int64))
    return torch.nn.functional.one_hot(labels, int(c["E"])).t().contiguous().half()


def tokens(c, seed, nimg=2):
    return torch.from_numpy(synth.tokens((nimg, int(c["N"]), int(c["C"])), int(seed))).half()


def pred_tokens(c, prompt, kind, call, nimg=2):
    return tokens(c, x_seed(int(c["seed"]), prompt, kind, call), nimg)


def scores(x, w, b, act, pat):
    value, gate = torch.nn.functional.linear(x, w, b).chunk(2, dim=-1)
    gate = act_fn(act)(gate)
    score = torch.matmul(gate.reshape(-1, gate.shape[-1]), pat.transpose(0, 1))
    return value, gate, score


def pred_hook(x, w, b, act, pat):
    """(value * act(gate), torch.max(score, dim=0) [E])."""
    value, gate, score = scores(x, w, b, act, pat)
    return value * gate, torch.max(score, dim=0)[0]


def freq_hook(x, w, b, act, pat, k, counter):
    """(masked value * gate, score [images, tokens, E]); counter (float64 [E]) += 1 / seq_len per token of image 0 and
    selected expert."""
    value, gate, score = scores(x, w, b, act, pat)
    bsz, seq_len = x.shape[0], x.shape[1]
    labels = torch.topk(score, k=k, dim=-1)[1].view(bsz, seq_len, k)
    first = labels[0].numpy()
    for i in range(first.shape[0]):
        counter[first[i, :]] += (1.0 / seq_len)
    mask = torch.nn.functional.embedding(labels, pat).sum(-2)
    gate = gate.clone()
    gate[mask == 0] = 0
    return value * gate, score.view(bsz, seq_len, -1)


def unpack_sel(sel, E):
    """sel [rows, ceil(E / 32)] int32 / uint32 words (numpy) -> bool [rows, E]; bits at or above E are dropped."""
    words = np.ascontiguousarray(sel).view(np.uint32)
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :E].astype(bool)


def pack_sel(on):
    """bool [rows, E] -> int32 words [rows, ceil(E / 32)] (bits at or above E clear)."""
    rows, E = on.shape
    pad = np.zeros((rows, -(-E // 32) * 32), dtype=bool)
    pad[:, :E] = on
    return np.packbits(pad, axis=1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)
