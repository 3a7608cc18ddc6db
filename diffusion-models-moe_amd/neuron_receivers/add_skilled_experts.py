"""AddExperts — drop-in for neuron_receivers/add_skilled_experts.py:9-71: the counterpart of RemoveExperts. Removal
zeroes a concept's experts; addition pushes them INTO every token's top-k by biasing their routing scores.

Semantics kept exactly, per hooked GEGLU call at counter (t, l) with MoE-fied `patterns` [E, F] and `k` (:35-71):
  * scores as MOEFy's (fp16 gate sums); then for every expert e of the SET expert_indices[t][l] (a duplicate id is
    applied once: indexed assignment, :55) score[:, e] = fp16(score[:, e] + b_e), b_e = fp16(5.0 * fp16(std[t][l][e])),
    std = predictivity_base_expert.json["time_steps"][str(t)][str(l)]["std"] (:13-15, :29) -- the file
    ExpertPredictivity's statistics write (sdmoe.discovery.StatMeter.save). Two rounding points: the scalar product on
    the fp16 tensor (made on the host by ops.expert_bias with the reference's own torch operations), then the fp16
    add (on the device). No `t < 20` cut-off; an empty list changes no score;
  * k' = int(0.8 * k) experts are selected (:57, Python float arithmetic: k = 12 -> 9), their neurons kept, the rest
    of the gate zeroed; out = value * gate; the masked gate is appended to self.gates; the counter advances once.
Nothing is removed (no removed-expert bitmask on this path). With `patterns is None` the output is dense.
Constructor defect of the snapshot fixed, not replicated, as in the other receivers: `replace_fn` is accepted as a
keyword and `keep_nsfw` no longer lands in the `replace_fn` slot (:10-11).
Stated differences from the reference:
  * a LISTED expert whose std (or 5 * std in fp16) is NaN or infinite raises ValueError (StatMeter writes NaN for a
    cell it never updated; the reference would add NaN to every token's score);
  * k' < 1 raises ValueError (the reference's topk(k=0) would zero every neuron);
  * activation_stats= / expert_indices= give the statistics (a dict of the JSON's shape, or a path) and the lists
    directly; bias_scale / k_fraction default to the reference's literals 5.0 and 0.8.
MI355X layout: each non-empty (t, l) list becomes ONE fp16 bias vector [E] on the device, uploaded once (prepare);
GEGLU.routed(bias=, k=) adds it to the score buffer with one small streaming kernel (sdmoe_score_bias) between the
fused projection's scores and the unchanged top-k kernels run at k' (fused path), or inside the routing kernel
(sdmoe_geglu_route_bias; store_gates=True, or a FeedForward that does not allow the fused path).
count_selected (this port's addition): each call also takes the top-k bitmask and reduces it on the device
(sdmoe_expert_stats); selection_count[t][l] is then the int64 [E] number of tokens that selected each expert in that
call (copied to the host once per pipeline call, by flush()), selection_rate(t, l) the fraction of tokens that selected
each LISTED expert -- the first number a user of AddExperts wants.
test() (:74-103) is the one every receiver of this port inherits (BaseNeuronReceiver.test: a run without and a run with
the hooks, every stored gate >= 0 exactly when the U-Net is relufied, checked from device results; no image is saved).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from sdmoe import mask_io, ops

from neuron_receivers.base_receiver import GEGLU
from neuron_receivers.predictivity import NeuronPredictivity

STATS_FILE = 'predictivity_base_expert.json'  # add_skilled_experts.py:15


def stats_path(path_expert_indx: str) -> str:
    """add_skilled_experts.py:13-15: the statistics file next to the adjective's results, three levels above the lists."""
    adj = path_expert_indx.split('/')[-3]
    base_path = path_expert_indx.split(adj)[0]
    return os.path.join(base_path, adj, STATS_FILE)


def k_selected(k: int, k_fraction: float = 0.8) -> int:
    """add_skilled_experts.py:57: int(0.8 * k) in Python float arithmetic."""
    return int(k_fraction * k)


class AddExperts(NeuronPredictivity):
    def __init__(self, seed, path_expert_indx, T, n_layers, keep_nsfw=False, replace_fn=GEGLU, expert_indices=None,
                 activation_stats=None, bias_scale=5.0, k_fraction=0.8, count_selected=False, **kw):
        super().__init__(seed, T, n_layers, replace_fn=replace_fn, keep_nsfw=keep_nsfw, **kw)
        if activation_stats is None:
            activation_stats = stats_path(path_expert_indx)
        if not isinstance(activation_stats, dict):
            with open(activation_stats) as f:
                activation_stats = json.load(f)
        cells = activation_stats.get('time_steps', activation_stats)
        self.bias_scale = bias_scale
        self.k_fraction = k_fraction
        self.count_selected = count_selected
        self.expert_indices = {}
        self.avg_activation = {}  # (the reference's name for the std lists, :29)
        for i in range(T):
            self.expert_indices[i] = {}
            self.avg_activation[i] = {}
            ci = cells[str(i)] if str(i) in cells else cells[i]
            for j in range(n_layers):
                if expert_indices is not None:
                    self.expert_indices[i][j] = [int(e) for e in expert_indices[i][j]]
                else:
                    self.expert_indices[i][j] = mask_io.load_expert_list(
                        os.path.join(path_expert_indx, f'timestep_{i}_layer_{j}.json'))
                cij = ci[str(j)] if str(j) in ci else ci[j]
                self.avg_activation[i][j] = list(cij['std'])
        self.timestep = 0
        self.layer = 0
        self.gates = []
        self._bias = {}
        self.selection_count = {t: {} for t in range(T)}
        self.selection_tokens = {t: {} for t in range(T)}
        self._sel_pending = []  # (t, l, tokens, device int32 [1, E] counts) of the running pipeline call

    def prepare(self, model):
        """Upload the fp16 bias vector of every (t, l) with a non-empty list, once (layer l = l-th hooked GEGLU)."""
        mods = [m for _, m in self.hook_modules(model)]
        for t in range(self.T):
            for l in range(self.n_layers):
                m = mods[l % len(mods)]
                if m.patterns is not None:
                    self.bias_for(m, t, l)

    def observe_activation(self, model, ann, bboxes=None):
        self.prepare(model)
        try:
            return super().observe_activation(model, ann, bboxes)
        finally:
            self.flush_selection()

    def bias_for(self, module, t, l):
        ids = self.expert_indices[t][l]
        if len(ids) == 0:
            return None
        bias = self._bias.get((t, l))
        if bias is None:
            bias = self._bias[(t, l)] = ops.expert_bias(ids, self.avg_activation[t][l], module.patterns.shape[0],
                                                        module.proj.weight.device, scale=self.bias_scale)
        return bias

    def hook_fn(self, module, input, output):
        x = input[0]
        if module.patterns is None:
            out, gate = module.routed(x, want_gate=self.store_gates)
        else:
            k = k_selected(module.k, self.k_fraction)
            if k < 1:
                raise ValueError(f"AddExperts: int({self.k_fraction} * {module.k}) = {k} experts would be selected")
            E = module.patterns.shape[0]
            tokens = x.numel() // x.shape[-1]
            sel = score = None
            if self.count_selected:
                # ops.expert_stats takes the [tokens, E] score view for its shape; only the selection bits are reduced.
                # On the fused path this buffer is the one routed() would allocate anyway; on the unfused path it is
                # an extra [tokens, E] fp16 write per call (score_out of the routing kernel), 1 / 40 of its gate_out.
                sel = torch.empty((tokens, (E + 31) // 32), dtype=torch.int32, device=x.device)
                score = torch.empty((tokens, E), dtype=torch.float16, device=x.device)
            out, gate = module.routed(x, want_gate=self.store_gates, sel_out=sel, score_out=score,
                                      bias=self.bias_for(module, self.timestep, self.layer), k=k)
            if self.count_selected:
                count = torch.empty((1, E), dtype=torch.int32, device=x.device)
                ops.expert_stats(score, sel=sel, count=count)
                self._sel_pending.append((self.timestep, self.layer, tokens, count))
        self.update_time_layer()
        if self.store_gates:
            self.gates.append(gate.detach().cpu())
        return out

    # this hook_fn only hands input[0] to module.routed(), which resolves a LayerNorm deferred into the GEGLU call:
    # the block's norm3 may then stay folded into the projection GEMM (sdmoe.unet.FeedForward.run). A subclass that
    # overrides hook_fn does not inherit this (the marker names this exact function).
    _sdmoe_ln_safe_hook = hook_fn

    def flush_selection(self):
        """Materialise the pending device counts (one device->host copy) into selection_count[t][l] (int64 [E])."""
        if not self._sel_pending:
            return
        pending, self._sel_pending = self._sel_pending, []
        flat = torch.cat([p[3].reshape(-1) for p in pending]).cpu().numpy()
        o = 0
        for t, l, tokens, dev in pending:
            self.selection_count[t][l] = flat[o:o + dev.numel()].astype(np.int64)
            self.selection_tokens[t][l] = tokens
            o += dev.numel()

    def selection_rate(self, t, l):
        """{expert id: fraction of the tokens of call (t, l) that selected it} for the experts listed at (t, l)."""
        self.flush_selection()
        cnt, tokens = self.selection_count[t][l], self.selection_tokens[t][l]
        return {e: float(cnt[e]) / tokens for e in sorted(set(self.expert_indices[t][l]))}
