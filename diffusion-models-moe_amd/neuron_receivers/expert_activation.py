"""ExpertPredictivity — drop-in for neuron_receivers/expert_activation.py:9-66: the expert-level twin of
NeuronPredictivity, the first stage of the paired t-test route to the skilled-expert lists RemoveExperts reads
(modularity_analysis.py with `predictvity_for: expert` -> predictivity_{base,adj}_expert.json and diff_std_expert.json
-> paired_t_test_experts.py -> timestep_{t}_layer_{l}.json; sdmoe.discovery.expert_lists_from_statistics).

Per hooked GEGLU call with MoE-fied `patterns` (:51-59): the per-token expert scores of the activated gate, their
maximum over every token of the prompt's images (`torch.max(score, dim=0)`) kept as `max_gate[t][l]` (an fp16 numpy
array [E]) and fed to `self.predictivity` (sdmoe.discovery.StatMeter); the module output is the dense, unmasked
value * act(gate). With `patterns is None` the output is dense, no statistic is taken and the counter still advances.
MI355X path: `GEGLU.scored` (the projection GEMM whose epilogue produces the scores when FeedForward allows the fused
path, else the routing kernel) plus one small streaming pass over the scores (sdmoe_expert_stats); the maxima of a
whole pipeline call stay on the device and are copied to the host once, when observe_activation returns (the reference
syncs twice per hooked call). The counter, the lazy statistics, the pending list with flush() and the prompt lists are
NeuronPredictivity's: B prompts give B groups, image i belongs to prompt i % B, max_gate[t][l] is [B, E] and the
statistics take one row per prompt, in prompt order.
Fixed defects: the reference's constructor takes no `replace_fn` although modularity_analysis.py
:21-25 passes one, and forwards `keep_nsfw` into the `replace_fn` slot of its base class; both are accepted and land
where they belong. The counter wraps at n_layers - 1 instead of the hard-coded 15.
reset() empties max_gate; reset_time_layer() only resets the counter (:34-36) -- modularity_analysis.py calls it per
prompt and relies on max_gate being overwritten call by call.
"""
from __future__ import annotations

import torch

from sdmoe import ops

from neuron_receivers.base_receiver import GEGLU
from neuron_receivers.predictivity import NeuronPredictivity


class ExpertPredictivity(NeuronPredictivity):
    def __init__(self, seed, T, n_layers, replace_fn=GEGLU, keep_nsfw=False, **kw):
        super().__init__(seed, T, n_layers, replace_fn=replace_fn, keep_nsfw=keep_nsfw, **kw)
        self.sample_id = 0

    def reset_time_layer(self):
        self.timestep = 0
        self.layer = 0

    def reset(self):
        self._max_gate = None
        self._pending = []
        self.reset_time_layer()

    def hook_fn(self, module, input, output):
        if self.replace_fn is not GEGLU:
            raise NotImplementedError("ExpertPredictivity covers GEGLU projections; the GELU (PixArt) branch is out of "
                                      "scope")
        x = input[0]
        if module.patterns is None:
            out = module.dense(x)
            self.update_time_layer()
            return out
        nimg = x.shape[0] if x.dim() >= 3 else 1
        ngroups = 1 if self._nprompts is None else self._nprompts
        table = None if self._nprompts is None else self._image_table_dev(nimg, x.device)
        out, score = module.scored(x)
        colmax = torch.empty((ngroups, score.shape[1]), dtype=torch.float16, device=x.device)
        ops.expert_stats(score, rows_per_img=x.shape[-2] if x.dim() >= 3 else 0, img_group=table, ngroups=ngroups,
                         colmax=colmax)
        self._pending.append((self.timestep, self.layer, colmax))
        self.update_time_layer()
        return out

    def test(self, model):
        return True
