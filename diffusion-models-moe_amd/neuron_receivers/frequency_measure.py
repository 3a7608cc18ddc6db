"""FrequencyMeasure — drop-in for neuron_receivers/frequency_measure.py:6-64: the per-expert selection histogram
behind moefication/freq_expert_select.py's expert_counter_{topk}.json (sdmoe.discovery.accumulate_expert_counter /
save_expert_counter), the tool for choosing `topk_experts`.

Per hooked GEGLU call with MoE-fied `patterns` (:47-60): the module output is exactly MOEFy's (the per-token top-k
expert mask applied), and `label_counter[t][l]` (float64 numpy [E]) grows by the fraction of tokens that selected each
expert: count * (1.0 / seq_len), which equals the reference's repeated `+= 1.0 / seq_len` exactly for a power-of-two
seq_len (every U-Net level). With `patterns is None` the output is dense and nothing is counted; the counter advances.
Which images are counted: the reference counts only `labels[0]`, the first image of the call -- under classifier-free
guidance that is the UNCONDITIONAL image, not the prompt's. That is kept as the default, images="first";
images="all" (this port's addition) sums over every image of the prompt and divides by n_images * seq_len.
Prompt lists (this port's addition): for a list of B prompts the U-Net runs [uncond x B ; cond x B], image i belongs to
prompt i % B, and label_counter[t][l] is [B, E]: row p from image p ("first") or from images p and p + B ("all").
MI355X path: `GEGLU.routed(sel_out=, score_out=)` -- the same kernels as MOEFy, fused when FeedForward allows it --
plus one small streaming pass over the top-k bitmask (sdmoe_expert_stats); the int32 counts of a whole pipeline call
stay on the device and are copied to the host once, by flush(), when observe_activation returns (the reference copies
the labels on every hooked call and loops over up to 4096 tokens in Python).
The counter wraps at n_layers - 1 instead of the hard-coded 15. reset() zeroes the counters.
"""
from __future__ import annotations

import numpy as np
import torch

from sdmoe import ops
from sdmoe._lib import SdmoeError

from neuron_receivers.base_receiver import BaseNeuronReceiver


class FrequencyMeasure(BaseNeuronReceiver):
    def __init__(self, seed, T, n_layers, experts_per_layer, layer_names, images="first", **kw):
        kw.setdefault("store_gates", False)  # the reference's FrequencyMeasure keeps no gates
        super().__init__(seed, **kw)
        if images not in ("first", "all"):
            raise ValueError(f"images must be 'first' or 'all', got {images!r}")
        self.images = images
        self.T = T
        self.n_layers = n_layers
        self.experts_per_layer = experts_per_layer
        self.layer_names = layer_names
        self.label_counter = {}
        self.sample_id = 0
        self.flush_count = 0    # device->host copies done by flush() (one per pipeline call)
        self._pending = []      # (t, l, seq_len, device int32 [images, E] counts) of the running pipeline call
        self._nprompts = None   # None: a single prompt; B: a list of B prompts
        self.reset()

    def update_time_layer(self):
        if self.layer == self.n_layers - 1:
            self.layer = 0
            self.timestep += 1
        else:
            self.layer += 1

    def reset_time_layer(self):
        self.timestep = 0
        self.layer = 0

    def reset(self):
        for t in range(self.T):
            self.label_counter[t] = {}
            for i in range(self.n_layers):
                self.label_counter[t][i] = np.zeros(self.experts_per_layer[self.layer_names[i]])
        self._pending = []
        self.reset_time_layer()

    def set_prompts(self, ann):
        """Fix the grouping of the next calls: a prompt string (or None) is one prompt, a list of B prompts gives B
        rows."""
        self._nprompts = None if ann is None or isinstance(ann, str) else len(ann)

    def hook_fn(self, module, input, output):
        x = input[0]
        if module.patterns is None:
            out, _ = module.routed(x)
            self.update_time_layer()
            return out
        nimg = x.shape[0] if x.dim() >= 3 else 1
        seq_len = x.shape[-2]
        B = self._nprompts
        if B is not None and nimg not in (B, 2 * B):
            raise SdmoeError(f"the call runs {nimg} U-Net images, but {B} prompts were configured (expected {B} or, "
                             f"with guidance, {2 * B} images)")
        E = module.patterns.shape[0]
        sel = torch.empty((nimg * seq_len, (E + 31) // 32), dtype=torch.int32, device=x.device)
        score = torch.empty((nimg * seq_len, E), dtype=torch.float16, device=x.device)
        out, _ = module.routed(x, sel_out=sel, score_out=score)
        count = torch.empty((nimg, E), dtype=torch.int32, device=x.device)
        ops.expert_stats(score, sel=sel, rows_per_img=seq_len if x.dim() >= 3 else 0, count=count)
        self._pending.append((self.timestep, self.layer, seq_len, count))
        self.update_time_layer()
        return out

    # this hook_fn only hands input[0] to module.routed(), which resolves a LayerNorm deferred into the GEGLU call:
    # the block's norm3 may then stay folded into the projection GEMM (sdmoe.unet.FeedForward.run), as under MOEFy.
    _sdmoe_ln_safe_hook = hook_fn

    def flush(self):
        """Materialise the pending device counts (one device->host copy) into label_counter."""
        if not self._pending:
            return
        pending, self._pending = self._pending, []
        flat = torch.cat([p[3].reshape(-1) for p in pending]).cpu().numpy()
        self.flush_count += 1
        o = 0
        for t, l, seq_len, dev in pending:
            cnt = flat[o:o + dev.numel()].reshape(tuple(dev.shape)).astype(np.float64)
            o += dev.numel()
            nimg = cnt.shape[0]
            B = 1 if self._nprompts is None else self._nprompts
            if self.images == "first":
                rows = cnt[:B] * (1.0 / seq_len)
            else:
                rows = cnt.reshape(nimg // B, B, -1).sum(0) / float((nimg // B) * seq_len)
            rows = rows[0] if self._nprompts is None else rows
            cur = self.label_counter[t][l]
            self.label_counter[t][l] = cur + rows if np.shape(cur) == rows.shape else rows

    def observe_activation(self, model, ann, bboxes=None):
        self.set_prompts(ann)
        try:
            return super().observe_activation(model, ann, bboxes)
        finally:
            self.flush()
