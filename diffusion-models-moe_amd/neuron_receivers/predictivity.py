"""NeuronPredictivity — drop-in for neuron_receivers/predictivity.py:9-62: the (timestep, layer) counter every masking
receiver inherits, and the max-activation statistics of the paired t-test path.

Counter: one `update_time_layer()` per hooked call, wrapping `layer` at n_layers-1 and advancing `timestep` (hook
call order == U-Net execution order, one U-Net call per step).
Statistics (:42-53): per hooked GEGLU call, the per-neuron maximum of the activated gate over every token of the
prompt's images, kept as `max_gate[t][l]` (an fp16 numpy array, as the reference's `max_act.cpu().numpy()`) and fed
to `self.predictivity` (sdmoe.discovery.StatMeter); the module output is the dense value * act(gate).
MI355X path: `GEGLU.neurons` — the projection GEMM plus one streaming pass (sdmoe_geglu_neurons) that writes the
product and the column maximum; the maxima of a whole pipeline call stay on the device and are copied to the host
once, when observe_activation returns (the reference syncs on every hooked call).
Prompt batches (this port's addition): for a list of B prompts the U-Net runs [uncond x B ; cond x B], image i belongs
to prompt i % B; max_gate[t][l] is then [B, F] and the statistics are updated once per prompt, in prompt order. A single
prompt string is one group over all of its images: exactly the reference's `view(-1, F)` maximum.
The statistics objects are built on first use: subclasses that override hook_fn (RemoveExperts, the Wanda removers)
never touch them, and the constructor allocates nothing on a device.
Out of scope: the reference's GELU (PixArt) branch (:54-62, a column MEAN of a plain GELU projection) — hook_fn raises
NotImplementedError for any replace_fn but GEGLU.
"""
from __future__ import annotations

import torch

from neuron_receivers.base_receiver import GEGLU, BaseNeuronReceiver
from neuron_receivers.prompt_groups import PromptGroups


class NeuronPredictivity(PromptGroups, BaseNeuronReceiver):
    def __init__(self, seed, T, n_layers, replace_fn=GEGLU, keep_nsfw=False, hook_module='unet', **kw):
        super().__init__(seed, replace_fn, keep_nsfw, hook_module, **kw)
        self.T = T
        self.n_layers = n_layers
        self.timestep = 0
        self.layer = 0
        self._predictivity = None
        self._max_gate = None
        self._pending = []      # (t, l, device [ngroups, F] maxima) of the running pipeline call
        self._nprompts = None   # None: a single prompt (one group); B: a list of B prompts
        self._img_tables = {}       # (image count, device) -> int32 device image -> prompt table
        self.flush_count = 0        # device->host copies done by flush() (one per pipeline call)

    # ---- statistics, built on first use ----------------------------------------------------------------------------
    @property
    def predictivity(self):
        if self._predictivity is None:
            from sdmoe.discovery import StatMeter
            self._predictivity = StatMeter(self.T, self.n_layers)
        return self._predictivity

    @predictivity.setter
    def predictivity(self, meter):
        self._predictivity = meter

    @property
    def max_gate(self):
        if self._max_gate is None:
            self._max_gate = {t: {l: [] for l in range(self.n_layers)} for t in range(self.T)}
        return self._max_gate

    # ---- counter -----------------------------------------------------------------------------------------------------
    def update_time_layer(self):
        if self.layer == self.n_layers - 1:
            self.layer = 0
            self.timestep += 1
        else:
            self.layer += 1

    def reset_time_layer(self):
        self.timestep = 0
        self.layer = 0
        self._max_gate = None  # predictivity.py:35-39: the per-prompt maxima start over
        self._pending = []

    # ---- prompt groups: set_prompts / image_table / _image_table_dev come from PromptGroups (prompt_groups.py) ------
    def position_bits(self, module, seq_len, device):
        """Token positions that enter the maximum (None: all of them). NeuronPredictivityBB narrows them."""
        return None

    # ---- the hook --------------------------------------------------------------------------------------------------
    def hook_fn(self, module, input, output):
        if self.replace_fn is not GEGLU:
            raise NotImplementedError("NeuronPredictivity covers GEGLU projections; the reference's GELU (PixArt) branch "
                                      "takes a column mean of a plain GELU projection and is out of scope")
        x = input[0]
        nimg = x.shape[0] if x.dim() >= 3 else 1
        seq_len = x.shape[-2]
        ngroups = 1 if self._nprompts is None else self._nprompts
        table = None if self._nprompts is None else self._image_table_dev(nimg, x.device)
        colmax = torch.empty((ngroups, module.inner_dim), dtype=torch.float16, device=x.device)
        out, _ = module.neurons(x, colmax=colmax, img_group=table, ngroups=ngroups,
                                pos_bits=self.position_bits(module, seq_len, x.device))
        self._pending.append((self.timestep, self.layer, colmax))
        self.update_time_layer()
        return out

    def flush(self):
        """Materialise the pending device maxima (one device->host copy): max_gate[t][l] becomes an fp16 numpy array,
        [F] for a single prompt and [B, F] for a prompt list, and the statistics take one row per prompt, in order."""
        if not self._pending:
            return
        pending, self._pending = self._pending, []
        flat = torch.cat([p[2].reshape(-1) for p in pending]).cpu().numpy()
        self.flush_count += 1
        o = 0
        for t, l, dev in pending:
            rows = flat[o:o + dev.numel()].reshape(tuple(dev.shape))
            o += dev.numel()
            self.max_gate[t][l] = rows[0] if self._nprompts is None else rows
            for row in rows:
                self.predictivity.update(row, t, l)

    def observe_activation(self, model, ann, bboxes=None):
        self.set_prompts(ann)
        try:
            return super().observe_activation(model, ann, bboxes)
        finally:
            self.flush()
