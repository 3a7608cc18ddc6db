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

from sdmoe._lib import SdmoeError

from neuron_receivers.base_receiver import GEGLU, BaseNeuronReceiver


class NeuronPredictivity(BaseNeuronReceiver):
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

    # ---- prompt groups ---------------------------------------------------------------------------------------------
    def set_prompts(self, ann):
        """Fix the grouping of the next calls: a prompt string (or None) is one group over every image, a list of B
        prompts gives B groups."""
        self._nprompts = None if ann is None or isinstance(ann, str) else len(ann)
        self._img_tables = {}

    def image_table(self, nimg):
        """Prompt of each of the call's nimg U-Net images: i % B for B or, under guidance, 2 B images."""
        B = self._nprompts
        if B and nimg in (B, 2 * B):
            return [i % B for i in range(nimg)]
        raise SdmoeError(f"the call runs {nimg} U-Net images, but {B} prompts were configured (expected {B} or, with "
                         f"guidance, {2 * B if B else 0} images)")

    def _image_table_dev(self, nimg, device):
        key = (nimg, device)
        tab = self._img_tables.get(key)
        if tab is None:
            tab = self._img_tables[key] = torch.tensor(self.image_table(nimg), dtype=torch.int32, device=device)
        return tab

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
