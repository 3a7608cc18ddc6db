"""RemoveNeuronsNoiseHPO — drop-in for neuron_receivers/remove_skilled_neurons_noise_hpo.py:9-114, the receiver
modularity/remove_experts_noise_hpo.py drives to choose a concept's t-test confidence level: the concept prompt runs
with its skilled neurons removed and the U-Net's output of every step is compared with a BaseUNetReceiver run of the
base prompt.

Same constructor and file layout as RemoveNeuronsHPO. The override applies at EVERY timestep with a non-empty list: the
per-timestep trial switch is commented out in the reference (:51-55), so the trial is stored and never asked.
`observe_activation` returns (image(s), unet_output), unet_output[t] a CPU fp16 [nimg, 4, H, W] tensor (:79-82, :114);
`reset_time_layer` clears them (:31-39).
MI355X path (UNetOutputStore): the outputs are captured on the device through the pipeline's U-Net output seam, indexed
by the seam's step index (the reference indexes by its own counter, which the last GEGLU of the step has already
advanced: its `timestep - 1`, :80-81), and copied to the host once per call (store_outputs=False: never).
`noise_distance_to(base_receiver)` runs sdmoe_noise_distance on the two device stores and returns the driver's two
distances per step and prompt as host float64 arrays -- 4 T B doubles leave the device instead of 2 T blocking copies
of the outputs, and the L1-normalised distance is taken in float64 (the reference takes it on fp16 CPU tensors, where
the normalised elements are below fp16's smallest normal number).
Out of scope: the GELU (PixArt) branch (:64-73).
"""
from __future__ import annotations

from neuron_receivers.base_receiver import GEGLU
from neuron_receivers.remove_skilled_neurons_hpo import RemoveNeuronsHPO
from neuron_receivers.unet_output import UNetOutputStore


class RemoveNeuronsNoiseHPO(UNetOutputStore, RemoveNeuronsHPO):
    def __init__(self, seed, path_expert_indx, T, n_layers, dof_val, conf_val, trials_per_layer=None, replace_fn=GEGLU,
                 keep_nsfw=False, masks=None, store_outputs=True, **kw):
        super().__init__(seed, path_expert_indx, T, n_layers, dof_val, conf_val, trials_per_layer=trials_per_layer,
                         replace_fn=replace_fn, keep_nsfw=keep_nsfw, masks=masks, **kw)
        self.store_outputs = store_outputs
        self.clear_outputs()

    def reset_time_layer(self):
        super().reset_time_layer()
        self.clear_outputs()

    def decide(self, t, l):
        return self.expert_indices[t][l].size > 0

    def unet_hook_fn(self, step_index, eps, nimg, HW):
        self.capture(step_index, eps, nimg, HW)

    def observe_activation(self, model, ann, bboxes=None):
        self._captured = 0
        hook = model.register_unet_output_hook(self.unet_hook_fn)
        try:
            out, _ = super().observe_activation(model, ann, bboxes)
        finally:
            hook.remove()
        self.materialise_outputs()
        return out, self.unet_output
