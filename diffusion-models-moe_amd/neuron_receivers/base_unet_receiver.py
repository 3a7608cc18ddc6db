"""BaseUNetReceiver — drop-in for neuron_receivers/base_unet_receiver.py:7-45: the receiver that only records the
U-Net's output at every step (the base-prompt run of modularity/remove_experts_noise_hpo.py:60-63).

No GEGLU module is hooked, so the image is bit-identical to a bare pipeline call. `observe_activation` returns
(image(s), unet_output) with unet_output[t] a CPU fp16 [nimg, 4, H, W] tensor as in the reference (`output[0]` of the
U-Net's forward hook: the whole [uncond ; cond] batch).
MI355X path (UNetOutputStore): the steps are captured into a device store through the pipeline's U-Net output seam --
the loop calls unet.forward_nhwc, a module forward hook would never fire -- and copied to the host once, when the call
returns; `store_outputs=False` skips that copy for runs that only feed RemoveNeuronsNoiseHPO.noise_distance_to.
The seam's hook is removed in a `finally`. The constructor needs no device.
"""
from __future__ import annotations

from neuron_receivers.base_receiver import GEGLU
from neuron_receivers.predictivity import NeuronPredictivity
from neuron_receivers.unet_output import UNetOutputStore


class BaseUNetReceiver(UNetOutputStore, NeuronPredictivity):
    '''class to only store the output of the unet'''

    def __init__(self, seed, T, n_layers, store_outputs=True):
        super().__init__(seed, T, n_layers, GEGLU, keep_nsfw=False)
        self.store_outputs = store_outputs
        self.clear_outputs()

    def update_timestep(self):
        self.timestep += 1

    def reset_time(self):
        self.timestep = 0
        self.clear_outputs()

    def unet_hook_fn(self, step_index, eps, nimg, HW):
        self.capture(step_index, eps, nimg, HW)
        self.update_timestep()

    def observe_activation(self, model, ann, bboxes=None):
        self.set_prompts(ann)
        self._captured = 0
        hook = model.register_unet_output_hook(self.unet_hook_fn)
        try:
            out = self.run_model(model, ann)
        finally:
            hook.remove()
        self.materialise_outputs()
        return out, self.unet_output
