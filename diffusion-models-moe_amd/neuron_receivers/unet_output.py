"""UNetOutputStore — the part BaseUNetReceiver and RemoveNeuronsNoiseHPO share: every step's U-Net output kept on the
device during a pipeline call (this port's addition; the reference's unet_hook_fn copies each step to the host,
base_unet_receiver.py:25-29, remove_skilled_neurons_noise_hpo.py:79-82).

The pipeline's seam (StableDiffusionPipeline.register_unet_output_hook) hands over the live padded eps buffer after
every U-Net evaluation; `ops.noise_capture` copies its four valid channels into step `step_index` of a compact fp16
[T, nimg * HW, 4] device store on the same stream. When the call returns, `unet_output[t]` is materialised as the
reference's CPU fp16 [nimg, 4, H, W] tensors with ONE device->host copy (store_outputs=False skips it: the objective,
`ops.noise_distance`, reads the device stores). Steps are indexed by the seam's step index, not by the receiver's
(timestep, layer) counter (the reference's RemoveNeuronsNoiseHPO needs a `timestep - 1` workaround for that).
"""
from __future__ import annotations

import torch

from sdmoe import ops


class UNetOutputStore:
    store_outputs = True
    _store = None       # fp16 device [T, nimg * HW, 4]
    _captured = 0       # steps of the store written by the last call
    _nimg = 0
    output_copies = 0   # device->host copies done by materialise_outputs (one per pipeline call)

    def clear_outputs(self):
        self.unet_output = {t: [] for t in range(self.T)}
        self._captured = 0

    def capture(self, step_index, eps, nimg, HW):
        """The pipeline hook: eps's channels 0..3 -> step `step_index` of the device store."""
        if not 0 <= step_index < self.T:
            raise IndexError(f"the pipeline ran U-Net call {step_index}, but {type(self).__name__} was built for T = "
                             f"{self.T} calls")
        rows = nimg * HW
        if self._store is None or tuple(self._store.shape) != (self.T, rows, 4) or self._store.device != eps.device:
            self._store = torch.empty((self.T, rows, 4), dtype=torch.float16, device=eps.device)
            self._captured = 0
        ops.noise_capture(eps, self._store[step_index])
        self._nimg = nimg
        self._captured = max(self._captured, step_index + 1)

    def device_outputs(self):
        """(fp16 device [steps, nimg * HW, 4] view of the captured steps, nimg) of the last call."""
        if self._store is None or self._captured == 0:
            raise RuntimeError(f"{type(self).__name__} has captured no U-Net output yet: run observe_activation first")
        return self._store[:self._captured], self._nimg

    def materialise_outputs(self):
        """unet_output[t] = CPU fp16 [nimg, 4, H, W] for every captured step: one device->host copy."""
        if self._store is None or self._captured == 0 or not self.store_outputs:
            return
        dev, nimg = self.device_outputs()
        host = dev.cpu()
        self.output_copies += 1
        HW = host.shape[1] // nimg
        H = int(round(HW ** 0.5))
        shape = (nimg, H, HW // H, 4) if H * (HW // H) == HW else (nimg, 1, HW, 4)
        for t in range(host.shape[0]):
            self.unet_output[t] = host[t].view(*shape).permute(0, 3, 1, 2).contiguous()

    def noise_distance_to(self, base_receiver):
        """(l2 [steps, G], l1n [steps, G]) host float64 arrays (sdmoe.discovery.noise_distances): per step and prompt,
        torch.norm(base - own) and the distance of the L1-normalised outputs -- the two quantities of
        modularity/remove_experts_noise_hpo.py:74-84 -- from ops.noise_distance on base_receiver's device store (a) and
        this one's (b). G = the prompts of this receiver's last call (image i belongs to prompt i % B), 1 for a single
        prompt string."""
        from sdmoe.discovery import noise_distances
        a, nimg_a = base_receiver.device_outputs()
        b, nimg_b = self.device_outputs()
        if a.shape != b.shape or nimg_a != nimg_b:
            raise ValueError(f"the two receivers captured different runs: {tuple(a.shape)} ({nimg_a} images) and "
                             f"{tuple(b.shape)} ({nimg_b} images)")
        if self._nprompts is None:
            return noise_distances(ops.noise_distance(a, b, nimg_b))
        return noise_distances(ops.noise_distance(a, b, nimg_b, img_group=self._image_table_dev(nimg_b, b.device),
                                                  ngroups=self._nprompts))
