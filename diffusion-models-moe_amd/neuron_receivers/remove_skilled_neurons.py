"""RemoveNeurons — drop-in for neuron_receivers/remove_skilled_neurons.py:9-57 (`condition: t_test | AP` with
`remove_neurons: true`, modularity/remove_experts.py:130-135).

Reads `predictivity_{t}_{l}.json` (a 0/1 list per neuron; an empty list = nothing to remove in that call) for every
(t, l) and, on every hooked GEGLU call, overwrites the activated gate of the masked neurons with -0.17 before the
product: gate[:, :, mask == 1] = -0.17; hidden_states * gate (:35-41). On an fp16 tensor that constant is
-0.1700439453125. `self.gates` collects the gate AFTER the override, as the reference's does (store_gates=False
skips the copy).
As in the reference, the override applies at EVERY timestep: `remove_timesteps` (and `weights_shape`) are accepted,
stored and ignored.
MI355X path: each (t, l) mask is packed to one bit per neuron and uploaded once, at its first use; `GEGLU.neurons`
(projection GEMM + the sdmoe_geglu_neurons streaming pass) applies it. The constructor needs no device.
Out of scope: the GELU (PixArt) branch (:44-53).
"""
from __future__ import annotations

import json
import os

import numpy as np

from sdmoe import ops

from neuron_receivers.base_receiver import GEGLU
from neuron_receivers.predictivity import NeuronPredictivity

OVERRIDE_VALUE = -0.17  # remove_skilled_neurons.py:39


class RemoveNeurons(NeuronPredictivity):
    def __init__(self, seed, path_expert_indx, T, n_layers, replace_fn=GEGLU, keep_nsfw=False, remove_timesteps=None,
                 weights_shape=None, masks=None, **kw):
        super().__init__(seed, T, n_layers, replace_fn=replace_fn, keep_nsfw=keep_nsfw, **kw)
        self.expert_indices = {}
        for t in range(T):
            self.expert_indices[t] = {}
            for l in range(n_layers):
                if masks is not None:
                    m = masks[t][l]
                else:
                    with open(os.path.join(path_expert_indx, f'predictivity_{t}_{l}.json')) as f:
                        m = json.load(f)
                self.expert_indices[t][l] = np.asarray(m).reshape(-1) != 0
        self.remove_timesteps = remove_timesteps
        self.weights_shape = weights_shape
        self.gates = []
        self._bits = {}  # (t, l, device) -> int32 [F/32] device words

    @classmethod
    def from_masks(cls, seed, masks, T, n_layers, **kw):
        """masks[t][l]: in-memory 0/1 arrays [F] (empty = no override), in place of the JSON files."""
        return cls(seed, None, T, n_layers, masks=masks, **kw)

    def override_bits(self, module, t, l):
        """The packed (t, l) mask on module's device (uploaded at first use), or None for an empty list."""
        mask = self.expert_indices[t][l]
        if mask.size == 0:
            return None
        dev = module.proj.weight.device
        bits = self._bits.get((t, l, dev))
        if bits is None:
            if mask.size != module.inner_dim:
                raise ValueError(f"predictivity_{t}_{l}: {mask.size} neurons, the GEGLU has {module.inner_dim}")
            bits = self._bits[(t, l, dev)] = ops.neuron_bits(mask, dev)
        return bits

    def hook_fn(self, module, input, output):
        if self.replace_fn is not GEGLU:
            raise NotImplementedError("RemoveNeurons covers GEGLU projections; the reference's GELU (PixArt) branch is "
                                      "out of scope")
        bits = self.override_bits(module, self.timestep, self.layer)
        out, gate = module.neurons(input[0], override_bits=bits, override_value=OVERRIDE_VALUE,
                                   want_gate=self.store_gates)
        if self.store_gates:
            self.gates.append(gate.detach().cpu())
        self.update_time_layer()
        return out
