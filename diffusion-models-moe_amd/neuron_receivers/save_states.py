"""SaveStates — drop-in for neuron_receivers/save_states.py:8-33: keeps the activated gate of every hooked GEGLU call.

`hidden_states[t][l]` is the CPU copy of act(gate) of call (t, l) (:20-25; an empty tensor until that call ran), the
module output is the dense value * act(gate); `save(path)` writes the nested dict with torch.save (:32-33).
MI355X path: `GEGLU.neurons(..., want_gate=True)` -- the projection GEMM plus the sdmoe_geglu_neurons streaming pass,
which writes the product and the activated gate. The constructor needs no device.
"""
from __future__ import annotations

import torch

from neuron_receivers.base_receiver import GEGLU
from neuron_receivers.predictivity import NeuronPredictivity


class SaveStates(NeuronPredictivity):
    def __init__(self, seed, T, n_layers):
        super().__init__(seed, T, n_layers)
        self.hidden_states = {t: {l: torch.empty(0) for l in range(n_layers)} for t in range(T)}

    def hook_fn(self, module, input, output):
        if self.replace_fn is not GEGLU:
            raise NotImplementedError("SaveStates covers GEGLU projections")
        out, gate = module.neurons(input[0], want_gate=True)
        self.hidden_states[self.timestep][self.layer] = gate.detach().cpu()
        self.update_time_layer()
        return out

    def save(self, path):
        torch.save(self.hidden_states, path)
