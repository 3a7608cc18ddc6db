"""RemoveNeuronsHPO — drop-in for neuron_receivers/remove_skilled_neurons_hpo.py:9-73, the receiver
modularity/remove_experts_hpo.py drives to choose, per timestep, whether a concept's skilled neurons are removed.

Masks are read from `dof_{dof_val}_conf_{conf_val}/timestep_{t}_layer_{l}.json` under path_expert_indx (:13-19; a 0/1
list per neuron, an empty list = nothing to remove in that call). On a hooked GEGLU call with a non-empty list the
per-timestep decision update_for_t[t] says whether the override of RemoveNeurons applies (gate[:, :, mask == 1] = -0.17,
:49-51): 1 for t < 10, otherwise `trials_per_layer.suggest_categorical(f"timestep_{t}", [0, 1])` -- an optuna trial, or
anything with that method -- asked once per timestep and run (reset_time_layer starts a new run). `trials_per_layer` may
also be a sequence of T 0/1 values (the reference's commented-out `self.trial[self.timestep]`, :41). Decision 0 runs the
dense product; `self.gates` collects the gate after the override (store_gates=False skips the copy).
Fixed defect: the reference asks only at layer 0 and only if layer 0's list is non-empty (:42), so a timestep whose
first non-empty list belongs to a later layer raises KeyError at :49. Here the decision is taken at the timestep's
first call with a non-empty list, whichever layer that is.
MI355X path: RemoveNeurons' -- bit-packed masks uploaded at first use, `GEGLU.neurons`. `decide` and the constructor
need no device.
Out of scope: the GELU (PixArt) branch (:60-69).
"""
from __future__ import annotations

import json
import os

from neuron_receivers.base_receiver import GEGLU
from neuron_receivers.remove_skilled_neurons import OVERRIDE_VALUE, RemoveNeurons

FREE_TIMESTEPS = 10  # remove_skilled_neurons_hpo.py:43: below it the neurons are always removed


def read_hpo_masks(path_expert_indx, dof_val, conf_val, T, n_layers):
    """masks[t][l] from dof_{dof}_conf_{conf}/timestep_{t}_layer_{l}.json (remove_skilled_neurons_hpo.py:13-19)."""
    folder = os.path.join(path_expert_indx, f"dof_{dof_val}_conf_{conf_val}")
    masks = {}
    for t in range(T):
        masks[t] = {}
        for l in range(n_layers):
            with open(os.path.join(folder, f'timestep_{t}_layer_{l}.json')) as f:
                masks[t][l] = json.load(f)
    return masks


class RemoveNeuronsHPO(RemoveNeurons):
    def __init__(self, seed, path_expert_indx, T, n_layers, dof_val, conf_val, trials_per_layer=None, replace_fn=GEGLU,
                 keep_nsfw=False, masks=None, **kw):
        if masks is None:
            masks = read_hpo_masks(path_expert_indx, dof_val, conf_val, T, n_layers)
        super().__init__(seed, path_expert_indx, T, n_layers, replace_fn=replace_fn, keep_nsfw=keep_nsfw, masks=masks,
                         **kw)
        self.dof_val = dof_val
        self.conf_val = conf_val
        self.trial = trials_per_layer
        self.update_for_t = {}

    def reset_time_layer(self):
        super().reset_time_layer()
        self.update_for_t = {}  # a new run asks again

    def suggest(self, t):
        """The trial's 0/1 answer for timestep t >= 10."""
        if self.trial is None:
            raise ValueError(f"{type(self).__name__} needs trials_per_layer (an optuna trial or a sequence of T 0/1 "
                             f"values) to decide timestep {t}")
        if hasattr(self.trial, "suggest_categorical"):
            return int(self.trial.suggest_categorical(f"timestep_{t}", [0, 1]))
        return int(self.trial[t])

    def decide(self, t, l):
        """Whether the (t, l) call overrides its masked neurons. An empty list never does and asks nothing; the first
        non-empty list of a timestep fixes update_for_t[t]."""
        if self.expert_indices[t][l].size == 0:
            return False
        if t not in self.update_for_t:
            self.update_for_t[t] = 1 if t < FREE_TIMESTEPS else self.suggest(t)
        return self.update_for_t[t] == 1

    def hook_fn(self, module, input, output):
        if self.replace_fn is not GEGLU:
            raise NotImplementedError(f"{type(self).__name__} covers GEGLU projections; the reference's GELU (PixArt) "
                                      "branch is out of scope")
        bits = self.override_bits(module, self.timestep, self.layer) if self.decide(self.timestep, self.layer) else None
        out, gate = module.neurons(input[0], override_bits=bits, override_value=OVERRIDE_VALUE,
                                   want_gate=self.store_gates)
        if self.store_gates:
            self.gates.append(gate.detach().cpu())
        self.update_time_layer()
        return out
