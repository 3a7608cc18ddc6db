"""NeuronPredictivityBB — drop-in for neuron_receivers/neuron_predictivity_bb.py:9-63: NeuronPredictivity with the
maximum restricted to the bounding-box token positions of every image (`module.bounding_box`, set from the
`bboxes` argument of observe_activation: gate[:, bounding_box, :], :51-58).

The position list becomes a bit per token position once per (module, list) and rides along the same streaming pass
(sdmoe_geglu_neurons pos_bits); the module output is the dense product over every token, box or not.
Bounding boxes: None, an empty list or an index out of range falls back to all tokens (the reference's try/except
does; the same rule as GetExperts).
Fixed defect: the counter wraps at n_layers - 1 instead of the reference's hard-coded 15 (identical for SD-1.x's 16
layers; the fix GetExperts documents).
"""
from __future__ import annotations

from sdmoe import ops

from neuron_receivers.predictivity import NeuronPredictivity


class NeuronPredictivityBB(NeuronPredictivity):
    def position_bits(self, module, seq_len, device):
        bb = getattr(module, "bounding_box", None)
        if bb is None:
            return None
        idx = [int(i) for i in bb]
        if not idx or any(i < -seq_len or i >= seq_len for i in idx):
            return None  # reference: gate[:, bb, :] raises (or selects nothing) -> all tokens
        idx = [i % seq_len for i in idx]
        key = (tuple(idx), seq_len, str(device))
        cache = getattr(module, "_sdmoe_bb_bits", None)
        if cache is None or cache[0] != key:
            module._sdmoe_bb_bits = cache = (key, ops.position_bits(idx, seq_len, device))
        return cache[1]
