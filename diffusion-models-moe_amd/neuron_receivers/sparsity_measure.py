"""SparsityMeasure — drop-in for neuron_receivers/sparsity_measure.py:6-45: how sparse the FFN gates of a (relufied)
U-Net are, the measurement sparsity/check_sparsity.py turns into sparsity.json.

Reference (:13-18): every hooked GEGLU call copies its activated gate to the host; the driver then counts `gate == 0.0`
per call on the CPU (check_sparsity.py:41-46) and test() asserts `torch.all(gate >= 0)` over all of them (:39-41).
MI355X path: `GEGLU.sparsity` — the projection GEMM plus one streaming pass (sdmoe_geglu_sparsity) that writes the
dense product and counts on the device: per call and group of images the gate elements with |act(gate)| <= threshold
(threshold 0: the exact zeros of either sign, `gate == 0.0`), the elements with act(gate) < 0, and with per_neuron=True
the zero rows of every neuron. The counts of a whole pipeline call stay on the device and are copied to the host once,
when observe_activation returns (flush(); flush_count counts the copies). `calls` then holds one record per hooked
call, in call order:
    {"zeros": int64 [G], "negatives": int64 [G], "elements": int64 [G], "rows": int64 [G],
     "neuron_zeros": int32 [G, F] (per_neuron only)}
with G the number of groups. sdmoe.discovery.sparsity_ratios / accumulate_sparsity / neuron_zero_fraction turn them
into the driver's per-call ratio, its StatMeter and sparsity.json, and per-neuron zero fractions.
Differences from the reference:
  * counts, not gates: with store_gates=False nothing but the counts leaves the device. With store_gates=True (the
    base default) observe_activation still returns the list of host gates, so the reference's driver runs unchanged.
  * the ratio zeros / elements is the exact value of the driver's "mean over tokens of (zeros in the row / F)", which
    the driver evaluates in fp32 (a rounding difference below 1e-6).
  * test() asserts that the device's negative count is 0 for every call; no gate is stored for it.
  * prompt batches (this port's addition): a single prompt string is one group over every image of the call (the
    reference's [2, N, F] gate under guidance); a list of B prompts gives B groups, image i -> prompt i % B.
Out of scope: a replace_fn other than GEGLU (the PixArt GELU projection) — hook_fn raises NotImplementedError.
"""
from __future__ import annotations

import numpy as np
import torch

from neuron_receivers.base_receiver import GEGLU, BaseNeuronReceiver
from neuron_receivers.prompt_groups import PromptGroups


class SparsityMeasure(PromptGroups, BaseNeuronReceiver):
    def __init__(self, seed, threshold=0.0, per_neuron=False, **kw):
        super().__init__(seed, **kw)
        if not float(threshold) >= 0.0:
            raise ValueError(f"SparsityMeasure: threshold must be >= 0, got {threshold!r}")
        self.threshold = float(threshold)
        self.per_neuron = bool(per_neuron)
        self.calls = []         # one record per hooked call (filled by flush())
        self._pending = []      # (device totals [G, 2], device neuron zeros [G, F] or None, rows [G], F) per call
        self.flush_count = 0    # device->host copies done by flush() (one per pipeline call)

    def hook_fn(self, module, input, output):
        if self.replace_fn is not GEGLU:
            raise NotImplementedError("SparsityMeasure covers GEGLU projections; the reference's GELU (PixArt) "
                                      "projection is out of scope")
        x = input[0]
        nimg, ngroups, table = self.groups_of(x)
        F = module.inner_dim
        totals = torch.empty((ngroups, 2), dtype=torch.int64, device=x.device)
        col_zero = torch.empty((ngroups, F), dtype=torch.int32, device=x.device) if self.per_neuron else None
        out, gate = module.sparsity(x, threshold=self.threshold, col_zero=col_zero, totals=totals,
                                    img_group=table, ngroups=ngroups, want_gate=self.store_gates)
        if self.store_gates:
            self.gates.append(gate.detach().cpu())
        seq_len = x.shape[-2]
        groups = [0] * nimg if self._nprompts is None else self.image_table(nimg)
        rows = [seq_len * groups.count(g) for g in range(ngroups)]
        self._pending.append((totals, col_zero, rows, F))
        return out

    def flush(self):
        """Materialise the pending device counts (one device->host copy) as records appended to `calls`."""
        if not self._pending:
            return
        pending, self._pending = self._pending, []
        parts = [p[0].reshape(-1) for p in pending] + [p[1].reshape(-1).to(torch.int64) for p in pending
                                                       if p[1] is not None]
        flat = torch.cat(parts).cpu().numpy()
        self.flush_count += 1
        o = 2 * sum(p[0].shape[0] for p in pending)
        t = 0
        for totals, col_zero, rows, F in pending:
            G = totals.shape[0]
            tz = flat[t:t + 2 * G].reshape(G, 2)
            t += 2 * G
            rows = np.asarray(rows, dtype=np.int64)
            rec = {"zeros": tz[:, 0].copy(), "negatives": tz[:, 1].copy(), "elements": rows * F, "rows": rows}
            if col_zero is not None:
                rec["neuron_zeros"] = flat[o:o + G * F].reshape(G, F).astype(np.int32)
                o += G * F
            self.calls.append(rec)

    def observe_activation(self, model, ann, bboxes=None):
        self.set_prompts(ann)
        self.calls = []
        self._pending = []
        try:
            return super().observe_activation(model, ann, bboxes)
        finally:
            self.flush()

    def check_no_negatives(self):
        """sparsity_measure.py:39-41 from the counts: no hooked call saw a negative activated gate."""
        for i, rec in enumerate(self.calls):
            assert int(np.sum(rec["negatives"])) == 0, f"Relu failed (hooked call {i}: {rec['negatives'].tolist()} " \
                                                       f"negative gates)"

    def test(self, model, ann='A brown dog in the snow'):
        """sparsity_measure.py:20-45: one hooked run of `ann` (seeds 0, as the reference), then every call's negative
        count must be 0 -- true exactly for a relufied U-Net. No gate is stored and no image is saved; `calls` keeps
        the run's records. Returns the image."""
        keep, seed = self.store_gates, self.seed
        self.store_gates, self.seed = False, 0
        try:
            out, _ = self.observe_activation(model, ann)
        finally:
            self.store_gates, self.seed = keep, seed
        self.check_no_negatives()
        self.gates = []
        return out
