"""ConceptRouter — the concept checkers of the reference's benchmarks/concept_checkers.py as one device launch.

The reference's end-user flow (benchmarks/unified_editing.py:106-126) asks, per prompt, an ArtStyleChecker, a
NudityChecker and a MemorizedPromptChecker which concepts to remove. Each text checker runs its own fp32
CLIPTextModel pass per prompt, pools the 77 token rows, normalises, takes dot products against a bank of concept
features and decides with a few Python comparisons; the answer is a concept name on the host. Here the bank, the
checkers' group records and the row -> select-bit table live on the device, and sdmoe_concept_route turns the
text-encoder rows of a whole batch into the 32-bit select words WandaRemovePerPrompt consumes
(sdmoe_wmask_union_sets, sdmoe_linear_masked_sets) -- no host round trip, and for SD-1.x no second encoder pass: the
checker's text model is the pipeline's own (ViT-L/14, last_hidden_state), so the conditioning rows encode_prompt
wrote are the rows the checkers need (select_from_hidden).

Bank rows, in the order the add_* calls made them (each call: ONE batched encode, then ops.text_pool):
  add_art_styles   one row per concept: mean over the objects of unit(f"a {obj} by {c}") with the RAW concept string
                   (the reference computes preprocess_concepts' short names but never uses them for the bank,
                   concept_checkers.py:20-27, :161), not re-normalised (:44-64); then the no-concept row: the
                   re-normalised mean of unit('a photo of a' + t) -- the missing space is the reference's (:35).
                   Group: fires iff max > no-concept and max > threshold (:179); the bit is the arg-max concept's.
  add_nudity       one row per concept word f"a photo of a {c} {obj}", all labelled `label`; the no-concept row; the
                   anchor row: mean of the unit features of anchor_prompts, not re-normalised (:101-117). The caller
                   draws the anchors (the reference's unseeded np.random.choice of 100 lines, :106, is its business).
                   Group: fires iff max > no-concept, or anchor > no-concept (:127-133).
  add_memorized    no bank row: a host string-membership test (:237-241) that presets the label's bit.
bind(concept_names) fixes each row's select bit from the remover's concept order; a label the remover does not know
gets -1: when that row is the arg-max nothing is removed, even if the runner-up is known (unified_editing.py:116).

Differences from the reference:
  - float64 arithmetic on the fp16 tower's output rows, instead of fp32 arithmetic on the fp32 tower's;
  - prompts are truncated to 77 tokens by the tokenizer call, instead of slicing the ids afterwards (:69-70);
  - a zero feature (an all-zero block of rows: NaN similarities) fires nothing: every comparison on NaN is false, so
    the select word is the preset alone;
  - object_features is normalised once, not twice (:55, :59): the second pass is a no-op to within an ulp.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import SdmoeError

MAX_CONCEPTS = 32
CTX_LEN = 77


class ConceptRouter:
    def __init__(self, text_encoder, tokenizer, device=None):
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        self.device = torch.device(device) if device is not None else text_encoder.device
        self.row_labels = []     # per bank row: the concept label whose bit it sets, or None (no-concept / anchor rows)
        self.row_names = []      # per bank row: what it is, for similarity() and reports
        self.groups = []         # host records (row0, row1, neg_row, anchor_row, threshold)
        self.memorized = []      # [(set of prompts, label)]
        self.bank = None         # device float64 [R, D]
        self.concept_names = None
        self.row_bit = None      # host list, after bind()
        self._dev = None         # (row_bit, groups) on the device, after bind()
        self.last_sims = None    # device float64 [nprompt, R] of the last select

    # ---- encoding ------------------------------------------------------------------------------------------------
    def encode(self, prompts):
        """fp16 last_hidden_state rows [len(prompts) * 77, D] of one batched text-encoder pass."""
        if self.text_encoder is None or self.tokenizer is None:
            raise SdmoeError("ConceptRouter needs a text encoder and a tokenizer to encode prompts")
        ids = self.tokenizer(list(prompts), padding="max_length", max_length=CTX_LEN, truncation=True,
                             return_tensors="pt").input_ids
        return self.text_encoder.encode(ids)["hidden"]

    def _add_rows(self, feats, labels, names):
        row0 = len(self.row_labels)
        if self.bank is not None and self.bank.shape[1] != feats.shape[1]:
            raise SdmoeError(f"bank rows are {self.bank.shape[1]} wide, the new ones {feats.shape[1]}")
        self.bank = feats if self.bank is None else torch.cat([self.bank, feats])
        self.row_labels += labels
        self.row_names += names
        self.row_bit = self._dev = None  # bind() again
        return row0

    def _build(self, concept_prompts, nconcepts, neg_objects, anchor_prompts=()):
        """One batched encode of all bank prompts of a checker; returns float64 [nconcepts + 1 (+ 1), D]:
        the concept rows, the no-concept row, the anchor row if anchors are given."""
        negs = ['a photo of a' + t for t in neg_objects]
        anchors = list(anchor_prompts)
        if not concept_prompts or not negs or len(concept_prompts) % nconcepts:
            raise SdmoeError("a checker needs concepts, objects and neg_objects")
        rows = self.encode(list(concept_prompts) + negs + anchors)
        L = CTX_LEN
        n0, n1 = len(concept_prompts), len(concept_prompts) + len(negs)
        parts = [ops.text_pool(rows[:n0 * L], n0, group=n0 // nconcepts),
                 ops.text_pool(rows[n0 * L:n1 * L], len(negs), group=len(negs), renorm=True)]
        if anchors:
            parts.append(ops.text_pool(rows[n1 * L:], len(anchors), group=len(anchors)))
        return torch.cat(parts)

    # ---- the checkers ----------------------------------------------------------------------------------------------
    def add_art_styles(self, concepts, objects, neg_objects, threshold=0.55):
        concepts, objects = list(concepts), list(objects)
        feats = self._build([f"a {obj} by {c}" for c in concepts for obj in objects], len(concepts), neg_objects)
        row0 = self._add_rows(feats, concepts + [None], [f"art:{c}" for c in concepts] + ["art:none"])
        n = len(concepts)
        self.groups.append((row0, row0 + n, row0 + n, -1, float(threshold)))
        return self

    def add_nudity(self, concepts=('naked', 'sexy'), objects=(), neg_objects=(), anchor_prompts=(), label='naked'):
        concepts, objects = list(concepts), list(objects)
        anchors = list(anchor_prompts)
        feats = self._build([f"a photo of a {c} {obj}" for c in concepts for obj in objects], len(concepts),
                            neg_objects, anchors)
        n = len(concepts)
        labels = [label] * n + [None] + ([None] if anchors else [])
        names = [f"{label}:{c}" for c in concepts] + [f"{label}:none"] + ([f"{label}:anchor"] if anchors else [])
        row0 = self._add_rows(feats, labels, names)
        self.groups.append((row0, row0 + n, row0 + n, row0 + n + 1 if anchors else -1, float("-inf")))
        return self

    def add_memorized(self, prompts, label='memorize'):
        self.memorized.append((set(prompts), label))
        self.row_bit = self._dev = None
        return self

    def set_threshold(self, group, threshold):
        """Replace the threshold of group record `group` (None / -inf = none)."""
        row0, row1, neg, anchor, _ = self.groups[group]
        self.groups[group] = (row0, row1, neg, anchor, float("-inf") if threshold is None else float(threshold))
        self._dev = None
        return self

    # ---- binding to a remover's concept order ----------------------------------------------------------------------
    def labels(self):
        """Every label a checker can answer, in order of first appearance."""
        out = []
        for lab in [l for l in self.row_labels if l is not None] + [lab for _, lab in self.memorized]:
            if lab not in out:
                out.append(lab)
        return out

    def bind(self, concept_names):
        """Fix the select bit of every bank row (and memorized label) from the remover's concept order: bit i for
        concept_names[i], -1 for a label the remover does not know."""
        names = list(concept_names)
        if len(names) > MAX_CONCEPTS:
            raise SdmoeError(f"at most {MAX_CONCEPTS} concepts (one select bit each), got {len(names)}")
        if len(set(names)) != len(names):
            raise SdmoeError(f"concept names must be distinct, got {names}")
        index = {c: i for i, c in enumerate(names)}
        self.concept_names = names
        self.row_bit = [-1 if lab is None else index.get(lab, -1) for lab in self.row_labels]
        self._dev = None
        return self.row_bit

    def _tables(self):
        if self.row_bit is None:
            raise SdmoeError("ConceptRouter.bind(concept_names) has not been called since the last add_*")
        if self._dev is None:
            R = len(self.row_labels)
            self._dev = (torch.tensor(self.row_bit, dtype=torch.int32, device=self.device),
                         ops.concept_groups(self.groups, R, self.device))
        return self._dev

    def preset_words(self, prompts):
        """Host-side decisions as uint32 words: the memorized labels' bits for the prompts that are members."""
        index = {c: i for i, c in enumerate(self.concept_names or [])}
        words = np.zeros(len(prompts), dtype=np.uint32)
        for members, lab in self.memorized:
            if lab in index:
                for i, p in enumerate(prompts):
                    if p in members:
                        words[i] |= np.uint32(1 << index[lab])
        return words

    # ---- routing -----------------------------------------------------------------------------------------------------
    def select_from_hidden(self, rows, nprompt, prompts=None):
        """Select words (int32 device [nprompt], bit patterns of uint32) from fp16 text-encoder rows [nprompt * L, D]
        already on the device; prompts (optional) feeds the memorized checkers' preset. Keeps last_sims."""
        if self.row_bit is None:
            raise SdmoeError("ConceptRouter.bind(concept_names) has not been called since the last add_*")
        preset = None
        if self.memorized and prompts is not None:
            if len(prompts) != nprompt:
                raise SdmoeError(f"{len(prompts)} prompts for {nprompt} blocks of rows")
            preset = torch.from_numpy(self.preset_words(list(prompts)).view(np.int32).copy()).to(self.device)
        if self.bank is None:  # memorized checkers only: nothing to launch
            self.last_sims = None
            return preset if preset is not None else torch.zeros(nprompt, dtype=torch.int32, device=self.device)
        row_bit, groups = self._tables()
        sel, self.last_sims = ops.concept_route(rows, nprompt, self.bank, row_bit, groups, preset=preset)
        return sel

    def select(self, prompts):
        """Select words of a list of prompts: one batched encode, then select_from_hidden."""
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        if self.bank is None:
            return self.select_from_hidden(None, len(prompts), prompts)
        return self.select_from_hidden(self.encode(prompts), len(prompts), prompts)

    def names(self, select):
        """Select words -> per-prompt lists of concept names, in the bound concept order (one device -> host copy:
        for results.json, not for the hot path)."""
        if self.concept_names is None:
            raise SdmoeError("ConceptRouter.bind(concept_names) has not been called")
        words = np.asarray(select.cpu() if isinstance(select, torch.Tensor) else select).astype(np.int64) & 0xFFFFFFFF
        return [[c for i, c in enumerate(self.concept_names) if (int(w) >> i) & 1] for w in words]
