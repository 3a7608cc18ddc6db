"""The reference's concept checkers (benchmarks/concept_checkers.py) as thin shells over sdmoe.concepts.ConceptRouter.

Same class names, same constructor order (device, objects, neg_objects, concepts_to_remove=...), same
similarity(text) / decide(text) answers, so the loop body of benchmarks/unified_editing.py:106-126 runs unchanged.
There is no from_pretrained here: the text encoder and tokenizer come in as the text_encoder= / tokenizer= keywords
(sdmoe.clip.CLIPTextModel on the HIP kernels), and NudityChecker takes its anchor prompts as anchor_prompts= (left
out, it draws 100 lines of its anchor_file with np.random.choice as the reference does, :104-106).
Each checker owns a ConceptRouter with its one group, bound to its own labels; a batched caller builds ONE router
with all the checkers instead (sdmoe/concepts.py, whose docstring lists the numerical differences from the
reference) and never comes through here.
"""
from __future__ import annotations

import numpy as np

from sdmoe import ops
from sdmoe.concepts import ConceptRouter


_FULL_NAMES = {'Van Gogh': 'Vincent Van Gogh', 'Monet': 'Claude Monet'}


def preprocess_concepts(concepts_to_remove):
    """(the non-empty concepts, their short names: the text before the first comma, two artists spelled out) --
    the contract of concept_checkers.py:8-17. The short names are returned for callers that print them; the bank
    never uses them, there or here."""
    kept = [c for c in concepts_to_remove if c != '']
    short = [c.split(",")[0] for c in kept]
    return kept, [_FULL_NAMES.get(c, c) for c in short]


art_styles = ['Alex Alemany,painter', 'Van Gogh', 'Monet', 'Pablo Picasso']


class BaseConceptChecker:
    def __init__(self, device, objects, concepts_to_remove, text_encoder=None, tokenizer=None):
        self.concepts_to_remove = list(concepts_to_remove)
        self._bank_concepts = list(concepts_to_remove)  # the bank's rows, in order ('' included, as the reference)
        self.device = device
        self.list_of_objects = list(objects)
        self.router = ConceptRouter(text_encoder, tokenizer, device)

    def format_prompt(self, obj, concept=None):
        raise NotImplementedError

    def _route(self, text):
        rows = self.router.encode([text])
        sel = self.router.select_from_hidden(rows, 1)
        return rows, sel, self.router.last_sims[0]

    def similarity(self, text):
        """({concept: its similarity, a float64 device tensor [1]}, the prompt's unit feature [1, D])."""
        rows, _, sims = self._route(text)
        return {c: sims[i:i + 1] for i, c in enumerate(self._bank_concepts)}, ops.text_pool(rows, 1)

    def decide(self, text):
        raise NotImplementedError


class NudityChecker(BaseConceptChecker):
    anchor_file = 'modularity/datasets/i2p_prompts_seed_0_CompVis_stable-diffusion-v1-4.txt'

    def __init__(self, device, objects, neg_objects, concepts_to_remove=('naked', 'sexy'), text_encoder=None,
                 tokenizer=None, anchor_prompts=None):
        super().__init__(device, objects, concepts_to_remove, text_encoder, tokenizer)
        self.neg_objects = list(neg_objects)
        if anchor_prompts is None:
            with open(self.anchor_file, 'r') as f:
                anchor_prompts = list(np.random.choice(f.readlines(), 100))
        self.anchor_prompts = list(anchor_prompts)
        self.router.add_nudity(self.concepts_to_remove, self.list_of_objects, self.neg_objects, self.anchor_prompts,
                               label='naked')
        self.router.bind(['naked'])
        self.concepts_to_remove, self.concept_labels = preprocess_concepts(self.concepts_to_remove)

    def format_prompt(self, obj, c):
        return f"a photo of a {c} {obj}"

    def decide(self, text):
        _, sel, _ = self._route(text)
        return 'naked' if self.router.names(sel)[0] else 'none'


class ArtStyleChecker(BaseConceptChecker):
    def __init__(self, device, objects, neg_objects, concepts_to_remove=art_styles, text_encoder=None, tokenizer=None):
        super().__init__(device, objects, concepts_to_remove, text_encoder, tokenizer)
        self.neg_objects = list(neg_objects)
        self.threshold = 0.55
        self.router.add_art_styles(self.concepts_to_remove, self.list_of_objects, self.neg_objects, self.threshold)
        self.router.bind(self.router.labels())
        self.concepts_to_remove, _ = preprocess_concepts(self.concepts_to_remove)

    def format_prompt(self, obj, c):
        return f"a {obj} by {c}"

    def decide(self, text):
        _, sel, _ = self._route(text)
        names = self.router.names(sel)[0]
        return names[0] if names else 'none'


class MemorizedPromptChecker:
    def __init__(self, device, objects, neg_objects, concepts_to_remove=('memorize',), prompts=None,
                 parquet='modularity/datasets/sdv1_bb_edge_groundtruth.parquet', **unused):
        self.device = device
        if prompts is None:
            import pandas as pd
            prompts = pd.read_parquet(parquet)['caption'].values.tolist()
        self.prompts = list(prompts)
        self.threshold = 0.9

    def format_prompt(self, obj, concept=None):
        return obj

    def decide(self, text):
        return 'memorize' if text in self.prompts else 'none'
