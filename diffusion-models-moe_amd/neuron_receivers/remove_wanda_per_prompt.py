"""WandaRemovePerPrompt — a different concept set for each prompt of ONE batched pipeline call.

The reference's end-user removal flow (benchmarks/unified_editing.py:106-126) routes every prompt through its concept
checkers and calls MultiConceptRemoverWanda.remove_concepts(model, prompt, concepts_for_this_prompt): one prompt per
call, and for more than one concept a host-side OR over every (t, l) mask first (multi_concept_remover.py:43-53).
WandaRemoveNeuronsFast applies ONE mask per (t, l) to the whole call, so a stream of prompts with different concept
subsets could not use the batched engine. This receiver can: prompt i of the batch gets the union of ITS concepts'
Wanda masks on every hooked `ff.net.2`, a prompt with no concepts runs unmasked, and the down projection is still one
launch per layer at the full grid (sdmoe_linear_masked_sets: every row tile stages the mask of its image's set).

Same seam as WandaRemoveNeuronsFast: linear_hook_fn on the plain FFN, fused_linear on the routed one (mask columns
permuted by the layer's perm, top-k keep bits in the same launch), the (t, l) counter advancing once per hooked call.
Built from {concept: WandaRemoveNeuronsFast} (at most 32: a set is a 32-bit select word). set_prompt_concepts() fixes
the next call's distinct sets, their select words and the per-prompt set ids; the image table covers all U-Net
images -- with classifier-free guidance image b and image B + b both take prompt b's set.
Per hooked call: one sdmoe_wmask_union_sets launch makes the call's distinct unions from the stacked concept masks
into a reused buffer, then one sdmoe_linear_masked_sets. At latents under 8x8 (rows per image not a multiple of 64)
ops.linear_masked_sets runs sdmoe_linear_masked once per run of images on one set instead.

The union is EXACTLY the listed concepts. MultiConceptRemoverWanda's shared union remover starts from the last
configured concept's masks and keeps OR-ing across calls until it is reset (multi_concept_remover.py:24-41); none of
that applies here.

HBM: the concept masks of every (t, l) are held stacked [nconcepts][4C/64][C] in the masked GEMM's K-step-major
layout, converted once per (t, l, perm) straight from each remover's packed device bits (the conversion of
WandaRemoveNeuronsFast.device_kmajor, written into the stack so no second per-remover copy is kept) -- as many bytes
as the packed bits again: 316 MB per concept for SD-1.4 at T = 51, on top of the removers' own 316 MB each. The
union buffer is nsets masks of the largest layer (0.8 MB each for SD-1.4).

set_prompt_select() takes the call's select words as a device tensor instead (sdmoe.concepts.ConceptRouter writes
them): one set per prompt, the identity image table, no host copy and no dedupe -- which costs nsets = B unions per
hooked call instead of the number of distinct sets. With router= and no sets configured, observe_activation registers
a prompt hook for the call (StableDiffusionPipeline.register_prompt_hook): on an SD-1.x pipeline whose text encoder is
the router's own the router reads the conditional rows encode_prompt just wrote, otherwise (SDXL, synthetic
conditioning, another encoder) it encodes the prompts itself; either way the words go from sdmoe_concept_route straight into the union launch.

hook_module='unet' only: the text-encoder variant and the GEGLU-gate variant raise SdmoeError.
"""
from __future__ import annotations

import numpy as np
import torch

from sdmoe import ops
from sdmoe._lib import SdmoeError
from sdmoe.unet import LoRACompatibleLinear

from neuron_receivers.base_receiver import GEGLU
from neuron_receivers.predictivity import NeuronPredictivity

MAX_CONCEPTS = 32


class WandaRemovePerPrompt(NeuronPredictivity):
    _sdmoe_fused_nimg = True  # sdmoe.unet.FeedForward passes fused_linear the call's image count

    def __init__(self, removers, seed=0, replace_fn=GEGLU, keep_nsfw=False, hook_module='unet', router=None, **kw):
        removers = dict(removers)
        if not removers:
            raise SdmoeError("WandaRemovePerPrompt needs at least one concept remover")
        if len(removers) > MAX_CONCEPTS:
            raise SdmoeError(f"at most {MAX_CONCEPTS} concepts (one select bit each), got {len(removers)}")
        if hook_module != 'unet':
            raise SdmoeError(f"WandaRemovePerPrompt hooks the U-Net's ff.net.2 only, got hook_module={hook_module!r}")
        first = next(iter(removers.values()))
        for c, r in removers.items():
            if (r.T, r.n_layers) != (first.T, first.n_layers):
                raise SdmoeError(f"concept {c!r} has (T, n_layers) = {(r.T, r.n_layers)}, expected "
                                 f"{(first.T, first.n_layers)}")
        super().__init__(seed, first.T, first.n_layers, replace_fn, keep_nsfw, hook_module, **kw)
        self.removers = removers
        self.concepts = list(removers)
        self.sets, self.select, self.prompt_sets = [], [], []
        self.router = router     # sdmoe.concepts.ConceptRouter or None: routes a call that has no sets configured
        self._select_dev = None  # set_prompt_select: the call's select words, on the device
        self.last_select = None  # the select words the router wrote for the last routed call
        self._dev = {}     # ("stack", t, l, perm is None) -> (perm, the removers' packed masks, stacked device masks)
        self._tables = {}  # per-call device state: the select words, image tables by image count, union buffers

    # ---- per-call setup (host only) ------------------------------------------------------------------------------
    def set_prompt_concepts(self, concepts_per_prompt):
        """Fix the next call's concept sets: concepts_per_prompt[i] lists prompt i's concepts (empty = unmasked).
        Distinct sets (frozensets of names, in order of first use) get ids; self.select[s] has bit c set for concept
        number c of set s; self.prompt_sets[i] is prompt i's set id."""
        index = {c: i for i, c in enumerate(self.concepts)}
        sets, ids = [], []
        for cs in concepts_per_prompt:
            if isinstance(cs, str):
                raise SdmoeError(f"each prompt takes a LIST of concepts, got the string {cs!r}")
            for c in cs:
                if c not in index:
                    raise SdmoeError(f"unknown concept {c!r} (known: {', '.join(map(str, self.concepts))})")
            s = frozenset(cs)
            if s not in sets:
                sets.append(s)
            ids.append(sets.index(s))
        self.sets = sets
        self.select = [sum(1 << index[c] for c in s) for s in sets]
        self.prompt_sets = ids
        self._select_dev = None
        self._tables = {}
        return ids

    def set_prompt_select(self, select_dev):
        """Fix the next call's sets from select words already on the device (int32 [B], bit patterns of uint32 words,
        bit c = concept number c): one set per prompt, in prompt order, the identity image table [0..B-1] (twice over
        under guidance). The words are used as they are: no host copy, no dedupe, so every hooked call makes B unions
        where set_prompt_concepts makes one per distinct set."""
        if not isinstance(select_dev, torch.Tensor) or select_dev.dtype != torch.int32 or select_dev.dim() != 1 \
                or select_dev.numel() == 0:
            raise SdmoeError("set_prompt_select takes an int32 device tensor [B >= 1] of select words")
        if not select_dev.is_cuda:
            raise SdmoeError("set_prompt_select: the select words are not on a GPU device")
        B = select_dev.numel()
        self.sets, self.select = None, None
        self.prompt_sets = list(range(B))
        self._select_dev = select_dev.contiguous()
        self._tables = {}
        return self.prompt_sets

    def clear_prompt_sets(self):
        self.sets, self.select, self.prompt_sets = [], [], []
        self._select_dev = None
        self._tables = {}

    def image_table(self, nimg):
        """Set id of each of the call's nimg U-Net images: the prompts' ids, twice over ([uncond x B ; cond x B]) under
        classifier-free guidance."""
        B = len(self.prompt_sets)
        if B and nimg == B:
            return list(self.prompt_sets)
        if B and nimg == 2 * B:
            return list(self.prompt_sets) * 2
        raise SdmoeError(f"the call runs {nimg} U-Net images, but set_prompt_concepts configured {B} prompts "
                         f"(expected {B} or, with guidance, {2 * B} images)")

    # ---- device state ------------------------------------------------------------------------------------------------
    def stacked_masks(self, t, l, device, perm=None):
        """int64 [nconcepts, 4C/64, C]: every concept's (t, l) mask in sdmoe_linear_masked's layout, columns permuted
        by perm (int32 device [4C]) if given. Built once per (t, l, perm) and cached under WandaRemoveNeuronsFast's
        identity rules: the entry holds the perm tensor itself and is matched by identity, a new perm for the same
        (t, l) replaces it -- and so does a remover whose packed (t, l) mask was replaced (set_mask_bits)."""
        key = ("stack", t, l, perm is None)
        packed = tuple(r.mask_bits[t][l] for r in self.removers.values())
        ent = self._dev.get(key)
        if ent is None or ent[0] is not perm or len(ent[1]) != len(packed) or \
                any(a is not b for a, b in zip(ent[1], packed)):
            rs = list(self.removers.values())
            bits = [r.device_bits(t, l, device) for r in rs]
            N, K = bits[0].shape[0], bits[0].shape[1] * 8
            if any(tuple(b.shape) != (N, K // 8) for b in bits):
                raise ValueError(f"concept masks ({t},{l}) differ in shape: {[tuple(b.shape) for b in bits]}")
            stack = torch.empty((len(rs), K // 64, N), dtype=torch.int64, device=device)
            for c, b in enumerate(bits):
                ops.wmask_kmajor(b, perm, out=stack[c])
            ent = self._dev[key] = (perm, packed, stack)
        return ent[2]

    def _call_state(self, nimg, shape, device):
        """(select words on the device, host image table, its device copy, union buffer [nsets, *shape])."""
        sel = self._select_dev if self._select_dev is not None else self._tables.get(("select", device))
        if sel is None:
            words = np.array(self.select, dtype=np.uint32).view(np.int32)
            sel = self._tables[("select", device)] = torch.from_numpy(words.copy()).to(device)
        tab = self._tables.get(("table", nimg, device))
        if tab is None:
            host = self.image_table(nimg)
            tab = self._tables[("table", nimg, device)] = (host, torch.tensor(host, dtype=torch.int32, device=device))
        buf = self._tables.get(("union", shape, device))
        if buf is None:
            buf = self._tables[("union", shape, device)] = torch.empty((sel.numel(),) + shape, dtype=torch.int64,
                                                                      device=device)
        return sel, tab[0], tab[1], buf

    def _masked(self, module, x2d, weight, keep, perm, residual, nimg):
        if nimg <= 0 or x2d.shape[0] % nimg:
            raise SdmoeError(f"{x2d.shape[0]} rows are not {nimg} whole images")
        dev = module.weight.device
        stack = self.stacked_masks(self.timestep, self.layer, dev, perm)
        N, K = module.weight.shape
        if tuple(stack.shape[1:]) != (K // 64, N):
            raise ValueError(f"ff.net.2 mask ({self.timestep},{self.layer}) for a [{stack.shape[2]}, "
                             f"{stack.shape[1] * 64}] weight does not match weight {tuple(module.weight.shape)}")
        sel, table, table_dev, buf = self._call_state(nimg, tuple(stack.shape[1:]), dev)
        unions = ops.wmask_union_sets(stack, sel, out=buf)
        y = ops.linear_masked_sets(x2d, weight, module.bias, wmasks=unions, image_set=table, image_set_dev=table_dev,
                                   rows_per_img=x2d.shape[0] // nimg, keep=keep, residual=residual)
        self.update_time_layer()
        return y

    # ---- the receiver seam -----------------------------------------------------------------------------------------
    def fused_linear(self, module, x2d, keep, perm, weight_perm, residual, nimg=None):
        """WandaRemoveNeuronsFast.fused_linear with a mask per image: x2d is the GEGLU product in the experts' neuron
        order perm, keep its top-k keep bits (or None), weight_perm ff.net.2's weight in that order; nimg the call's
        image count (sdmoe.unet.FeedForward.run). Returns y + residual; advances the (t, l) counter."""
        if nimg is None:
            raise SdmoeError("WandaRemovePerPrompt.fused_linear needs the call's image count (nimg)")
        return self._masked(module, x2d, weight_perm, keep, perm, residual, nimg)

    def linear_hook_fn(self, module, input, output):
        x = input[0]
        if x.dim() < 3:
            raise SdmoeError(f"ff.net.2 input must be [images, tokens, 4C], got {tuple(x.shape)}")
        y = self._masked(module, x.reshape(-1, x.shape[-1]), module.weight, None, None, None, x.shape[0])
        return y.view(*x.shape[:-1], module.weight.shape[0])

    def hook_fn(self, module, input, output):
        raise SdmoeError("WandaRemovePerPrompt has no GEGLU-gate variant (masks over ff.net.2 only)")

    def text_hook_fn(self, module, input, output):
        raise SdmoeError("WandaRemovePerPrompt has no text-encoder variant (hook_module='unet' only)")

    def hook_modules(self, model):
        if self.hook_module != 'unet':
            raise SdmoeError(f"WandaRemovePerPrompt hooks the U-Net's ff.net.2 only, got {self.hook_module!r}")
        # remove_wanda_neurons_fast.py:107-112: LoRACompatibleLinear, 'ff.net' in name, not a '.proj'
        return [(n, m) for n, m in model.unet.named_modules()
                if isinstance(m, LoRACompatibleLinear) and 'ff.net' in n and 'proj' not in n]

    def prepare(self, model):
        for r in self.removers.values():
            r.prepare(model)

    def register_hooks(self, model, bboxes=None):
        return [self._register(m, self.linear_hook_fn) for _, m in self.hook_modules(model)]

    def _route_hook(self, model):
        """The prompt hook of a routed call: the router's select words for the call's prompts -> set_prompt_select."""
        from sdmoe.unet import CTX_LEN

        def hook(prompts, ctx, B):
            router = self.router
            if router.row_bit is None or router.concept_names != self.concepts:
                router.bind(self.concepts)
            # the conditional rows are the checkers' rows only when the router's bank came from the same encoder
            if model.text_encoder is not None and not model.is_sdxl and model.text_encoder is router.text_encoder:
                sel = router.select_from_hidden(ctx[B * CTX_LEN:], B, prompts)
            else:
                sel = router.select(prompts)
            self.last_select = sel
            self.set_prompt_select(sel)
        return hook

    def observe_activation(self, model, ann, bboxes=None):
        prompts = [ann] if isinstance(ann, str) else list(ann)
        if self.router is not None and not self.prompt_sets:
            handle = model.register_prompt_hook(self._route_hook(model))
            self.prepare(model)
            try:
                return super().observe_activation(model, ann, bboxes)
            finally:
                handle.remove()
                self.clear_prompt_sets()
        if len(prompts) != len(self.prompt_sets):
            raise SdmoeError(f"the call has {len(prompts)} prompts, set_prompt_concepts configured "
                             f"{len(self.prompt_sets)}")
        self.prepare(model)
        return super().observe_activation(model, ann, bboxes)
