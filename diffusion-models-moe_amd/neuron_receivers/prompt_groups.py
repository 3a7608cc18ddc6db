"""PromptGroups — the prompt-batch grouping shared by the receivers whose statistics are kept per prompt
(NeuronPredictivity and its subclasses, SparsityMeasure): this port's addition, the reference runs one prompt per call.

A single prompt string is one group over every image of the call. For a list of B prompts the U-Net runs
[uncond x B ; cond x B], image i belongs to prompt i % B, and the device kernels take that table as their img_group.
"""
from __future__ import annotations

import torch

from sdmoe._lib import SdmoeError


class PromptGroups:
    _nprompts = None    # None: a single prompt (one group); B: a list of B prompts
    _img_tables = None  # (image count, device) -> int32 device image -> prompt table

    def set_prompts(self, ann):
        """Fix the grouping of the next calls: a prompt string (or None) is one group over every image, a list of B
        prompts gives B groups."""
        self._nprompts = None if ann is None or isinstance(ann, str) else len(ann)
        self._img_tables = {}

    def image_table(self, nimg):
        """Prompt of each of the call's nimg U-Net images: i % B for B or, under guidance, 2 B images."""
        B = self._nprompts
        if B and nimg in (B, 2 * B):
            return [i % B for i in range(nimg)]
        raise SdmoeError(f"the call runs {nimg} U-Net images, but {B} prompts were configured (expected {B} or, with "
                         f"guidance, {2 * B if B else 0} images)")

    def _image_table_dev(self, nimg, device):
        if self._img_tables is None:
            self._img_tables = {}
        key = (nimg, device)
        tab = self._img_tables.get(key)
        if tab is None:
            tab = self._img_tables[key] = torch.tensor(self.image_table(nimg), dtype=torch.int32, device=device)
        return tab

    def groups_of(self, x):
        """(image count, group count, device image -> group table or None) of a hooked call's input x."""
        nimg = x.shape[0] if x.dim() >= 3 else 1
        if self._nprompts is None:
            return nimg, 1, None
        return nimg, self._nprompts, self._image_table_dev(nimg, x.device)
