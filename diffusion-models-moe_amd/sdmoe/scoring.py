"""Removal-quality scores on the device: the reference's only published numbers (`benchmarking results/**/
results.txt`), computed by benchmarks/artist_removal.py:173-215 ("Average CLIP score": mean CLIP image-image cosine of
the original and the removal image; "Average accuracy": share of prompts whose text-image cosine dropped after the
removal) and benchmarks/art_removal.py:80-127 (per-concept mean / std of the image-image cosine).

The reference saves PNGs, reloads them, resizes on the host with Pillow (CLIPProcessor) and runs fp32 CLIPModel on
the CPU one image per call. Here the images stay on the device from `pipe(..., output_type="pt")` to the scores:

    quantise (diffusers numpy_to_pil)   sdmoe_clip_quantise     [B, 3, H, W] fp16/fp32 -> uint8 NHWC
    Pillow-exact bicubic + centre crop  sdmoe_clip_resample_h/v uint8 intermediate, crop window only
    rescale, normalise, patchify        in the vertical pass's store: the patch GEMM's fp16 A operand
    vision / text towers                sdmoe.clip.CLIPModel    a whole batch of images in one pass
    cosines, sums, accuracy count       sdmoe_clip_scores       float64, fixed order; 3 n + 3 doubles leave the device

The uint8 pixels are bit-identical to Pillow's (tests/test_gpu_clip_score.py); the towers run fp16 storage / fp32
accumulation like the text encoder. There is no host path: images not on a GPU raise.
"""
from __future__ import annotations

import torch

from . import ops
from .clip import CLIPModel


class ClipScorer:
    """CLIP scores of (prompt, original image, removal image) triples.

    model: sdmoe.clip.CLIPModel; tokenizer: a transformers-style tokenizer (SyntheticCLIPTokenizer by default
    elsewhere in the package); size: the processor's shortest edge and crop (224 for the OpenAI checkpoints; it must
    equal the vision tower's image_size).

    `images` everywhere: one [B, 3, H, W] fp16 / fp32 tensor in [0, 1] (`output_type="pt"`), one [B, H, W, 3] uint8
    tensor, or a list of such tensors (3-D entries are single images; sizes may differ) -- all on the device."""

    def __init__(self, model: CLIPModel, tokenizer, size: int = 224):
        if size != model.vision_model.config.image_size:
            raise ValueError(f"size {size} is not the vision tower's image_size "
                             f"{model.vision_model.config.image_size}")
        self.model = model
        self.tokenizer = tokenizer
        self.size = int(size)
        self.patch = model.vision_model.config.patch_size

    # -- front end ---------------------------------------------------------------------------------------------
    def _u8_batches(self, images):
        """images -> list of contiguous uint8 [b, H, W, 3] device batches (quantised where they are floats)."""
        items = list(images) if isinstance(images, (list, tuple)) else [images]
        out = []
        for t in items:
            if not torch.is_tensor(t):
                raise TypeError(f"images must be device tensors, got {type(t).__name__}")
            if t.dim() == 3:
                t = t[None]
            if t.dim() != 4:
                raise ValueError(f"image tensor of shape {tuple(t.shape)}: expected [B, 3, H, W] or [B, H, W, 3]")
            if t.dtype == torch.uint8:
                if t.shape[3] != 3:
                    raise ValueError(f"uint8 images must be NHWC [B, H, W, 3], got {tuple(t.shape)}")
                out.append(t.contiguous())
            else:
                out.append(ops.clip_quantise(t.contiguous()))
        return out

    def _run(self, images, want_a, want_u8):
        batches = self._u8_batches(images)
        n = sum(b.shape[0] for b in batches)
        S, dev = self.size, batches[0].device
        a = u8 = None
        if want_a:
            G2 = (S // self.patch) ** 2
            a = torch.empty((n * G2, ops.clip_padded_k(self.patch)), dtype=torch.float16, device=dev)
        if want_u8:
            u8 = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
        b0 = 0
        for b in batches:
            nb = b.shape[0]
            ops.clip_preprocess(b, S, self.patch,
                                a_out=None if a is None else a[b0 * G2:(b0 + nb) * G2],
                                u8_out=None if u8 is None else u8[b0:b0 + nb])
            b0 += nb
        return a, u8

    def preprocess(self, images):
        """The patch-embedding GEMM's A operand, fp16 [n * G^2, Kpad]: CLIPImageProcessor's pixel_values, patchified."""
        return self._run(images, True, False)[0]

    def preprocess_u8(self, images):
        """The resized, centre-cropped uint8 pixels [n, size, size, 3] (what Pillow hands the processor)."""
        return self._run(images, False, True)[1]

    # -- features ----------------------------------------------------------------------------------------------
    def image_features(self, images):
        """CLIPModel.get_image_features of the images, fp16 [n, projection_dim], in one pass."""
        return self.model.get_image_features(self.preprocess(images))

    def text_features(self, prompts):
        """CLIPModel.get_text_features of the prompts, fp16 [n, projection_dim]."""
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        return self.model.get_text_features(self.tokenizer(prompts).input_ids)

    # -- scores ------------------------------------------------------------------------------------------------
    def _pair_features(self, orig_images, removed_images):
        """Both image sets through the tower in one batch -> (orig rows, removal rows)."""
        bo, br = self._u8_batches(orig_images), self._u8_batches(removed_images)
        n = sum(b.shape[0] for b in bo)
        if n != sum(b.shape[0] for b in br):
            raise ValueError("orig_images and removed_images differ in count")
        f = self.model.get_image_features(self.preprocess(bo + br))  # one A operand: removal rows at batch offset n
        return f[:n], f[n:]

    def score_removal(self, prompts, orig_images, removed_images):
        """artist_removal.py:180-207 for n prompts: per-prompt `similarity_orig`, `similarity_removed`, `image_sim`
        (float64 host tensors), `average_clipscore` (mean image_sim) and `average_acc` (share with similarity_orig >
        similarity_removed, strict)."""
        t = self.text_features(prompts)
        fo, fr = self._pair_features(orig_images, removed_images)
        n = t.shape[0]
        if fo.shape[0] != n:
            raise ValueError(f"{n} prompts but {fo.shape[0]} image pairs")
        out = ops.clip_scores(t, fo, fr).cpu()
        return {"similarity_orig": out[:n], "similarity_removed": out[n:2 * n], "image_sim": out[2 * n:3 * n],
                "average_clipscore": out[3 * n].item() / n, "average_acc": out[3 * n + 2].item() / n}

    def image_similarity(self, orig_images, removed_images):
        """art_removal.py:114-125: per-pair image-image cosines `sim` with their `mean_sim` and population `std`
        (np.mean / np.std)."""
        fo, fr = self._pair_features(orig_images, removed_images)
        n = fo.shape[0]
        out = ops.clip_scores(None, fo, fr).cpu()
        mean = out[3 * n].item() / n
        var = max(out[3 * n + 1].item() / n - mean * mean, 0.0)
        return {"sim": out[2 * n:3 * n], "mean_sim": mean, "std": var ** 0.5}

    @staticmethod
    def write_results(path, result):
        """results.txt in the reference's format (artist_removal.py:213-215)."""
        with open(path, "w") as f:
            f.write(f"Average CLIP score: {result['average_clipscore']}\n")
            f.write(f"Average accuracy: {result['average_acc']}\n")
