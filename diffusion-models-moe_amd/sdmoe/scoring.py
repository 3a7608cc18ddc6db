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

import json

import torch

from . import ops
from .clip import CLIPModel
from .resnet import ResNet


def _u8_batches(images):
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
        return _u8_batches(images)

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


def match_table(categories, labels):
    """The reference's top-k name match (benchmarks/object_erase.py:253-284) as a bit table: int32 [len(labels),
    ceil(len(categories) / 32)] holding uint32 words, bit c % 32 of word c // 32 of row g set where class c counts as
    a hit for label g. The label is stripped and split on spaces; a class is a hit if any space-separated word of its
    category name is among the label's words. Names are compared as given: the reference lower-cases its labels but
    not the category names, so a capitalised name word never matches ("English springer" matches through "springer",
    never through "English"). That quirk is kept."""
    words = (len(categories) + 31) // 32
    rows = []
    for label in labels:
        want = set(label.strip().split(" "))
        row = [0] * words
        for c, name in enumerate(categories):
            if any(w in want for w in name.split(" ")):
                row[c >> 5] |= 1 << (c & 31)
        rows.append(row)
    t = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), words)
    return torch.where(t >= 1 << 31, t - (1 << 32), t).to(torch.int32)


class ObjectScorer:
    """Object-erasure accuracy (the reference's Imagenette experiment, benchmarks/object_erase.py:247-302 and
    save_union_over_time.py:264-276): every removal image through torchvision's ImageClassification preset and
    resnet50, the top-5 class names matched word by word against the prompt's label, acc = hits / n.

    The reference scores one reloaded PNG per call on the host. Here the images stay on the device:

        quantise (diffusers numpy_to_pil)    sdmoe_clip_quantise
        Pillow-exact bilinear resize to      sdmoe_clip_resample_h/v with the triangle filter's tables, crop offsets
          `resize`, centre crop `size`         int(round((h - size) / 2.0)) (half-even, torchvision's center_crop)
        to_tensor, normalize, stem im2col    sdmoe_stem_rows
        ResNet                               sdmoe.resnet.ResNet, a whole batch in one pass
        top-k, name match, hit count         sdmoe_topk_hits: n k + n + 1 integers leave the device

    model: sdmoe.resnet.ResNet; categories: the class names in class-id order (the caller's data, e.g.
    ResNet50_Weights.DEFAULT.meta["categories"]) or None -- then only the methods that need no names work.
    `images` as for ClipScorer: [B, 3, H, W] floats in [0, 1], [B, H, W, 3] uint8, or a list of such (sizes may
    differ), all on the device. torchvision's tensor-input antialias path is not reproduced: the preset is applied
    as on a PIL image, which is what the reference feeds it."""

    def __init__(self, model: ResNet, categories=None, size: int = 224, resize: int = 232):
        model.config.check_size(size)
        if resize < size:
            raise ValueError(f"resize {resize} is smaller than the crop {size}")
        if categories is not None and len(categories) != model.config.num_classes:
            raise ValueError(f"{len(categories)} category names for {model.config.num_classes} classes")
        self.model = model
        self.categories = None if categories is None else list(categories)
        self.size, self.resize = int(size), int(resize)
        self._tables = {}

    def preprocess_u8(self, images):
        """The resized, centre-cropped uint8 pixels [n, size, size, 3] (what the preset's to_tensor sees)."""
        batches = _u8_batches(images)
        n, S = sum(b.shape[0] for b in batches), self.size
        u8 = torch.empty((n, S, S, 3), dtype=torch.uint8, device=batches[0].device)
        b0 = 0
        for b in batches:
            ops.clip_preprocess(b, S, u8_out=u8[b0:b0 + b.shape[0]], resize=self.resize, filter="bilinear",
                                half_even=True)
            b0 += b.shape[0]
        return u8

    def logits(self, images):
        """fp16 [n, num_classes], all images in one pass."""
        return self.model(self.preprocess_u8(images))

    def _table(self, labels):
        """(device bit table over the distinct labels, device int32 label row per image)."""
        if self.categories is None:
            raise ValueError("ObjectScorer was built without category names (categories=None)")
        distinct = sorted(set(labels))
        key = tuple(distinct)
        table = self._tables.get(key)
        if table is None:
            table = self._tables[key] = match_table(self.categories, distinct).to(self.model.device)
        row = {lab: g for g, lab in enumerate(distinct)}
        return table, torch.tensor([row[lab] for lab in labels], dtype=torch.int32).to(self.model.device)

    def topk(self, images, k: int = 5):
        """The k best class ids per image, int32 [n, k] on the host, descending (ties to the lower id)."""
        lg = self.logits(images)
        n = lg.shape[0]
        table = torch.zeros((1, (lg.shape[1] + 31) // 32), dtype=torch.int32, device=lg.device)
        return ops.topk_hits(lg, table, torch.zeros(n, dtype=torch.int32, device=lg.device), k)[0].cpu()

    def score_erasure(self, images, labels, k: int = 5):
        """object_erase.py:253-302 for n images and their n labels (lower-cased object names, as the reference's
        prompts CSV carries them): {"acc": hits / n, "hits": int32 [n], "topk": int32 [n, k]} (host tensors)."""
        labels = [labels] if isinstance(labels, str) else list(labels)
        table, rows = self._table(labels)
        lg = self.logits(images)
        if lg.shape[0] != len(labels):
            raise ValueError(f"{len(labels)} labels but {lg.shape[0]} images")
        topk, hit, total = ops.topk_hits(lg, table, rows, k)
        out = torch.cat([topk.reshape(-1), hit, total]).cpu()
        n = len(labels)
        if out[-1].item() < 0:
            raise ops._lib.SdmoeError("sdmoe_topk_hits: a label row outside the match table")
        return {"acc": out[-1].item() / n, "hits": out[n * k:n * k + n], "topk": out[:n * k].reshape(n, k)}

    @staticmethod
    def write_results(path, result):
        """results.json in the reference's format (object_erase.py:300-302)."""
        with open(path, "w") as f:
            json.dump({"acc": result["acc"]}, f)
