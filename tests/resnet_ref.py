"""CPU restatement of the object-erasure scorer (sdmoe/scoring.py ObjectScorer, sdmoe/resnet.py, csrc/imagenet.hip).

Front end: torchvision's ImageClassification preset on a PIL image -- resize the shortest edge to `resize` (long edge
int(resize * long / short)) with Image.resize(BILINEAR) through Pillow itself, centre crop at int(round((h - crop) /
2.0)) (Python's half-even round), u8 / 255, (x - mean) / std in fp32 -- and the stem's im2col A operand in NumPy.
Network: torchvision's ResNet (v1.5 bottleneck) in plain fp32 torch: F.conv2d, eval-mode F.batch_norm, F.max_pool2d,
mean, F.linear. torchvision is not a dependency of the test suite, so this restatement is NOT pinned against
torchvision itself (as the U-Net body is not pinned against diffusers): it follows torchvision/models/resnet.py and
transforms/_presets.py by reading.

Two modes of the network:
  fp32          the weights as given, BatchNorm unfolded: what the reference runs.
  fp16 storage  what the device stores: every BatchNorm folded into its conv in fp32 and rounded to fp16 once, the
                pixel values and every layer's output rounded to fp16; all arithmetic still fp32 on the CPU. It
                models the storage format only -- not the fp16 products' accumulation order in the MFMA GEMMs.
The gap between the two on one seed is the yardstick of the GPU parity tests (tests/test_gpu_object_score.py)."""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BN_EPS = 1e-5
STEM_K, STEM_KPAD = 147, 192


# -- front end ----------------------------------------------------------------------------------------------------

def resize_shape(h, w, resize):
    short, long = (h, w) if h <= w else (w, h)
    new_long = int(resize * long / short)
    return (resize, new_long) if h <= w else (new_long, resize)


def crop_offsets(oh, ow, crop):
    """torchvision center_crop: int(round((h - crop) / 2.0)) -- half-even, not (h - crop) // 2."""
    return int(round((oh - crop) / 2.0)), int(round((ow - crop) / 2.0))


def preprocess_u8(img, crop, resize):
    """One [H, W, 3] uint8 image through Pillow's bilinear resize and the centre crop -> [crop, crop, 3] uint8."""
    from PIL import Image
    oh, ow = resize_shape(img.shape[0], img.shape[1], resize)
    out = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
    top, left = crop_offsets(oh, ow, crop)
    return np.ascontiguousarray(out[top:top + crop, left:left + crop])


def quantise(x):
    """[3, H, W] floats in [0, 1] -> [H, W, 3] uint8 (diffusers numpy_to_pil)."""
    q = np.clip(np.rint(np.asarray(x).astype(np.float32) * np.float32(255.0)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(q.transpose(1, 2, 0))


def normalise(u8):
    """[..., 3] uint8 -> float32 ((u8 * (1/255)) - mean) / std."""
    x = u8.astype(np.float32) * np.float32(1.0 / 255.0)
    return (x - np.array(MEAN, np.float32)) / np.array(STD, np.float32)


def pixel_values(u8):
    """[B, S, S, 3] uint8 crops -> the preset's float32 [B, 3, S, S]."""
    return torch.from_numpy(normalise(u8)).permute(0, 3, 1, 2).contiguous()


def stem_rows(u8):
    """[B, S, S, 3] uint8 -> fp16 [B * So^2, STEM_KPAD]: row b So^2 + oy So + ox, column c 49 + ky 7 + kx = the
    normalised pixel (2 oy - 3 + ky, 2 ox - 3 + kx), zero outside the image and in the padding columns."""
    B, S = u8.shape[:2]
    So = (S - 1) // 2 + 1
    pix = np.zeros((B, S + 6, S + 6, 3), np.float16)
    pix[:, 3:3 + S, 3:3 + S] = normalise(u8).astype(np.float16)
    out = np.zeros((B, So, So, STEM_KPAD), np.float16)
    for c in range(3):
        for ky in range(7):
            for kx in range(7):
                out[..., c * 49 + ky * 7 + kx] = pix[:, ky:ky + 2 * So:2, kx:kx + 2 * So:2, c]
    return out.reshape(B * So * So, STEM_KPAD)


# -- network ------------------------------------------------------------------------------------------------------

def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    s = gamma / torch.sqrt(var + eps)
    return w * s.view(-1, 1, 1, 1), beta - mean * s


def to_rows(x):
    """[B, C, H, W] -> NHWC rows [B * H * W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def from_rows(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


class ResNetRef:
    """The restatement over a torchvision-named fp32 state dict. fp16_storage selects the mode (module docstring)."""

    def __init__(self, sd, cfg, fp16_storage=False):
        self.sd = {k: v.float() for k, v in sd.items()}
        self.cfg, self.h = cfg, fp16_storage

    def q(self, x):
        return x.half().float() if self.h else x

    def conv_bn(self, x, conv, bn, stride=1, padding=0, relu=True):
        sd = self.sd
        w = sd[f"{conv}.weight"]
        g, b, m, v = (sd[f"{bn}.{n}"] for n in ("weight", "bias", "running_mean", "running_var"))
        if self.h:
            wf, bf = fold_bn(w, g, b, m, v)
            y = F.conv2d(x, wf.half().float(), bf.half().float(), stride=stride, padding=padding)
        else:
            y = F.batch_norm(F.conv2d(x, w, None, stride=stride, padding=padding), m, v, g, b, False, 0.0, BN_EPS)
        return self.q(F.relu(y) if relu else y)

    def stem_conv(self, pix):
        return self.conv_bn(self.q(pix), "conv1", "bn1", stride=2, padding=3)

    def maxpool(self, x):
        return F.max_pool2d(x, 3, 2, 1)

    def block(self, x, spec):
        p, cin, width, cout, stride, down = spec
        h = self.conv_bn(x, f"{p}.conv1", f"{p}.bn1")
        h = self.conv_bn(h, f"{p}.conv2", f"{p}.bn2", stride=stride, padding=1)
        h = self.conv_bn(h, f"{p}.conv3", f"{p}.bn3", relu=False)
        idt = self.conv_bn(x, f"{p}.downsample.0", f"{p}.downsample.1", stride=stride, relu=False) if down else x
        return self.q(F.relu(h + idt))

    def head(self, x):
        w, b = self.sd["fc.weight"], self.sd["fc.bias"]
        if self.h:
            w, b = w.half().float(), b.half().float()
        return self.q(F.linear(self.q(x.mean((2, 3))), w, b))

    def forward(self, pix):
        with torch.no_grad():
            x = self.maxpool(self.stem_conv(pix))
            for spec in self.cfg.blocks():
                x = self.block(x, spec)
            return self.head(x)


# -- scoring ------------------------------------------------------------------------------------------------------

def topk_stable(logits, k):
    """Top-k ids of float rows by a stable sort of (-logit, id); NaN first (torch.topk's ranking)."""
    out = []
    for row in np.asarray(logits, np.float64):
        nan = np.isnan(row)
        key = np.where(nan, 0.0, -row) + 0.0  # -0 == +0
        out.append(np.lexsort((np.arange(len(row)), key, ~nan))[:k])  # last key first: NaN, then -logit, then id
    return np.array(out, np.int32)


def hits(topk, categories, labels):
    """object_erase.py:253-284 per image: 1 if a word of one of the top-k names is among the label's words."""
    out = []
    for ids, label in zip(topk, labels):
        words = label.strip().split(" ")
        out.append(int(any(w in words for c in ids for w in categories[int(c)].split(" "))))
    return np.array(out, np.int32)


# -- shared cases ---------------------------------------------------------------------------------------------------

def smooth_images(seed, sizes):
    """Smooth high-contrast colour fields, fp16 [3, H, W] in [0, 1], one per (H, W) of `sizes`."""
    g = torch.Generator().manual_seed(int(seed))
    out = []
    for hw in sizes:
        low = torch.rand(1, 3, 4, 4, generator=g)
        im = F.interpolate(low, size=hw, mode="bilinear")[0]
        out.append(((im - 0.5) * 3 + 0.5).clamp(0, 1).half())
    return out


def crops(images, crop, resize):
    """The preset's uint8 crops [n, crop, crop, 3] of fp16 [3, H, W] images, through Pillow."""
    return np.stack([preprocess_u8(quantise(i.float().numpy()), crop, resize) for i in images])


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


# The top-5 / acc case: tiny() at crop 64 (resize 72), 12 images of mixed sizes, 40 synthetic category names. Seeds
# searched on the CPU (tests/test_object_score_host.py asserts what the search found): with delta = 4 x the largest
# |logit difference| between the two CPU modes, at most 10 % of the images have a reference 5th-to-6th logit gap
# within delta.
TOPK_CROP, TOPK_RESIZE = 64, 72
TOPK_SIZES = ((80, 80), (72, 96), (96, 64), (64, 64)) * 3
# Of seeds 0..29, 12 keep every image and 14 exclude one (8.3 %); the three below: no exclusion with the smallest kept
# gap at 3.6 x and 5 x delta (seeds 4, 12), and one exclusion (seed 1), so that the exclusion path runs too.
TOPK_SEEDS = (4, 12, 1)
TOPK_MAX_EXCLUDED = 0.10


def categories40():
    """40 two-word names: the first word is shared by five classes, the second is the class's own."""
    kinds = ("cassette", "English", "garbage", "gas", "golf", "chain", "French", "tench")
    return [f"{kinds[c % 8]} thing{c}" for c in range(40)]


def topk_labels(n):
    """Lower-cased labels as the reference's prompt CSV carries them: multi-word, one that can only match through a
    capitalised category word (and so never does), one that matches nothing."""
    base = ("cassette player", "english springer", "garbage truck", "thing7", "golf ball thing3", "parachute")
    return [base[i % len(base)] for i in range(n)]


def topk_case(seed):
    """{'cfg', 'sd', 'images', 'u8', 'ref32', 'ref16', 'delta', 'gap', 'keep'}: the two CPU modes' logits on one seed,
    delta, each image's reference 5th-to-6th gap and which images the comparison keeps."""
    from sdmoe.resnet import ResNetConfig, make_resnet_state_dict
    cfg = ResNetConfig.tiny()
    sd = make_resnet_state_dict(cfg, seed)
    images = smooth_images(100 + seed, TOPK_SIZES)
    u8 = crops(images, TOPK_CROP, TOPK_RESIZE)
    pix = pixel_values(u8)
    ref32 = ResNetRef(sd, cfg).forward(pix)
    ref16 = ResNetRef(sd, cfg, fp16_storage=True).forward(pix)
    delta = 4.0 * (ref32 - ref16).abs().max().item()
    srt = ref32.sort(1, descending=True).values
    gap = (srt[:, 4] - srt[:, 5]).numpy()
    return {"cfg": cfg, "sd": sd, "images": images, "u8": u8, "ref32": ref32, "ref16": ref16, "delta": delta,
            "gap": gap, "keep": gap > delta}
