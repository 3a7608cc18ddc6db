"""torchvision's ResNet (v1.5 bottleneck: the stride sits on the 3x3 conv) on the HIP kernels, for the object-erasure
scorer (sdmoe.scoring.ObjectScorer; the reference's benchmarks/object_erase.py:247-302 runs torchvision.models.resnet50
in fp32 on the host, one image per call).

Every BatchNorm is folded into its conv on the host in fp32 and the result rounded to fp16 once; activations are NHWC
fp16 rows [images * H * W, C]. The forward pass uses only existing GEMM / conv kernels plus csrc/imagenet.hip:

    stem      ops.stem_rows (normalise + im2col of the 7x7 / stride 2 conv) -> ops.linear(ReLU) -> ops.maxpool3x3s2
    block     ops.linear(ReLU) [1x1] -> ops.conv3x3(stride, ReLU) -> ops.linear [1x1] -> ops.add_relu(identity)
    block 0   of each stage (projection shortcut): the 3x3 conv writes h into the left columns of one [rows, width +
              Cin] buffer, ops.gather_rows puts the (stride-subsampled) block input x_s into the right columns, and
              conv3 + downsample + add + ReLU are ONE ops.linear(ReLU) with the weights [W3 | Wd] concatenated along K
              and the two folded biases summed in fp32: neither branch output is written or re-read.
    head      ops.avgpool_rows -> ops.linear (fc)

There is no host path: the model lives on a GPU device.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import ops

BN_EPS = 1e-5  # torchvision's BatchNorm2d default


@dataclass
class ResNetConfig:
    layers: tuple = (3, 4, 6, 3)
    widths: tuple = (64, 128, 256, 512)
    expansion: int = 4
    num_classes: int = 1000
    stem_width: int = 64

    def __post_init__(self):
        self.layers, self.widths = tuple(self.layers), tuple(self.widths)
        if len(self.layers) != 4 or len(self.widths) != 4 or min(self.layers) < 1:
            raise ValueError(f"ResNetConfig: four stages of >= 1 block each, got layers={self.layers} "
                             f"widths={self.widths}")
        if self.stem_width % 64 or any(w % 64 for w in self.widths):
            raise ValueError("ResNetConfig: widths must be multiples of 64 (the conv kernel's channel slice)")
        if self.expansion < 1 or self.num_classes % 8 or self.num_classes <= 0:
            raise ValueError("ResNetConfig: expansion >= 1 and num_classes a positive multiple of 8 (the GEMM's N)")

    @staticmethod
    def resnet50():
        return ResNetConfig()

    @staticmethod
    def tiny():
        return ResNetConfig(layers=(1, 1, 1, 1), num_classes=40)

    @property
    def features(self) -> int:
        return self.widths[3] * self.expansion

    def check_size(self, size: int) -> None:
        """The stem, the max pool and stages 2-4 each halve the extent; a size at which one of them would see an odd
        extent is refused (torchvision would round up there; no test covers it)."""
        if size <= 0 or size % 32:
            raise ValueError(f"image size {size}: a stride-2 stage would see an odd extent (need a multiple of 32)")

    def blocks(self):
        """[(prefix, Cin, width, Cout, stride, has_downsample)] in forward order."""
        out, cin = [], self.stem_width
        for li, (n, w) in enumerate(zip(self.layers, self.widths)):
            for i in range(n):
                stride = 2 if (i == 0 and li > 0) else 1
                cout = w * self.expansion
                out.append((f"layer{li + 1}.{i}", cin, w, cout, stride, i == 0 and (stride != 1 or cin != cout)))
                cin = cout
        return out


def resnet_param_specs(cfg: ResNetConfig):
    """[(torchvision key, shape)] of every tensor ResNet.from_state_dict reads."""
    def bn(p, c):
        return [(f"{p}.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var")]

    s = [("conv1.weight", (cfg.stem_width, 3, 7, 7))] + bn("bn1", cfg.stem_width)
    for p, cin, w, cout, stride, down in cfg.blocks():
        s += [(f"{p}.conv1.weight", (w, cin, 1, 1))] + bn(f"{p}.bn1", w)
        s += [(f"{p}.conv2.weight", (w, w, 3, 3))] + bn(f"{p}.bn2", w)
        s += [(f"{p}.conv3.weight", (cout, w, 1, 1))] + bn(f"{p}.bn3", cout)
        if down:
            s += [(f"{p}.downsample.0.weight", (cout, cin, 1, 1))] + bn(f"{p}.downsample.1", cout)
    return s + [("fc.weight", (cfg.num_classes, cfg.features)), ("fc.bias", (cfg.num_classes,))]


def make_resnet_state_dict(cfg: ResNetConfig, seed: int = 0):
    """Synthetic fp32 weights under torchvision's names (no checkpoint ships with the package): He-normal convs
    (std sqrt(2 / fan_in)), BatchNorm gamma 0.5 on bn3 and the downsample BN and 1 elsewhere (x a jitter of 5 %),
    beta and running_mean ~ N(0, 0.1), running_var ~ U(0.5, 1.5), fc as nn.Linear initialises it. Activations stay
    far inside fp16's range at every stage (largest |activation| of fp32 ResNet-50 at 224 on seed 0: 32)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, shape in resnet_param_specs(cfg):
        if len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            sd[name] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif name.startswith("fc."):
            bound = cfg.features ** -0.5
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif name.endswith("running_var"):
            sd[name] = torch.rand(shape, generator=g) + 0.5
        elif name.endswith(".weight"):
            base = 0.5 if (".bn3." in name or ".downsample.1." in name) else 1.0
            sd[name] = base * (1.0 + 0.05 * torch.randn(shape, generator=g))
        else:  # BatchNorm bias, running_mean
            sd[name] = 0.1 * torch.randn(shape, generator=g)
    return sd


def fold_bn(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """Eval-mode BatchNorm folded into the conv in front of it, in fp32: w' = w * gamma / sqrt(var + eps) per output
    channel, b' = beta - mean * gamma / sqrt(var + eps)."""
    s = gamma.float() / torch.sqrt(var.float() + eps)
    return w.float() * s.view(-1, *([1] * (w.dim() - 1))), beta.float() - mean.float() * s


def prepare_weights(sd, cfg: ResNetConfig):
    """Host side of ResNet.from_state_dict: {name: fp16 tensor in the kernels' layouts}. A missing key raises KeyError,
    a wrong shape ValueError.
      stem.w [64, STEM_KPAD] (columns c 49 + ky 7 + kx, zero padding), <block>.w1 [width, Cin], <block>.w2 in
      ops.conv_weight_from_torch's layout, <block>.w3 [Cout, width] or, with a projection shortcut, [Cout, width + Cin]
      = [W3 | Wd] with bias b3 + bd (summed in fp32), fc.w [classes, features]; every *.b its folded bias."""
    for name, shape in resnet_param_specs(cfg):
        if name not in sd:
            raise KeyError(f"ResNet state dict lacks {name!r}")
        if tuple(sd[name].shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(sd[name].shape)}, expected {tuple(shape)}")

    def folded(conv, bn):
        return fold_bn(sd[f"{conv}.weight"], *(sd[f"{bn}.{n}"] for n in ("weight", "bias", "running_mean",
                                                                         "running_var")))

    out = {}
    w, b = folded("conv1", "bn1")
    stem = torch.zeros((cfg.stem_width, ops.STEM_KPAD), dtype=torch.float32)
    stem[:, :ops.STEM_K] = w.reshape(cfg.stem_width, ops.STEM_K)
    out["stem.w"], out["stem.b"] = stem.half(), b.half()
    for p, cin, width, cout, stride, down in cfg.blocks():
        w1, b1 = folded(f"{p}.conv1", f"{p}.bn1")
        w2, b2 = folded(f"{p}.conv2", f"{p}.bn2")
        w3, b3 = folded(f"{p}.conv3", f"{p}.bn3")
        out[f"{p}.w1"], out[f"{p}.b1"] = w1.reshape(width, cin).half().contiguous(), b1.half()
        out[f"{p}.w2"], out[f"{p}.b2"] = ops.conv_weight_from_torch(w2.half()), b2.half()
        w3 = w3.reshape(cout, width)
        if down:
            wd, bd = folded(f"{p}.downsample.0", f"{p}.downsample.1")
            w3, b3 = torch.cat([w3, wd.reshape(cout, cin)], 1), b3 + bd
        out[f"{p}.w3"], out[f"{p}.b3"] = w3.half().contiguous(), b3.half()
    out["fc.w"], out["fc.b"] = sd["fc.weight"].float().half().contiguous(), sd["fc.bias"].float().half()
    return out


class Bottleneck:
    """One torchvision Bottleneck on folded weights. run(x, nimg, H, W) -> (y, OH, OW)."""

    def __init__(self, name, cin, width, cout, stride, down, wts, device):
        self.name, self.cin, self.width, self.cout, self.stride, self.down = name, cin, width, cout, stride, down
        for n in ("w1", "b1", "w2", "b2", "w3", "b3"):
            setattr(self, n, wts[f"{name}.{n}"].to(device))
        self._idx = {}

    def _shortcut_rows(self, nimg, H, W, device):
        """Row indices of the block input that the 1x1 / stride-s shortcut conv reads, int32 [nimg * OH * OW]."""
        key = (nimg, H, W)
        idx = self._idx.get(key)
        if idx is None:
            s = self.stride
            ys, xs = torch.arange(0, H, s), torch.arange(0, W, s)
            base = (torch.arange(nimg) * (H * W)).view(-1, 1, 1)
            idx = (base + ys.view(1, -1, 1) * W + xs.view(1, 1, -1)).reshape(-1).to(torch.int32)
            idx = self._idx[key] = idx.to(device)
        return idx

    def run(self, x, nimg, H, W):
        s = self.stride
        OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
        h = ops.linear(x, self.w1, self.b1, act=ops.ACT_RELU)
        if not self.down:
            h = ops.conv3x3(h, nimg, H, W, self.w2, self.b2, stride=s, act=ops.ACT_RELU)
            y = ops.linear(h, self.w3, self.b3)
            return ops.add_relu(y, x, out=y), OH, OW
        cat = torch.empty((nimg * OH * OW, self.width + self.cin), dtype=torch.float16, device=x.device)
        ops.conv3x3(h, nimg, H, W, self.w2, self.b2, stride=s, act=ops.ACT_RELU, out=cat[:, :self.width])
        ops.gather_rows(x, self._shortcut_rows(nimg, H, W, x.device), out=cat[:, self.width:])
        return ops.linear(cat, self.w3, self.b3, act=ops.ACT_RELU), OH, OW


class ResNet:
    """ResNet on the device. forward(u8) takes the cropped uint8 pixels [B, S, S, 3] (ObjectScorer.preprocess_u8) and
    returns fp16 logits [B, num_classes]; stem / blocks / head run the same pass one stage at a time."""

    def __init__(self, cfg: ResNetConfig, wts, device):
        self.config, self.device = cfg, torch.device(device)
        if self.device.type != "cuda":
            raise ops._lib.SdmoeError("ResNet: the model needs a GPU device; sdmoe has no CPU path")
        self.stem_w, self.stem_b = wts["stem.w"].to(device), wts["stem.b"].to(device)
        self.fc_w, self.fc_b = wts["fc.w"].to(device), wts["fc.b"].to(device)
        self.blocks = [Bottleneck(*spec, wts, device) for spec in cfg.blocks()]

    @classmethod
    def from_state_dict(cls, sd, cfg: ResNetConfig, device="cuda"):
        return cls(cfg, prepare_weights(sd, cfg), device)

    def stem_conv(self, u8):
        """conv1 + bn1 + relu: [B, S, S, 3] uint8 -> ([B * So^2, 64], So)."""
        self.config.check_size(u8.shape[1])
        So = (u8.shape[1] - 1) // 2 + 1
        return ops.linear(ops.stem_rows(u8), self.stem_w, self.stem_b, act=ops.ACT_RELU), So

    def stem(self, u8):
        """conv1 + bn1 + relu + maxpool -> (x, H, W)."""
        x, So = self.stem_conv(u8)
        return ops.maxpool3x3s2(x, u8.shape[0], So, So), (So - 1) // 2 + 1, (So - 1) // 2 + 1

    def head(self, x, nimg, HW):
        """avgpool + fc -> logits [nimg, num_classes]."""
        return ops.linear(ops.avgpool_rows(x, nimg, HW), self.fc_w, self.fc_b)

    def forward(self, u8):
        nimg = u8.shape[0]
        x, H, W = self.stem(u8)
        for blk in self.blocks:
            x, H, W = blk.run(x, nimg, H, W)
        return self.head(x, nimg, H * W)

    __call__ = forward
