"""Shapes the U-Net's FeedForward down projections issue (test helper, no GPU).

A Transformer-block FFN at level i of a U-Net with latent side S runs its down projection (`ff.net.2`, reference
`LoRACompatibleLinear` hooked by remove_wanda_neurons_fast.py:107-112; fused keep-masked form in sdmoe/unet.py
FeedForward.run) as an M x K x N product with M = U-Net batch x (S / 2^i)^2 tokens, K = 4C, N = C. The U-Net batch
is 2 x prompts per call (CFG)."""
from sdmoe.config import UNetConfig

PROMPTS_PER_CALL = (1, 2, 8, 16)  # the reference's one-prompt call (base_receiver.py:73) .. 16 prompts per GPU


def _level(name, nblk):
    parts = name.split(".")
    if parts[0] == "mid_block":
        return nblk - 1
    i = int(parts[1])
    return i if parts[0] == "down_blocks" else nblk - 1 - i


def down_projection_shapes(model="sd14", prompts=PROMPTS_PER_CALL):
    """Sorted distinct (M, K, N) of the FFN down projections of `model` ('sd14' 512^2 or 'sdxl' 1024^2)."""
    cfg = UNetConfig.sd14() if model == "sd14" else UNetConfig.sdxl()
    nblk = len(cfg.block_out_channels)
    out = set()
    for name, C in cfg.geglu_layers():
        side = cfg.sample_size >> _level(name, nblk)
        for b in prompts:
            out.add((2 * b * side * side, 4 * C, C))
    return sorted(out)


def geglu_projection_shapes(model="sd14", prompts=PROMPTS_PER_CALL):
    """Sorted distinct (M, F, K) of the routed GEGLU projections (`ff.net.0`: M tokens x 2F outputs x K, F = 4C
    neurons, K = C): the same triples as the down projection that follows, read the other way round."""
    return down_projection_shapes(model, prompts)


def conv3x3_shapes(model="sd14", prompts=PROMPTS_PER_CALL):
    """Sorted distinct 3x3 convs of `model` as (nimg, H, Cin, Cin2, Cout, stride, upsample, residual), H = W, in the
    form sdmoe/unet.py issues them: conv_in (4 -> 64 padded input channels), every ResnetBlock2D's conv1 and conv2
    (conv2 with the 1x1 shortcut of a channel-changing block folded in as Cin2 extra channels, else with the block
    input as residual), the stride-2 downsamplers, the nearest-2x upsample convs and conv_out (4 -> 8 padded outputs).
    Block wiring as diffusers' UNet2DConditionModel: an up block's resnet takes the previous output plus one skip."""
    cfg = UNetConfig.sd14() if model == "sd14" else UNetConfig.sdxl()
    ch, L = cfg.block_out_channels, cfg.layers_per_block
    nblk = len(ch)
    convs = [(cfg.sample_size, 64, 0, ch[0], 1, 0, 0), (cfg.sample_size, ch[0], 0, 8, 1, 0, 0)]  # conv_in, conv_out

    def resnet(side, cin, cout):
        convs.append((side, cin, 0, cout, 1, 0, 0))
        convs.append((side, cout, 0 if cin == cout else cin, cout, 1, 0, int(cin == cout)))

    for i, c in enumerate(ch):
        side = cfg.sample_size >> i
        for j in range(L):
            resnet(side, ch[max(i - 1, 0)] if j == 0 else c, c)
        if i < nblk - 1:
            convs.append((side, c, 0, c, 2, 0, 0))
    for _ in range(2):
        resnet(cfg.sample_size >> (nblk - 1), ch[-1], ch[-1])
    rev = ch[::-1]
    for i, c in enumerate(rev):
        side = cfg.sample_size >> (nblk - 1 - i)
        for j in range(L + 1):
            skip = rev[min(i + 1, nblk - 1)] if j == L else c
            resnet(side, (rev[max(i - 1, 0)] if j == 0 else c) + skip, c)
        if i < nblk - 1:
            convs.append((side, c, 0, c, 1, 1, 0))
    return sorted({(2 * b,) + c for b in prompts for c in convs})
