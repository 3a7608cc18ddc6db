"""CPU restatement of the CLIP scorer's front end and score arithmetic (sdmoe/scoring.py, csrc/clip_image.hip).

Front end: diffusers' numpy_to_pil quantisation, Pillow's 8-bit bicubic resampler (libImaging/Resample.c:
precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc -- horizontal pass, uint8
intermediate, vertical pass), transformers' CLIP resize rule (shortest edge to S, long edge int(S * long / short)),
the centre crop, rescale + normalise, and the patch-embedding GEMM's A operand layout. Scores: the float64
arithmetic of the reference's benchmarks/artist_removal.py:196-207 and art_removal.py:114-125.

Everything here is NumPy on the host; tests/test_clip_score_host.py pins it against Pillow, transformers and torch,
tests/test_gpu_clip_score.py holds the HIP kernels to it bit for bit."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2  # Pillow's 8bpc fixed point: 22 fractional bits
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def quantise(x):
    """[B, 3, H, W] floats in [0, 1] -> [B, H, W, 3] uint8: (images * 255).round().astype('uint8') on float32."""
    x = np.asarray(x).astype(np.float32)
    q = np.clip(np.rint(x * np.float32(255.0)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(q.transpose(0, 2, 3, 1))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """Pillow's per-axis tables: bounds int32 [out, 2] = (xmin, taps), kk int32 [out, ksize] (22-bit fixed point,
    zero past the taps)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = np.array([_bicubic((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(n)], np.float64)
        ww = 0.0
        for v in w:  # Pillow's running sum, not NumPy's pairwise one
            ww += v
        if ww != 0.0:
            w = w / ww
        for x in range(n):
            v = w[x] * (1 << PRECISION_BITS)
            kk[i, x] = int(v - 0.5) if w[x] < 0 else int(v + 0.5)
        bounds[i] = (xmin, n)
    return bounds, kk


def _pass(img, bounds, kk, axis):
    """One 8bpc pass along `axis` of a [H, W, C] uint8 image for the table's outputs."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(bounds),) + src.shape[1:], np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[i, :n].astype(np.int64), src[lo:lo + n], axes=(0, 0))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, out_h, out_w):
    """PIL.Image.resize((out_w, out_h), BICUBIC) of a [H, W, 3] uint8 image."""
    h, w = img.shape[:2]
    bx, kx = coeffs(w, out_w)
    by, ky = coeffs(h, out_h)
    return _pass(_pass(img, bx, kx, 1), by, ky, 0)


def resize_shape(h, w, size):
    """transformers' shortest-edge rule: (out_h, out_w)."""
    short, long = (h, w) if h <= w else (w, h)
    new_long = int(size * long / short)
    return (size, new_long) if h <= w else (new_long, size)


def crop_offsets(out_h, out_w, size):
    return (out_h - size) // 2, (out_w - size) // 2


def preprocess_u8(img, size):
    """Resize (shortest edge -> size) and centre crop of one [H, W, 3] uint8 image -> [size, size, 3] uint8."""
    oh, ow = resize_shape(img.shape[0], img.shape[1], size)
    top, left = crop_offsets(oh, ow, size)
    return resize_u8(img, oh, ow)[top:top + size, left:left + size]


def normalise(u8):
    """[..., 3] uint8 -> float32 ((u8 * (1/255)) - mean) / std, CLIP's image_mean / image_std."""
    x = u8.astype(np.float32) * np.float32(1.0 / 255.0)
    return (x - np.array(CLIP_MEAN, np.float32)) / np.array(CLIP_STD, np.float32)


def padded_k(patch):
    return -(-3 * patch * patch // 64) * 64


def patchify(pix, patch):
    """[B, S, S, 3] float32 pixel values -> the patch GEMM's A operand, fp16 [B * G * G, Kpad]: row b G^2 + py G + px,
    column c p^2 + iy p + ix, zero padding columns."""
    B, S = pix.shape[:2]
    G = S // patch
    a = pix.reshape(B, G, patch, G, patch, 3).transpose(0, 1, 3, 5, 2, 4).reshape(B * G * G, 3 * patch * patch)
    out = np.zeros((B * G * G, padded_k(patch)), np.float16)
    out[:, :a.shape[1]] = a.astype(np.float16)
    return out


def a_operand(imgs_u8, size, patch):
    """List of [H, W, 3] uint8 images -> A operand fp16."""
    return patchify(normalise(np.stack([preprocess_u8(i, size) for i in imgs_u8])), patch)


def cosine(x, y, eps=1e-8):
    """torch.nn.functional.cosine_similarity on float64 upcasts of [n, D] rows."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    nx = np.maximum(np.sqrt((x * x).sum(-1)), eps)
    ny = np.maximum(np.sqrt((y * y).sum(-1)), eps)
    return (x * y).sum(-1) / (nx * ny)


def removal_scores(T, A, R):
    """artist_removal.py:196-207 over n prompts: per-prompt cosines, mean image similarity, share of prompts whose
    text-image cosine dropped (strict >)."""
    so, sr, si = cosine(T, A), cosine(T, R), cosine(A, R)
    n = len(si)
    return {"similarity_orig": so, "similarity_removed": sr, "image_sim": si,
            "average_clipscore": float(si.sum() / n), "average_acc": float((so > sr).sum() / n)}


# -- the fp32 transformers oracle and the end-to-end accuracy cases shared by the host and GPU tests -----------------

ACC_SIZES = ((40, 56), (64, 64), (96, 64))  # image sizes of an accuracy case, cycled: both non-square orientations
ACC_PAIRS = 6
ACC_MARGIN = 4e-2  # |similarity_orig - similarity_removed| of every pair under the fp32 oracle (twice the cosine bar)
# searched over seeds 0..39 on the CPU (3 qualify: 1, 20, 26); minimum margins 0.0457 and 0.0952, oracle accuracies
# 0.5 and 0.667 -- both outcomes of the strict > occur in each case (tests/test_clip_score_host.py asserts the margin)
ACC_SEEDS = (1, 26)


def h16(sd):
    """The weights as the device stores them: rounded to fp16, held in fp32."""
    return {k: v.half().float() for k, v in sd.items()}


def hf_clip_model(text_cfg, vision_cfg, sd):
    """transformers.CLIPModel (fp32, eval) of sdmoe's configs carrying the state dict `sd`."""
    import torch
    from transformers import CLIPConfig, CLIPModel
    t, v = text_cfg, vision_cfg
    cfg = CLIPConfig(
        text_config=dict(vocab_size=t.vocab_size, hidden_size=t.hidden_size, intermediate_size=t.intermediate_size,
                         num_hidden_layers=t.num_hidden_layers, num_attention_heads=t.num_attention_heads,
                         max_position_embeddings=t.max_position_embeddings, hidden_act=t.hidden_act,
                         layer_norm_eps=t.layer_norm_eps, eos_token_id=t.eos_token_id, bos_token_id=t.bos_token_id,
                         pad_token_id=t.pad_token_id, projection_dim=t.projection_dim),
        vision_config=dict(hidden_size=v.hidden_size, intermediate_size=v.intermediate_size,
                           num_hidden_layers=v.num_hidden_layers, num_attention_heads=v.num_attention_heads,
                           image_size=v.image_size, patch_size=v.patch_size, hidden_act=v.hidden_act,
                           layer_norm_eps=v.layer_norm_eps, projection_dim=v.projection_dim),
        projection_dim=v.projection_dim)
    m = CLIPModel(cfg).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert set(missing) <= {"logit_scale"} and not unexpected, (missing, unexpected)
    return m.to(torch.float32)


def hf_image_features(model, pixel_values):
    """get_image_features spelled out (its return type differs between transformers versions)."""
    import torch
    with torch.no_grad():
        return model.visual_projection(model.vision_model(pixel_values=pixel_values).pooler_output)


def hf_text_features(model, input_ids):
    import torch
    with torch.no_grad():
        return model.text_projection(model.text_model(input_ids=input_ids).pooler_output)


def pixel_values(imgs_u8, size):
    """CLIPImageProcessor's pixel_values [n, 3, size, size] float32 of uint8 HWC images, through this restatement."""
    import torch
    pv = np.stack([normalise(preprocess_u8(i, size)) for i in imgs_u8])
    return torch.from_numpy(pv).permute(0, 3, 1, 2).contiguous()


def accuracy_case(seed):
    """One end-to-end scoring case: tiny text / vision configs, their seeded weights, ACC_PAIRS prompts and fp16
    `output_type="pt"` image pairs [3, H, W] of ACC_SIZES (smooth high-contrast colour fields)."""
    import torch
    from sdmoe.clip import CLIPTextConfig, CLIPVisionConfig, make_clip_state_dict, make_clip_vision_state_dict
    tc = CLIPTextConfig.tiny(128, 2, 2, projection_dim=64)
    vc = CLIPVisionConfig.tiny(128, 2, 2, patch=4, image=28, projection_dim=64)
    sd = {**make_clip_state_dict(tc, seed), **make_clip_vision_state_dict(vc, seed)}
    g = torch.Generator().manual_seed(int(seed))

    def images():
        out = []
        for i in range(ACC_PAIRS):
            low = torch.rand(1, 3, 3, 3, generator=g)
            im = torch.nn.functional.interpolate(low, size=ACC_SIZES[i % len(ACC_SIZES)], mode="bilinear")[0]
            out.append(((im - 0.5) * 3 + 0.5).clamp(0, 1).half())
        return out

    prompts = [f"a painting of subject {i} by artist {7 * i}" for i in range(ACC_PAIRS)]
    return {"text_cfg": tc, "vision_cfg": vc, "sd": sd, "prompts": prompts, "orig": images(), "removed": images()}


def accuracy_oracle(case):
    """The reference's route for a case: quantise, Pillow-exact preprocessing, fp32 transformers CLIPModel on the
    fp16-rounded weights, artist_removal.py's arithmetic in float64."""
    from sdmoe.clip import SyntheticCLIPTokenizer
    m = hf_clip_model(case["text_cfg"], case["vision_cfg"], h16(case["sd"]))
    size = case["vision_cfg"].image_size

    def feats(imgs):
        u8 = [quantise(i[None].numpy())[0] for i in imgs]
        return hf_image_features(m, pixel_values(u8, size)).double().numpy()

    ids = SyntheticCLIPTokenizer(pad_token_id=case["text_cfg"].pad_token_id)(case["prompts"]).input_ids
    t = hf_text_features(m, ids).double().numpy()
    return removal_scores(t, feats(case["orig"]), feats(case["removed"]))
