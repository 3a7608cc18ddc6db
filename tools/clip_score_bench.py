"""Times the removal-quality scores two ways on the same device images, in one process, alternating round by round:

  device   sdmoe.scoring.ClipScorer.score_removal on n pairs of fp16 `output_type="pt"` images [n, 3, H, W] with a
           random-init ViT-B/32 CLIPModel: quantise + Pillow-exact resample + patchify, both towers, sdmoe_clip_scores,
           one copy of 3 n + 3 doubles
  host     the reference's route (benchmarks/artist_removal.py:173-207) on the same images: device -> host copy,
           diffusers' numpy_to_pil, CLIPImageProcessorPil, fp32 transformers CLIPModel on the CPU one image per call
           (the PNG save / reload is left out: it would only add to the host time)

and the device front end alone (quantise + resample_h + resample_v for the 2 n images) from device events, against the
bytes it must move by its shapes: fp16 planes read, uint8 NHWC written and read, the uint8 intermediate written and
read, the fp16 A operand written.

Each route timing is a host clock around work that ends synchronised. Warm-up rounds first; medians with min / max.

usage: python tools/clip_score_bench.py [--n 8] [--H 512] [--W 512] [--rounds 7] [--host-rounds 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "diffusion-models-moe_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from sdmoe import ops  # noqa: E402
from sdmoe.clip import (CLIPModel, CLIPTextConfig, CLIPVisionConfig, SyntheticCLIPTokenizer,  # noqa: E402
                        make_clip_state_dict, make_clip_vision_state_dict)
from sdmoe.scoring import ClipScorer  # noqa: E402


def hf_model(tc, vc, sd):
    from transformers import CLIPConfig
    from transformers import CLIPModel as HFCLIPModel
    cfg = CLIPConfig(
        text_config=dict(vocab_size=tc.vocab_size, hidden_size=tc.hidden_size, intermediate_size=tc.intermediate_size,
                         num_hidden_layers=tc.num_hidden_layers, num_attention_heads=tc.num_attention_heads,
                         hidden_act=tc.hidden_act, eos_token_id=tc.eos_token_id, bos_token_id=tc.bos_token_id,
                         pad_token_id=tc.pad_token_id, projection_dim=tc.projection_dim),
        vision_config=dict(hidden_size=vc.hidden_size, intermediate_size=vc.intermediate_size,
                           num_hidden_layers=vc.num_hidden_layers, num_attention_heads=vc.num_attention_heads,
                           image_size=vc.image_size, patch_size=vc.patch_size, hidden_act=vc.hidden_act,
                           projection_dim=vc.projection_dim),
        projection_dim=vc.projection_dim)
    m = HFCLIPModel(cfg).eval()
    m.load_state_dict(sd, strict=False)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8, help="prompts; 2 n images are scored")
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--W", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_score_bench needs a GPU")
    from PIL import Image
    from transformers import CLIPImageProcessorPil
    n, H, W = a.n, a.H, a.W
    tc, vc = CLIPTextConfig.vit_b32(), CLIPVisionConfig.vit_b32()
    sd = {**make_clip_state_dict(tc, 0), **make_clip_vision_state_dict(vc, 0)}
    tok = SyntheticCLIPTokenizer(pad_token_id=tc.pad_token_id)
    scorer = ClipScorer(CLIPModel.from_state_dict(sd, tc, vc, "cuda"), tok, size=224)
    hf = hf_model(tc, vc, {k: v.half().float() for k, v in sd.items()})
    proc = CLIPImageProcessorPil()
    g = torch.Generator().manual_seed(0)
    low = torch.rand(2 * n, 3, 16, 16, generator=g)
    imgs = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic").clamp(0, 1).half().cuda()
    orig, removed = imgs[:n].contiguous(), imgs[n:].contiguous()
    prompts = [f"a painting of subject {i} by artist {7 * i}" for i in range(n)]
    torch.cuda.synchronize()

    def device_route():
        return scorer.score_removal(prompts, orig, removed)

    def host_route():
        cs = torch.nn.functional.cosine_similarity
        acc, clip = 0, 0.0
        with torch.no_grad():
            for i in range(n):
                pil = []
                for t in (orig[i], removed[i]):
                    x = t.cpu().permute(1, 2, 0).float().numpy()
                    pil.append(Image.fromarray((x * 255).round().astype("uint8")))
                ids = tok([prompts[i]]).input_ids
                tf = hf.text_projection(hf.text_model(input_ids=ids).pooler_output)
                f = [hf.visual_projection(hf.vision_model(
                    pixel_values=proc(images=p, return_tensors="pt")["pixel_values"]).pooler_output) for p in pil]
                so, sr = cs(tf, f[0]), cs(tf, f[1])
                acc += 1 if so > sr else 0
                clip += cs(f[0], f[1]).item()
        return clip / n, acc / n

    times = {"device": [], "host": []}
    res = {}
    for r in range(a.warmup + a.rounds):
        routes = [("device", device_route)]
        if r < 1 + a.host_rounds:
            routes.append(("host", host_route))
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name] = fn()
            dt = time.perf_counter() - t0
            if (name == "device" and r >= a.warmup) or (name == "host" and r >= 1):
                times[name].append(dt)

    # the front end alone: device events around 10 back-to-back passes over the 2 n images
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    G2, kpad = 49, ops.clip_padded_k(32)
    a_op = torch.empty((2 * n * G2, kpad), dtype=torch.float16, device="cuda")
    u8 = torch.empty((2 * n, H, W, 3), dtype=torch.uint8, device="cuda")
    plan = ops.clip_resample_plan(H, W, 224, imgs.device)
    front = []
    for r in range(a.warmup + a.rounds):
        ev0.record()
        for _ in range(10):
            ops.clip_quantise(imgs, out=u8)
            ops.clip_preprocess(u8, 224, 32, a_out=a_op)
        ev1.record()
        torch.cuda.synchronize()
        if r >= a.warmup:
            front.append(ev0.elapsed_time(ev1) / 10 * 1e3)
    B = 2 * n
    nbytes = (B * 3 * H * W * 2 + B * H * W * 3          # quantise: fp16 planes in, uint8 NHWC out
              + B * plan.nrows * W * 3 + B * plan.nrows * 224 * 3   # horizontal: rows read, intermediate written
              + B * plan.nrows * 224 * 3 + a_op.numel() * 2)        # vertical: intermediate read, A operand written
    lines = [f"# removal scores, {n} prompts / {B} images {H}x{W} fp16, ViT-B/32 (random init), "
             f"{torch.cuda.get_device_name(0)}, one process, routes alternated, warm-up first"]
    for name, what in (("device", "ClipScorer.score_removal: front end, both towers, sdmoe_clip_scores, 1 copy"),
                       ("host", "device->host copy, numpy_to_pil, CLIPImageProcessorPil, fp32 CLIPModel on the CPU")):
        v = [x * 1e3 for x in times[name]]
        lines.append(f"{name:6s} {statistics.median(v):10.3f} ms (min {min(v):.3f}, max {max(v):.3f}, {len(v)} rounds)"
                     f"   {what}")
    lines.append(f"host/device {statistics.median(times['host']) / statistics.median(times['device']):.1f}")
    fm = statistics.median(front)
    lines.append(f"front end only (device events, 10 back-to-back passes; 3 launches per pass): {fm:.1f} us per pass "
                 f"(min {min(front):.1f}, max {max(front):.1f}); {nbytes / 1e6:.1f} MB moved per pass from shapes = "
                 f"{nbytes / fm / 1e6:.3f} TB/s")
    d, h = res["device"], res["host"]
    lines.append(f"scores: device average_clipscore {d['average_clipscore']:.6f} average_acc {d['average_acc']:.4f}; "
                 f"host {h[0]:.6f} {h[1]:.4f}; |diff| {abs(d['average_clipscore'] - h[0]):.2e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
