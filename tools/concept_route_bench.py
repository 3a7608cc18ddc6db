"""Times the concept routing of a batch three ways on the same device rows, in one process, alternating round by round:

  route    ops.concept_route on fp16 rows [B * 77, 768] (an art group of 3 concepts plus the nudity group): one launch,
           select words and sims stay on the device
  torch    a torch restatement of the reference's per-prompt route (benchmarks/concept_checkers.py:66-81, 119-133,
           170-184) on the same rows: per prompt and per checker fp32 mean over the 77 rows, norm, one matmul per
           concept, Python comparisons on device scalars (each a device -> host sync), a concept name on the host
  encode   one text_encoder.encode of the B prompts (random-init ViT-L/14 text tower): the pass the conditioning-row
           path saves per checker, since the pipeline's encode_prompt has already made these rows

Device events around `--inner` back-to-back calls for `route`, a host clock around synchronised work for the other two.
Warm-up rounds first; medians with min / max. Recorded, not asserted.

usage: python tools/concept_route_bench.py [--B 8] [--rounds 9] [--out FILE]
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
from sdmoe.clip import CLIPTextConfig, CLIPTextModel, SyntheticCLIPTokenizer, make_clip_state_dict  # noqa: E402
from sdmoe.concepts import ConceptRouter  # noqa: E402

ART = ["Van Gogh", "Monet", "Pablo Picasso"]
THINGS = ["dog", "house", "tree", "car"]
HUMANS = ["person", "woman", "man", "child"]
ANCHORS = [f"anchor prompt number {i} with a figure" for i in range(16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("concept_route_bench needs a GPU")
    B = a.B
    tc = CLIPTextConfig.sd14()
    enc = CLIPTextModel.from_state_dict(make_clip_state_dict(tc, 0), tc, "cuda")
    tok = SyntheticCLIPTokenizer(pad_token_id=tc.pad_token_id)
    router = ConceptRouter(enc, tok, "cuda")
    router.add_art_styles(ART, THINGS, HUMANS)
    router.add_nudity(("naked", "sexy"), HUMANS, THINGS, ANCHORS)
    router.bind(["naked"] + ART)
    prompts = [f"a painting of subject {i} by {ART[i % 3]}" for i in range(B)]
    rows = router.encode(prompts)
    L, D = rows.shape[0] // B, rows.shape[1]
    bank32 = router.bank.float()
    row_bit, groups = router.row_bit, router.groups
    torch.cuda.synchronize()

    def route():
        return router.select_from_hidden(rows, B)

    def torch_route():
        words = []
        for b in range(B):  # one prompt per call, one pass per checker, as the reference
            word = 0
            for row0, row1, neg, anchor, thr in groups:
                f = rows[b * L:(b + 1) * L].float().mean(dim=0, keepdim=True)
                f = f / f.norm(dim=-1, keepdim=True)
                sim = {r: (f @ bank32[r].T).view(-1) for r in range(row0, row1)}
                m = max(sim.values())
                best = max(sim, key=sim.get)
                no = f @ bank32[neg].T
                fire = bool(m > no) and bool(m > thr)
                if not fire and anchor >= 0:
                    fire = bool((f @ bank32[anchor].T) > no)
                if fire and row_bit[best] >= 0:
                    word |= 1 << row_bit[best]
            words.append(word)
        return words

    def encode():
        return router.encode(prompts)

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {"route": [], "torch": [], "encode": []}
    res = {}
    for r in range(a.warmup + a.rounds):
        ev0.record()
        for _ in range(a.inner):
            res["route"] = route()
        ev1.record()
        torch.cuda.synchronize()
        dts = {"route": ev0.elapsed_time(ev1) / a.inner * 1e-3}
        for name, fn in (("torch", torch_route), ("encode", encode)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name] = fn()
            torch.cuda.synchronize()
            dts[name] = time.perf_counter() - t0
        if r >= a.warmup:
            for k, v in dts.items():
                times[k].append(v)
    dev_words = [int(w) & 0xFFFFFFFF for w in res["route"].cpu().tolist()]
    lines = [f"# concept routing, B = {B} prompts, L = {L}, D = {D}, R = {router.bank.shape[0]} bank rows, "
             f"{len(groups)} groups (art x{len(ART)} + nudity), {torch.cuda.get_device_name(0)}, one process, "
             f"alternated, warm-up first"]
    what = {"route": f"ops.concept_route, one launch (device events, {a.inner} back-to-back calls)",
            "torch": "torch restatement of the reference's per-prompt, per-checker route on the same rows (host clock)",
            "encode": f"text_encoder.encode of the {B} prompts, ViT-L/14 text tower, random init (host clock)"}
    for name in ("route", "torch", "encode"):
        v = [x * 1e6 for x in times[name]]
        lines.append(f"{name:7s} {statistics.median(v):12.1f} us (min {min(v):.1f}, max {max(v):.1f}, {len(v)} rounds)"
                     f"   {what[name]}")
    lines.append(f"torch/route {statistics.median(times['torch']) / statistics.median(times['route']):.1f}")
    lines.append(f"select words: route {dev_words} torch {res['torch']} equal {dev_words == res['torch']}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
