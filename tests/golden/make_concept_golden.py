"""Golden vectors for the concept router, made by running the REFERENCE's own concept checkers.

Runs only in the build container (the reference tree is not present on the GPU box). It imports the reference's
benchmarks/concept_checkers.py with a stub `transformers` whose CLIPTokenizer / CLIPTextModel return hidden states
that are a deterministic function of the prompt string (tests/concept_ref.py: stub_hidden, fp16-representable fp32
[1, 77, 64]), builds its ArtStyleChecker and NudityChecker, and records decide() / similarity() on the prompts below.
The NudityChecker reads its anchor prompts from a file relative to the working directory and draws 100 of them with
np.random.choice: the maker runs in a scratch directory holding ANCHOR_LINES under that name, seeds NumPy, and records
the draw. Only data is written (hidden states, banks, sims, decisions); nothing of the reference's source is copied.

The reference computes in fp32, the port in float64 on the same inputs: the a-priori gap of a cosine is
(L + 2 D) 2^-24 = 1.2e-5. The maker asserts that EVERY comparison the reference makes -- arg-max vs the other concepts,
max vs no-concept, max vs the threshold, anchors vs no-concept -- has a margin of at least 10x that for every recorded
prompt, so no decision of the fixture hangs on rounding.

Fixture kinds: concept_bank, concept_prompts (every fixture of this directory names its kind and the dtype of its
inputs). index.json is left alone.
Writes tests/golden/concept_bank.npz (bank prompts, their hidden states, the reference's bank features) and
tests/golden/concept_prompts.npz (test prompts, hidden states, sims, decisions, expected removal lists).
Usage: python tests/golden/make_concept_golden.py
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import concept_ref as C  # noqa: E402

REF = os.environ.get("SDMOE_REFERENCE", "/root/reference")

ART = ["Van Gogh", "Monet", "Pablo Picasso"]
NUDITY = ["naked", "sexy"]
THINGS = ["dog", "house"]
HUMANS = ["person", "woman"]
REMOVER_CONCEPTS = ["naked", "Van Gogh", "Pablo Picasso"]  # 'Monet' is an art concept the remover does not have
ANCHOR_LINES = ["a nude figure lying on a bed\n", "portrait of a topless model at sunset\n",
                "a sensual body in dim light\n", "bare skin and wet hair on the beach\n"]
PROMPTS = [
    "a cat by Van Gogh", "starry night over a village by Van Gogh", "a house by Monet", "water lilies by Monet",
    "a portrait by Pablo Picasso", "a guitar and a bottle by Pablo Picasso", "sunflowers in a vase",
    "a dog in the snow", "a photo of a red car", "a house on a hill", "Van Gogh", "a painting of Monet and a dog",
    "a photo of a naked person", "a sexy woman on the beach", "a naked man by Van Gogh", "a woman reading a book",
    "a person walking a dog", "portrait of a model at sunset", "wet hair and bare skin", "a nude figure",
    "a photo of a house", "a bottle on a table", "a sexy dog by Pablo Picasso", "",
]


def load_reference():
    strings = []

    class Enc:
        def __init__(self, ids):
            self.input_ids = ids

        def to(self, device):
            return self

    class CLIPTokenizer:
        @classmethod
        def from_pretrained(cls, name):
            return cls()

        def __call__(self, text, return_tensors="pt", padding="max_length"):
            ids = torch.zeros((1, C.L_STUB), dtype=torch.int64)
            strings.append(str(text))
            ids[0, 0] = len(strings) - 1
            return Enc(ids)

    class CLIPTextModel:
        @classmethod
        def from_pretrained(cls, name):
            return cls()

        def to(self, device):
            return self

        def __call__(self, ids):
            return {"last_hidden_state": torch.from_numpy(C.stub_hidden(strings[int(ids[0, 0])]))[None]}

    tr = types.ModuleType("transformers")
    tr.CLIPTokenizer, tr.CLIPTextModel = CLIPTokenizer, CLIPTextModel
    sys.modules["transformers"] = tr
    spec = importlib.util.spec_from_file_location("ref_concept_checkers",
                                                  os.path.join(REF, "benchmarks", "concept_checkers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, strings


def main():
    mod, strings = load_reference()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "modularity", "datasets"))
        anchor_name = "i2p_prompts_seed_0_CompVis_stable-diffusion-v1-4.txt"
        with open(os.path.join(tmp, "modularity", "datasets", anchor_name), "w") as f:
            f.writelines(ANCHOR_LINES)
        os.chdir(tmp)
        try:
            with torch.no_grad():
                art = mod.ArtStyleChecker("cpu", THINGS, HUMANS, concepts_to_remove=ART)
                np.random.seed(0)
                nud = mod.NudityChecker("cpu", HUMANS, THINGS, concepts_to_remove=NUDITY)
        finally:
            os.chdir(cwd)
    np.random.seed(0)
    anchors = [str(s) for s in np.random.choice(ANCHOR_LINES, 100)]
    bank_prompts = sorted(set(strings))

    gap = 10 * C.COS_GAP
    rec = {k: [] for k in ("art_sims", "art_neg", "art_decide", "nud_sims", "nud_neg", "nud_anchor", "nud_decide",
                           "expected")}
    worst = np.inf
    with torch.no_grad():
        for p in PROMPTS:
            sim, tf = art.similarity(p)
            s = np.array([float(sim[c]) for c in ART], dtype=np.float32)
            neg = float(tf @ art.no_concept_embeds.T)
            m = np.sort(s)[::-1]
            margins = [m[0] - m[1], abs(m[0] - neg), abs(m[0] - art.threshold)]
            a_dec = art.decide(p)
            sim, tf = nud.similarity(p)
            s2 = np.array([float(sim[c]) for c in NUDITY], dtype=np.float32)
            neg2 = float(tf @ nud.no_concept_embeds.T)
            anc = float(tf @ nud.anchor_features.T)
            margins += [abs(s2.max() - neg2), abs(anc - neg2)]
            n_dec = nud.decide(p)
            assert min(margins) >= gap, (p, margins)
            worst = min(worst, min(margins))
            expected = []  # benchmarks/unified_editing.py:113-117 with all_concepts_to_remove = REMOVER_CONCEPTS
            if n_dec == "naked" and "naked" in REMOVER_CONCEPTS:
                expected.append("naked")
            if a_dec != "none" and a_dec in REMOVER_CONCEPTS:
                expected.append(a_dec)
            for k, v in zip(rec, (s, neg, a_dec, s2, neg2, anc, n_dec, expected)):
                rec[k].append(v)
            print(f"{p!r:50} art {a_dec:14} {s.round(3)} neg {neg:.3f} | nud {n_dec:6} {s2.round(3)} neg {neg2:.3f} "
                  f"anchor {anc:.3f} -> {expected}")
    print(f"smallest margin of any comparison: {worst:.3e} (required {gap:.3e})")
    # the fixture must show both outcomes of every clause
    assert {"none", "Van Gogh", "Monet", "Pablo Picasso"} <= set(rec["art_decide"])
    assert {"none", "naked"} <= set(rec["nud_decide"])
    anchor_only = [p for p, s2, n, a in zip(PROMPTS, rec["nud_sims"], rec["nud_neg"], rec["nud_anchor"])
                   if s2.max() < n < a]
    assert anchor_only, "no prompt fires through the anchor clause alone"
    assert any(a == "Monet" for a in rec["art_decide"])  # the absent concept is somebody's arg-max

    def hid(ps):
        return np.stack([C.stub_hidden(p) for p in ps]).astype(np.float16)

    np.savez_compressed(
        os.path.join(HERE, "concept_bank.npz"), kind="concept_bank", dtype="float16",
        meta=json.dumps({"art": ART, "nudity": NUDITY, "things": THINGS, "humans": HUMANS, "anchors": anchors,
                         "remover_concepts": REMOVER_CONCEPTS, "threshold": art.threshold,
                         "bank_prompts": bank_prompts}),
        hidden=hid(bank_prompts),
        art_bank=np.stack([art.all_concept_features[c].numpy() for c in ART]),
        art_neg=art.no_concept_embeds.numpy(),
        nud_bank=np.stack([nud.all_concept_features[c].numpy() for c in NUDITY]),
        nud_neg=nud.no_concept_embeds.numpy(), nud_anchor=nud.anchor_features.numpy())
    np.savez_compressed(
        os.path.join(HERE, "concept_prompts.npz"), kind="concept_prompts", dtype="float16",
        meta=json.dumps({"prompts": PROMPTS, "art_decide": rec["art_decide"], "nud_decide": rec["nud_decide"],
                         "expected": rec["expected"], "anchor_only": anchor_only}),
        hidden=hid(PROMPTS), art_sims=np.stack(rec["art_sims"]), art_neg=np.array(rec["art_neg"], dtype=np.float32),
        nud_sims=np.stack(rec["nud_sims"]), nud_neg=np.array(rec["nud_neg"], dtype=np.float32),
        nud_anchor=np.array(rec["nud_anchor"], dtype=np.float32))
    for n in ("concept_bank.npz", "concept_prompts.npz"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
