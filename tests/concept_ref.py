"""NumPy float64 restatement of the concept router (sdmoe_text_pool / sdmoe_concept_route), written from their
description in include/sdmoe.h, plus the deterministic stand-in text encoder the concept goldens were made with.

pool / text_pool / route are the reference the device kernels and the golden fixture are compared against; margins()
gives, per prompt, the smallest gap of any comparison the group rule makes, so a test can assert that its inputs decide
nothing by rounding before it asks for equal select words.
"""
import re
import zlib

import numpy as np

L_STUB, D_STUB = 77, 64
COS_GAP = (L_STUB + 2 * D_STUB) * 2.0 ** -24  # a-priori fp32-vs-float64 gap of one cosine of the stub's features


# ---- the restatement -------------------------------------------------------------------------------------------------
def pool(X, nseq):
    """X [nseq * L, D] (any float dtype) -> unit mean features float64 [nseq, D]; an all-zero block gives NaN."""
    X = np.asarray(X, dtype=np.float64)
    p = X.reshape(nseq, -1, X.shape[-1]).mean(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return p / np.sqrt((p * p).sum(axis=1, keepdims=True))


def text_pool(X, nseq, group=1, renorm=False):
    f = pool(X, nseq)
    m = f.reshape(nseq // group, group, -1).sum(axis=1) / group
    if renorm:
        with np.errstate(invalid="ignore", divide="ignore"):
            m = m / np.sqrt((m * m).sum(axis=1, keepdims=True))
    return m


def group_fires(sims, group):
    """(fires, first arg-max row) of one group record on one prompt's sims; anything involving NaN is false."""
    row0, row1, neg, anchor, thr = group
    thr = -np.inf if thr is None else thr
    best, m = row0, sims[row0]
    for r in range(row0 + 1, row1):
        if sims[r] > m:
            best, m = r, sims[r]
    fire = bool(m > sims[neg] and m > thr) or bool(anchor >= 0 and sims[anchor] > sims[neg])
    return fire, best


def route(feats, bank, row_bit, groups, preset=None):
    """(select uint32 [B], sims float64 [B, R]) from unit features [B, D]."""
    sims = np.asarray(feats, dtype=np.float64) @ np.asarray(bank, dtype=np.float64).T
    sel = np.zeros(len(sims), dtype=np.uint32) if preset is None else np.array(preset, dtype=np.uint32)
    for b in range(len(sims)):
        for g in groups:
            fire, best = group_fires(sims[b], g)
            if fire and row_bit[best] >= 0:
                sel[b] |= np.uint32(1 << row_bit[best])
    return sel, sims


def margins(sims, groups):
    """Per prompt, the smallest |gap| of any comparison the rule makes: max vs every other row of the group, max vs the
    no-concept row, max vs a finite threshold, anchor vs the no-concept row. Rows that are bit-identical copies of the
    arg-max row are not counted (the first one wins by rule, not by rounding). NaN sims give inf (nothing compares)."""
    out = np.full(len(sims), np.inf)
    for b, s in enumerate(sims):
        if np.isnan(s).any():
            continue
        for row0, row1, neg, anchor, thr in groups:
            best = row0 + int(np.argmax(s[row0:row1]))
            m = s[best]
            gaps = [abs(m - s[r]) for r in range(row0, row1) if r != best and s[r] != m] + [abs(m - s[neg])]
            if thr is not None and np.isfinite(thr):
                gaps.append(abs(m - thr))
            if anchor >= 0:
                gaps.append(abs(s[anchor] - s[neg]))
            out[b] = min(out[b], min(gaps))
    return out


def names_of(select, concept_names):
    return [[c for i, c in enumerate(concept_names) if (int(w) >> i) & 1] for w in np.asarray(select, dtype=np.uint32)]


# ---- the stand-in text encoder of the goldens ------------------------------------------------------------------------
_STOP = {"a", "an", "of", "by", "the", "photo", "in", "on", "with", "and", "at"}


def stub_hidden(prompt):
    """Hidden states of a prompt string, fp16-representable float32 [77, 64]: one seeded direction per word on every
    row (function words weigh less), plus seeded noise per row."""
    vec = np.zeros(D_STUB)
    for w in re.findall(r"[a-z]+", prompt.lower()):
        d = np.random.default_rng(zlib.crc32(w.encode())).standard_normal(D_STUB)
        vec += (0.25 if w in _STOP else 1.0) * d
    noise = np.random.default_rng(zlib.crc32(("noise:" + prompt).encode())).standard_normal((L_STUB, D_STUB))
    return (vec[None, :] + 0.5 * noise).astype(np.float16).astype(np.float32)


class StubTokenizer:
    """Keeps the prompt strings: input_ids[i, 0] indexes them, the other 76 ids are padding."""

    def __init__(self):
        self.strings = []

    def __call__(self, text, padding="max_length", max_length=None, truncation=True, return_tensors="pt"):
        import torch
        texts = [text] if isinstance(text, str) else list(text)
        ids = torch.zeros((len(texts), L_STUB), dtype=torch.int64)
        for i, t in enumerate(texts):
            self.strings.append(t)
            ids[i, 0] = len(self.strings) - 1
        enc = type("Enc", (), {})()
        enc.input_ids = ids
        enc.to = lambda device: enc
        return enc


class StubTextEncoder:
    """sdmoe.clip.CLIPTextModel's encode() contract on stored hidden states: {"hidden": fp16 [nseq * 77, 64]}."""

    def __init__(self, tokenizer, device, hidden=None):
        self.tokenizer, self.device, self.hidden = tokenizer, device, hidden or {}
        self.calls = 0

    def encode(self, input_ids, **kw):
        import torch
        self.calls += 1
        rows = []
        for i in input_ids[:, 0].tolist():
            s = self.tokenizer.strings[i]
            rows.append(np.asarray(self.hidden[s]) if s in self.hidden else stub_hidden(s))
        x = np.concatenate(rows).astype(np.float16)
        return {"hidden": torch.from_numpy(x).to(self.device)}


# ---- the golden fixture (tests/golden/make_concept_golden.py) ---------------------------------------------------------
def load_golden():
    """The reference checkers' recorded run: {"bank": {...}, "prompts": {...}} with the JSON meta unpacked."""
    import json
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for key in ("bank", "prompts"):
        with np.load(os.path.join(gold, f"concept_{key}.npz"), allow_pickle=False) as z:
            d = {k: z[k] for k in z.files if k not in ("meta", "kind", "dtype")}
            d.update(json.loads(str(z["meta"])))
        out[key] = d
    return out


def golden_bank_prompts(meta):
    """The bank prompts of the two checkers in the router's order, as (art, art negatives, nudity, nudity negatives,
    anchors): the reference's templates, literally."""
    art = [f"a {o} by {c}" for c in meta["art"] for o in meta["things"]]
    art_neg = ['a photo of a' + t for t in meta["humans"]]
    nud = [f"a photo of a {c} {o}" for c in meta["nudity"] for o in meta["humans"]]
    nud_neg = ['a photo of a' + t for t in meta["things"]]
    return art, art_neg, nud, nud_neg, list(meta["anchors"])


def golden_router_tables(meta):
    """(row labels, group records) of a router holding the art checker then the nudity checker."""
    na, nn = len(meta["art"]), len(meta["nudity"])
    labels = list(meta["art"]) + [None] + ["naked"] * nn + [None, None]
    groups = [(0, na, na, -1, float(meta["threshold"])), (na + 1, na + 1 + nn, na + 1 + nn, na + 2 + nn, None)]
    return labels, groups


def golden_bank_restated(bank):
    """The router's bank [R, D] in float64 from the recorded hidden states of the bank prompts."""
    hidden = dict(zip(bank["bank_prompts"], bank["hidden"]))

    def rows(ps):
        return np.concatenate([hidden[p] for p in ps])
    art, art_neg, nud, nud_neg, anchors = golden_bank_prompts(bank)
    return np.concatenate([
        text_pool(rows(art), len(art), group=len(bank["things"])),
        text_pool(rows(art_neg), len(art_neg), group=len(art_neg), renorm=True),
        text_pool(rows(nud), len(nud), group=len(bank["humans"])),
        text_pool(rows(nud_neg), len(nud_neg), group=len(nud_neg), renorm=True),
        text_pool(rows(anchors), len(anchors), group=len(anchors))])


def golden_reference_rows(bank, prompts):
    """The reference's own numbers in the router's row order: (bank [R, D], sims [nprompt, R]) as float64."""
    ref_bank = np.concatenate([bank["art_bank"], bank["art_neg"][None], bank["nud_bank"], bank["nud_neg"][None],
                               bank["nud_anchor"][None]]).astype(np.float64)
    ref_sims = np.concatenate([prompts["art_sims"], prompts["art_neg"][:, None], prompts["nud_sims"],
                               prompts["nud_neg"][:, None], prompts["nud_anchor"][:, None]], axis=1).astype(np.float64)
    return ref_bank, ref_sims


def golden_expected_words(bank, prompts):
    names = bank["remover_concepts"]
    return np.array([sum(1 << names.index(c) for c in cs) for cs in prompts["expected"]], dtype=np.uint32)
