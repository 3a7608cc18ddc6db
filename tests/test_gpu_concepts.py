"""The concept router on the MI355X: sdmoe_text_pool and sdmoe_concept_route against the NumPy float64 restatement
(tests/concept_ref.py) on padded, offset and poisoned buffers, the group rule's edges stated exactly, the reference
checkers' recorded run (tests/golden/concept_*.npz) through ConceptRouter, and the whole chain from prompts to removal
images through the pipeline's prompt hook.

Bars: features and sims within 1e-12 absolute of the float64 restatement (the project's float64 bar, as
sdmoe_clip_scores); select words equal, after asserting on the CPU that no comparison of the inputs has a margin under
1e-9; against the reference's fp32 numbers the a-priori gap (L + 2 D) 2^-24; images torch.equal.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concept_ref as C  # noqa: E402

from sdmoe import _lib, ops  # noqa: E402
from sdmoe.concepts import ConceptRouter  # noqa: E402

DEV = "cuda"
F64_BAR = 1e-12
MARGIN = 1e-9

# (B, L, D, R): one row / one chunk; odd everything; the stub's shape; SD-1.x width (two row slices); D % 8 != 0 with
# more bank rows than select bits; SDXL's wider tower (one row slice)
SHAPES = [(1, 1, 8, 1), (3, 5, 40, 3), (2, 77, 64, 5), (4, 77, 768, 7), (5, 77, 100, 33), (2, 77, 1280, 4)]
LAYOUTS = ["dense", "padded", "offset1"]


def case(B, L, D, R, seed=0):
    """Host inputs of one kernel case: fp16 rows, float64 bank, row bits, groups, preset."""
    rng = np.random.default_rng(1000 * seed + 7 * B + 3 * L + D + R)
    bank = rng.standard_normal((R, D))
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    # every prompt leans towards a bank row, so the sims are not all alike
    lean = bank[rng.integers(0, R, B)]
    X = (0.3 * rng.standard_normal((B, L, D)) + lean[:, None, :] + 0.1 * rng.standard_normal((B, 1, D)))
    X = X.reshape(B * L, D).astype(np.float16)
    row_bit = [-1 if r % 5 == 4 else (r * 7) % 32 for r in range(R)]
    if R >= 3:
        groups = [(0, R - 2, R - 2, R - 1, None), (0, max(1, R // 2), R - 1, -1, 0.05)]
    else:  # too few rows for a group with its own no-concept row: one row against the other, or no group at all
        groups = [(0, 1, 1, -1, None)] if R == 2 else []
    preset = rng.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32) & np.uint32(0x00F00000)
    return X, bank, row_bit, groups, preset


def expected(X, B, bank, row_bit, groups, preset):
    feats = C.pool(X, B)
    sel, sims = C.route(feats, bank, row_bit, groups, preset)
    return feats, sel, sims


def test_case_margins_on_the_cpu():
    """No case decides anything by rounding: every comparison margin of every case's inputs is at least 1e-9."""
    for B, L, D, R in SHAPES:
        X, bank, row_bit, groups, preset = case(B, L, D, R)
        _, _, sims = expected(X, B, bank, row_bit, groups, preset)
        assert C.margins(sims, groups).min() >= MARGIN, (B, L, D, R)


def place(a, layout, poison):
    """A device view of host array a [rows, cols] in one of the layouts, the bytes around it poisoned."""
    rows, cols = a.shape
    t = torch.from_numpy(a)
    if layout == "dense":
        return t.to(DEV)
    if layout == "padded":
        ld = cols + 16 + (-cols % 8)  # a multiple of 8: 16-byte loads stay possible, with a ragged last chunk
        buf = torch.full((rows, ld), poison, dtype=t.dtype, device=DEV)
        buf[:, :cols] = t.to(DEV)
        return buf[:, :cols]
    buf = torch.full((rows * cols + 9,), poison, dtype=t.dtype, device=DEV)  # the pointer off by one element
    view = buf[1:1 + rows * cols].view(rows, cols)
    view.copy_(t.to(DEV))
    return view


def i32(words):
    return torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B,L,D,R", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_text_pool_and_concept_route_match_the_restatement(B, L, D, R, layout):
    X, bank, row_bit, groups, preset = case(B, L, D, R)
    feats, sel, sims = expected(X, B, bank, row_bit, groups, preset)
    assert C.margins(sims, groups).min() >= MARGIN
    x = place(X, layout, float("nan"))
    if layout == "offset1":
        assert x.data_ptr() % 4 == 2  # the 2-byte path
    bk = place(bank, "padded" if layout == "padded" else "dense", float("nan"))
    # features: per prompt, the whole batch as one group with and without the second normalisation
    for group, renorm in ((1, False), (B, False), (B, True)):
        out = torch.full((B // group, D), float("nan"), dtype=torch.float64, device=DEV)
        got = ops.text_pool(x, B, group=group, renorm=renorm, out=out)
        assert got.data_ptr() == out.data_ptr()
        exp = C.text_pool(X, B, group, renorm)
        err = np.abs(got.cpu().numpy() - exp).max()
        print(f"text_pool group={group} renorm={renorm}: max err {err:.3e}")
        assert err <= F64_BAR, (group, renorm, err)
    assert np.abs(ops.text_pool(x, B).cpu().numpy() - feats).max() <= F64_BAR
    # route: poisoned outputs, preset in
    sel_out = torch.full((B,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    sims_out = torch.full((B, R), float("nan"), dtype=torch.float64, device=DEV)
    s, sm = ops.concept_route(x, B, bk, row_bit, groups, preset=i32(preset), select_out=sel_out, sims_out=sims_out)
    assert s.data_ptr() == sel_out.data_ptr() and sm.data_ptr() == sims_out.data_ptr()
    err = np.abs(sm.cpu().numpy() - sims).max()
    print(f"sims: max err {err:.3e}; select {[hex(w) for w in u32(s)]}")
    assert err <= F64_BAR, err
    assert np.array_equal(u32(s), sel)
    # without sims_out, tables already on the device: the same words
    s2, none = ops.concept_route(x, B, bk, torch.tensor(row_bit, dtype=torch.int32, device=DEV),
                                 ops.concept_groups(groups, R, DEV), preset=i32(preset), sims=False)
    assert none is None and torch.equal(s2, s)
    if layout != "dense":  # the 16-byte and the 2-byte path add the same numbers in the same order
        xd = torch.from_numpy(X).to(DEV)
        sd, smd = ops.concept_route(xd, B, bk, row_bit, groups, preset=i32(preset))
        assert torch.equal(sd, s) and torch.equal(smd.view(torch.int64), sm.view(torch.int64))


def test_wrappers_refuse_what_the_kernels_do_not_take():
    x = torch.zeros((2 * 3, 16), dtype=torch.float16, device=DEV)
    bank = torch.zeros((2, 16), dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError):
        ops.text_pool(x.float(), 2)
    with pytest.raises(ValueError):
        ops.text_pool(x, 4)                      # 6 rows are not 4 sequences
    with pytest.raises(ValueError):
        ops.text_pool(x, 2, group=3)
    with pytest.raises(ValueError):
        ops.text_pool(torch.zeros((2, 2056), dtype=torch.float16, device=DEV), 2)  # D > 2048
    with pytest.raises(ValueError):
        ops.concept_route(x, 2, bank[:, :8], [0, 1], [])
    with pytest.raises(ValueError):
        ops.concept_route(x, 2, bank, [0, 1], [], preset=torch.zeros(3, dtype=torch.int32, device=DEV))
    lib = _lib.load()
    assert lib.sdmoe_text_pool(x.data_ptr(), 4096, 2, 3, 2049, 1, 0, bank.data_ptr(), 4096, None) == -3


# ---- the rule's edges, exact ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges():
    """Four prompts of 4 rows, D = 64, over an orthonormal frame e0..e5: prompt b's rows are a fixed mix of the frame
    plus small noise, prompt 3 is all zero. Bank rows: 0, 1 identical (e0-ish), 2 = e1, 3 = -e0, 4 = e2 (a no-concept
    row), 5 = e0 + e3 (an anchor)."""
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.standard_normal((64, 6)))
    e = q.T
    mix = np.array([[1.0, 0.3, 0.1, 0.0, 0.0, 0.0],    # mostly e0
                    [0.2, 1.0, 0.3, 0.0, 0.0, 0.0],    # mostly e1
                    [0.4, 0.1, 0.7, 0.8, 0.0, 0.0]])   # between e0, e2 and e3
    X = np.zeros((4, 4, 64))
    X[:3] = (mix @ e)[:, None, :] + 0.02 * rng.standard_normal((3, 4, 64))
    X = X.reshape(16, 64).astype(np.float16)
    row = (e[0] + 0.1 * e[4]) / np.linalg.norm(e[0] + 0.1 * e[4])
    bank = np.stack([row, row.copy(), e[1], -e[0], e[2], (e[0] + e[3]) / np.sqrt(2)])
    return torch.from_numpy(X).to(DEV), torch.from_numpy(bank).to(DEV), X, bank


def run(edges, row_bit, groups, preset=None):
    x, bank, X, bank_h = edges
    sel, sims = ops.concept_route(x, 4, bank, row_bit, groups, preset=None if preset is None else i32(preset))
    sims_h = sims.cpu().numpy()
    # whatever the case: the words are the rule applied to the sims the kernel wrote, and prompt 3 is NaN
    exp, _ = C.route(np.zeros((4, 1)), np.zeros((1, 1)), row_bit, [], preset)
    for b in range(4):
        for g in groups:
            fire, best = C.group_fires(sims_h[b], g)
            if fire and row_bit[best] >= 0:
                exp[b] |= np.uint32(1 << row_bit[best])
    assert np.array_equal(u32(sel), exp)
    assert np.isnan(sims_h[3]).all() and not np.isnan(sims_h[:3]).any()
    return u32(sel), sims_h


def test_rule_first_of_identical_rows_wins(edges):
    sel, sims = run(edges, [3, 4, 5, -1, -1, -1], [(0, 3, 4, -1, None)])
    assert sims[0, 0] == sims[0, 1] and sims[0, 0] > sims[0, 2]  # identical rows: bit-identical sims
    assert sel[0] == 1 << 3                                      # row 0's bit, not row 1's
    assert sel[1] == 1 << 5 and sel[3] == 0
    sel, _ = run(edges, [4, 3, 5, -1, -1, -1], [(0, 3, 4, -1, None)])
    assert sel[0] == 1 << 4


def test_rule_threshold_is_strict(edges):
    _, sims = run(edges, [0, 0, 1, -1, -1, -1], [(0, 3, 4, -1, None)])
    m = float(sims[0, 0])  # prompt 0's maximum, as the kernel wrote it
    sel, _ = run(edges, [0, 0, 1, -1, -1, -1], [(0, 3, 4, -1, m)])
    assert sel[0] == 0  # m > m is false
    sel, _ = run(edges, [0, 0, 1, -1, -1, -1], [(0, 3, 4, -1, float(np.nextafter(m, -np.inf)))])
    assert sel[0] == 1
    sel, _ = run(edges, [0, 0, 1, -1, -1, -1], [(0, 3, 4, -1, float(np.nextafter(m, np.inf)))])
    assert sel[0] == 0


def test_rule_anchor_clause_alone(edges):
    # group over row 3 (-e0) only: for prompt 2 its sim is below the no-concept row 4, the anchor row 5 is above it
    sel, sims = run(edges, [-1, -1, -1, 7, -1, -1], [(3, 4, 4, 5, None)])
    assert sims[2, 3] < sims[2, 4] < sims[2, 5] and sel[2] == 1 << 7
    assert sims[1, 5] < sims[1, 4] and sims[1, 3] < sims[1, 4] and sel[1] == 0  # neither clause
    sel, _ = run(edges, [-1, -1, -1, 7, -1, -1], [(3, 4, 4, -1, None)])          # no anchor: nothing
    assert sel[2] == 0


def test_rule_unknown_argmax_removes_nothing(edges):
    sel, sims = run(edges, [-1, -1, 9, 9, -1, -1], [(0, 4, 4, -1, None)])
    assert sims[0, 0] > sims[0, 2] > sims[0, 4]  # the runner-up row 2 is known and would fire
    assert sel[0] == 0
    assert sel[1] == 1 << 9                      # prompt 1's arg-max is row 2


def test_rule_bit31_preset_and_no_groups(edges):
    preset = np.array([0x10, 0, 0x80000000, 0x44], dtype=np.uint32)
    sel, _ = run(edges, [31, 31, 0, -1, -1, -1], [(0, 3, 4, -1, None)], preset)
    # prompt 0 fires bit 31 next to its preset, prompt 1 bit 0, prompt 2 stays under its no-concept row, and the
    # all-zero prompt keeps the preset alone
    assert sel.tolist() == [0x80000010, 1, 0x80000000, 0x44]
    sel, sims = run(edges, [31, 31, 0, -1, -1, -1], [], preset)
    assert sel.tolist() == preset.tolist()       # G = 0
    sel, _ = run(edges, [31, 31, 0, -1, -1, -1], [])
    assert sel.tolist() == [0, 0, 0, 0]


def test_two_launches_are_bit_identical():
    B, L, D, R = SHAPES[3]
    X, bk, row_bit, groups, preset = case(B, L, D, R)
    xd, bd = torch.from_numpy(X).to(DEV), torch.from_numpy(bk).to(DEV)
    a = ops.concept_route(xd, B, bd, row_bit, groups, preset=i32(preset))
    b = ops.concept_route(xd, B, bd, row_bit, groups, preset=i32(preset))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    f, g = ops.text_pool(xd, B, group=2, renorm=True), ops.text_pool(xd, B, group=2, renorm=True)
    assert torch.equal(f.view(torch.int64), g.view(torch.int64))


# ---- the reference checkers' recorded run -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    g = C.load_golden()
    bank, pr = g["bank"], g["prompts"]
    hidden = dict(zip(bank["bank_prompts"], bank["hidden"]))
    hidden.update(zip(pr["prompts"], pr["hidden"]))
    tok = C.StubTokenizer()
    enc = C.StubTextEncoder(tok, DEV, hidden)
    return bank, pr, enc, tok


def test_router_reproduces_the_reference_checkers(gold):
    bank, pr, enc, tok = gold
    r = ConceptRouter(enc, tok, DEV)
    r.add_art_styles(bank["art"], bank["things"], bank["humans"], threshold=bank["threshold"])
    r.add_nudity(bank["nudity"], bank["humans"], bank["things"], bank["anchors"], label="naked")
    assert enc.calls == 2  # one batched encode per checker
    labels, groups = C.golden_router_tables(bank)
    assert r.row_labels == labels
    assert [g[:4] for g in r.groups] == [g[:4] for g in groups] and r.groups[0][4] == bank["threshold"]
    ref_bank, ref_sims = C.golden_reference_rows(bank, pr)
    err_bank = np.abs(r.bank.cpu().numpy() - ref_bank).max()
    assert np.abs(r.bank.cpu().numpy() - C.golden_bank_restated(bank)).max() <= F64_BAR
    assert r.bind(bank["remover_concepts"]) == [1, -1, 2, -1, 0, 0, -1, -1]
    sel = r.select(pr["prompts"])
    assert enc.calls == 3 and sel.dtype == torch.int32 and sel.is_cuda
    err_sims = np.abs(r.last_sims.cpu().numpy() - ref_sims).max()
    print(f"max |bank - reference| = {err_bank:.3e}, max |sims - reference| = {err_sims:.3e} (bound {C.COS_GAP:.3e})")
    assert err_bank <= C.COS_GAP and err_sims <= C.COS_GAP
    assert np.array_equal(u32(sel), C.golden_expected_words(bank, pr))
    assert r.names(sel) == pr["expected"]
    # a memorized caption presets its bit next to what the device decides
    r.add_memorized([pr["prompts"][2], "never asked"], label="memorize")
    r.bind(bank["remover_concepts"] + ["memorize"])
    sel2 = r.select(pr["prompts"][:4])
    exp = C.golden_expected_words(bank, pr)[:4].copy()
    exp[2] |= 1 << 3
    assert np.array_equal(u32(sel2), exp)


def test_checker_shells_answer_as_the_reference(gold):
    from benchmarks.concept_checkers import ArtStyleChecker, NudityChecker
    bank, pr, enc, tok = gold
    art = ArtStyleChecker(DEV, bank["things"], bank["humans"], concepts_to_remove=bank["art"], text_encoder=enc,
                          tokenizer=tok)
    nud = NudityChecker(DEV, bank["humans"], bank["things"], concepts_to_remove=bank["nudity"], text_encoder=enc,
                        tokenizer=tok, anchor_prompts=bank["anchors"])
    assert [art.decide(p) for p in pr["prompts"]] == pr["art_decide"]
    assert [nud.decide(p) for p in pr["prompts"]] == pr["nud_decide"]
    sim, feat = art.similarity(pr["prompts"][0])
    assert list(sim) == bank["art"] and tuple(feat.shape) == (1, C.D_STUB)
    got = np.array([float(sim[c]) for c in bank["art"]])
    assert np.abs(got - pr["art_sims"][0]).max() <= C.COS_GAP


# ---- from prompts to removal images -----------------------------------------------------------------------------------
PROMPTS = ["a dog in the style of van gogh", "a painting of a river", "water lilies by monet",
           "a naked person on a beach"]
STEPS = 3


class _Ctx:
    pass


def choose_threshold(sims, row_bit, groups, names):
    """The art group's threshold, chosen on the restatement: the first candidate (none, then the midpoints between
    the prompts' sorted group maxima) for which the sets hold the empty set and two distinct non-empty ones."""
    row0, row1 = groups[0][:2]
    m = np.sort(sims[:, row0:row1].max(axis=1))
    for thr in [None] + [float((a + b) / 2) for a, b in zip(m[:-1], m[1:])]:
        gs = [groups[0][:4] + (thr,)] + list(groups[1:])
        sel = np.zeros(len(sims), dtype=np.uint32)
        for b in range(len(sims)):
            for g in gs:
                fire, best = C.group_fires(sims[b], g)
                if fire and row_bit[best] >= 0:
                    sel[b] |= np.uint32(1 << row_bit[best])
        sets = {frozenset(s) for s in C.names_of(sel, names)}
        if frozenset() in sets and len(sets) >= 3 and C.margins(sims, gs).min() >= MARGIN:
            return thr, gs, sel
    raise AssertionError(f"no threshold separates the prompts: maxima {m}")


@pytest.fixture(scope="module")
def pctx():
    """4 prompts with CFG, 3 DDIM steps on UNetConfig.tiny(32) (levels 32x32 .. 4x4: the one-launch, forced-tile and
    per-run paths of linear_masked_sets all occur) with the tiny text encoder of the U-Net's cross-attention width
    attached; two concepts, 'van gogh' and 'naked', of random 0.3-density masks; a router with an art group ('van gogh',
    and 'monet' which the remover lacks) and a nudity-style group labelled 'naked'."""
    from neuron_receivers import MultiConceptRemoverWanda, WandaRemoveNeuronsFast, WandaRemovePerPrompt
    from sdmoe.clip import attach_text_encoders
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline
    from sdmoe.unet import UNet2DConditionModel
    from sdmoe.weights import make_state_dict
    c = _Ctx()
    cfg = UNetConfig.tiny(32)
    unet = UNet2DConditionModel.from_state_dict(make_state_dict(cfg, 41), cfg, DEV)
    c.pipe = StableDiffusionPipeline(unet, DEV, num_inference_steps=STEPS)
    attach_text_encoders(c.pipe, seed=5)
    assert c.pipe.text_encoder.config.hidden_size == cfg.cross_attention_dim
    c.synth = StableDiffusionPipeline(unet, DEV, num_inference_steps=STEPS)  # synthetic conditioning, same U-Net
    downs = [m for n, m in unet.named_modules() if n.endswith("ff.net.2")]
    c.T, c.L = STEPS, len(downs)
    rng = np.random.default_rng(42)
    masks = {k: {t: {l: (rng.random(tuple(downs[l].weight.shape)) < 0.3).astype(np.int64) for l in range(c.L)}
                 for t in range(c.T)} for k in ("van gogh", "naked")}
    c.removers = {k: WandaRemoveNeuronsFast(0, None, c.T, c.L, masks=m, store_gates=False) for k, m in masks.items()}
    c.mc = MultiConceptRemoverWanda(None, 0, c.T, c.L, concepts_to_remove=list(masks), removers=c.removers)
    c.rec = WandaRemovePerPrompt(c.removers, seed=0, store_gates=False)
    r = c.router = ConceptRouter(c.pipe.text_encoder, c.pipe.tokenizer, DEV)
    r.add_art_styles(["van gogh", "monet"], ["dog", "river"], ["person", "man"], threshold=0.55)
    r.add_nudity(("naked", "nude"), ["person", "man"], ["dog", "river"], ["a nude on a beach", "bare skin"], label="naked")
    c.names = list(masks)  # the remover's concept order; 'monet' stays unknown to it
    r.bind(c.names)
    assert r.row_bit == [0, -1, -1, 1, 1, -1, -1]

    def explicit(pipe, sets):
        c.rec.set_prompt_concepts(sets)
        c.rec.reset_time_layer()
        out, _ = c.rec.observe_activation(pipe, PROMPTS)
        return [o.clone() for o in out]
    c.explicit = explicit

    def restated(rows):
        """(threshold groups, select words) the restatement gives for fp16 rows [B * 77, D] from the device."""
        feats = C.pool(rows.cpu().numpy(), len(PROMPTS))
        _, sims = C.route(feats, r.bank.cpu().numpy(), r.row_bit, [])
        return choose_threshold(sims, r.row_bit, r.groups, c.names)
    c.restated = restated
    return c


def test_routed_call_equals_the_explicit_sets(pctx):
    c, r, B = pctx, pctx.router, len(PROMPTS)
    ctx = c.pipe.encode_prompt(PROMPTS)
    cond = ctx[B * 77:]
    thr, groups, words = c.restated(cond)
    sets = C.names_of(words, c.names)
    print(f"threshold {thr}, sets {sets}")
    assert [] in sets and len({frozenset(s) for s in sets if s}) >= 2
    r.set_threshold(0, thr)
    imgs, sel = c.mc.remove_concepts_routed(c.pipe, PROMPTS, r)
    assert sel.dtype == torch.int32 and sel.is_cuda and np.array_equal(u32(sel), words)
    assert r.names(sel) == sets
    assert c.pipe._prompt_hooks == [] and c.mc.per_prompt_remover.prompt_sets == []  # nothing left behind
    exp = c.explicit(c.pipe, sets)
    for i in range(B):
        assert torch.equal(imgs[i], exp[i]), i
    # the receiver's own entry: router= and no sets configured
    from neuron_receivers import WandaRemovePerPrompt
    rec = WandaRemovePerPrompt(c.removers, seed=0, store_gates=False, router=r)
    out, _ = rec.observe_activation(c.pipe, PROMPTS)
    assert np.array_equal(u32(rec.last_select), words) and all(torch.equal(out[i], exp[i]) for i in range(B))
    # the conditioning rows of the call and the router's own encode decide alike, bit for bit
    a = r.select_from_hidden(cond, B)
    sims_a = r.last_sims.clone()
    b = r.select(PROMPTS)
    print(f"max |sims(conditioning rows) - sims(own encode)| = {(sims_a - r.last_sims).abs().max().item():.3e}")
    assert torch.equal(a, b) and np.array_equal(u32(a), words)


def test_pipeline_without_a_prompt_hook_is_the_parent_path(pctx):
    """pipe(prompts) with no hook registered against the parent's __call__ body restated here; a hook that was
    registered and removed, or one that does nothing, changes no bit either."""
    from sdmoe.pipeline import initial_latents
    from sdmoe.unet import IN_PAD, OUT_PAD
    pipe, B = pctx.pipe, len(PROMPTS)
    assert pipe._prompt_hooks == []
    torch.manual_seed(0)
    got = pipe(PROMPTS, seed=0).images
    cfg = pipe.config
    lat = torch.cat([initial_latents(0, i, cfg) for i in range(B)]).to(DEV, torch.float32).contiguous()
    ctx = pipe.encode_prompt(PROMPTS)
    HW = cfg.sample_size ** 2
    x_in = torch.zeros((2 * B * HW, IN_PAD), dtype=torch.float16, device=DEV)
    eps = torch.empty((2 * B * HW, OUT_PAD), dtype=torch.float16, device=DEV)
    ops.prepare_input(lat, x_in, 2)
    pipe._denoise(dict(lat=lat, x_in=x_in, eps=eps, ctx=ctx, add_hidden=None), STEPS, pipe.guidance_scale, True)
    for i in range(B):
        assert torch.equal(got[i], lat[i]), i
    seen = []
    h = pipe.register_prompt_hook(lambda prompts, ctx, n: seen.append((list(prompts), tuple(ctx.shape), n)))
    again = pipe(PROMPTS, seed=0).images
    h.remove()
    assert seen == [(PROMPTS, (2 * B * 77, cfg.cross_attention_dim), B)]
    after = pipe(PROMPTS, seed=0).images
    assert len(seen) == 1 and all(torch.equal(got[i], again[i]) and torch.equal(got[i], after[i]) for i in range(B))


def test_routed_call_on_synthetic_conditioning(pctx):
    """No text encoder on the pipeline: the hook lets the router encode the prompts itself."""
    c, r, B = pctx, pctx.router, len(PROMPTS)
    assert c.synth.text_encoder is None
    thr, groups, words = c.restated(r.encode(PROMPTS))
    sets = C.names_of(words, c.names)
    r.set_threshold(0, thr)
    imgs, sel = c.mc.remove_concepts_routed(c.synth, PROMPTS, r)
    assert np.array_equal(u32(sel), words)
    exp = c.explicit(c.synth, sets)
    assert all(torch.equal(imgs[i], exp[i]) for i in range(B))
    assert any(not torch.equal(imgs[i], e) for i, e in enumerate(c.explicit(c.synth, [[]] * B)) if sets[i])
