"""CPU-only tests of the concept router: the NumPy restatement (tests/concept_ref.py) against the reference checkers'
recorded run (tests/golden/concept_*.npz), ConceptRouter's bookkeeping (bind, names, the memorized preset), the ops
wrappers' argument validation, and the receiver / pipeline seams' host side. No GPU compute is launched here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concept_ref as C  # noqa: E402

from sdmoe import _lib, ops  # noqa: E402
from sdmoe.concepts import ConceptRouter  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return C.load_golden()


def test_restatement_reproduces_the_reference_checkers(gold):
    """The reference computes in fp32, the restatement in float64 on the same fp16-representable inputs: bank rows and
    sims agree to the a-priori gap (L + 2 D) 2^-24, and -- the maker asserted every comparison's margin at 10x that --
    every decision is equal."""
    bank, pr = gold["bank"], gold["prompts"]
    mine = C.golden_bank_restated(bank)
    ref_bank, ref_sims = C.golden_reference_rows(bank, pr)
    assert mine.shape == ref_bank.shape == (8, C.D_STUB)
    err_bank = np.abs(mine - ref_bank).max()
    labels, groups = C.golden_router_tables(bank)
    names = bank["remover_concepts"]
    row_bit = [-1 if lab is None or lab not in names else names.index(lab) for lab in labels]
    assert row_bit == [1, -1, 2, -1, 0, 0, -1, -1]  # 'Monet' is unknown to the remover; naked / sexy share a bit
    n = len(pr["prompts"])
    assert n >= 24 and pr["hidden"].shape == (n, C.L_STUB, C.D_STUB)
    feats = C.pool(pr["hidden"].reshape(n * C.L_STUB, C.D_STUB), n)
    sel, sims = C.route(feats, mine, row_bit, groups)
    err_sims = np.abs(sims - ref_sims).max()
    print(f"max |bank - reference| = {err_bank:.3e}, max |sims - reference| = {err_sims:.3e} (bound {C.COS_GAP:.3e})")
    assert err_bank <= C.COS_GAP and err_sims <= C.COS_GAP
    assert C.margins(sims, groups).min() >= 9 * C.COS_GAP
    assert C.names_of(sel, names) == pr["expected"]
    assert np.array_equal(sel, C.golden_expected_words(bank, pr))
    # the checkers' own answers, group by group
    for b in range(n):
        fire, best = C.group_fires(sims[b], groups[0])
        assert (bank["art"][best] if fire else "none") == pr["art_decide"][b], pr["prompts"][b]
        fire, _ = C.group_fires(sims[b], groups[1])
        assert ("naked" if fire else "none") == pr["nud_decide"][b], pr["prompts"][b]
    # the fixture exercises what it claims: an arg-max the remover lacks, the anchor clause alone, the empty set
    assert "Monet" in pr["art_decide"] and pr["anchor_only"] and [] in pr["expected"]


def test_restatement_rule_edges():
    sims = np.array([0.5, 0.7, 0.7, 0.2, 0.9])
    assert C.group_fires(sims, (0, 3, 3, -1, None)) == (True, 1)  # the first row reaching the maximum
    assert C.group_fires(sims, (0, 3, 3, -1, 0.7)) == (False, 1)  # strict threshold
    assert C.group_fires(sims, (0, 3, 3, -1, np.nextafter(0.7, 0))) == (True, 1)
    assert C.group_fires(sims, (0, 1, 1, 4, None)) == (True, 0)   # 0.5 < 0.7 but the anchor 0.9 > 0.7
    assert C.group_fires(np.full(5, np.nan), (0, 3, 3, 4, None)) == (False, 0)
    sel, _ = C.route(np.eye(2), np.eye(2), [31, -1], [(0, 1, 1, -1, None), (1, 2, 0, -1, None)], preset=[4, 0])
    assert sel.tolist() == [(1 << 31) | 4, 0]  # bit 31 and the preset; an arg-max without a bit removes nothing
    z = C.pool(np.zeros((4, 8)), 2)
    assert np.isnan(z).all()


def _router(labels):
    r = ConceptRouter(None, None, "cpu")
    r._add_rows(torch.zeros((len(labels), 4), dtype=torch.float64), list(labels), [str(x) for x in labels])
    return r


def test_bind_maps_labels_to_bits():
    r = _router(["Van Gogh", "Monet", None, "naked", "naked", None, None])
    r.add_memorized(["a memorised caption"], label="memorize")
    assert r.labels() == ["Van Gogh", "Monet", "naked", "memorize"]
    with pytest.raises(_lib.SdmoeError):
        r.select_from_hidden(None, 1)  # not bound yet
    assert r.bind(["naked", "Van Gogh", "memorize"]) == [1, -1, -1, 0, 0, -1, -1]  # unknown -> -1, shared bit
    assert r.bind(["x"] * 0 + [f"c{i}" for i in range(31)] + ["Monet"])[1] == 31
    with pytest.raises(_lib.SdmoeError):
        r.bind([f"c{i}" for i in range(33)])
    with pytest.raises(_lib.SdmoeError):
        r.bind(["naked", "naked"])
    r.bind(["naked"])
    r._add_rows(torch.zeros((1, 4), dtype=torch.float64), ["late"], ["late"])
    assert r.row_bit is None  # a new row needs a new bind
    with pytest.raises(_lib.SdmoeError):
        r._add_rows(torch.zeros((1, 5), dtype=torch.float64), ["wide"], ["wide"])


def test_names_round_trip():
    r = _router(["a"])
    names = [f"c{i}" for i in range(32)]
    r.bind(names)
    sets = [[], ["c0"], ["c31"], ["c0", "c5", "c31"], names]
    words = np.array([sum(1 << names.index(c) for c in s) for s in sets], dtype=np.uint32)
    assert r.names(torch.from_numpy(words.view(np.int32).copy())) == sets  # int32 bit patterns, as on the device
    assert r.names(words) == sets
    assert C.names_of(words, names) == sets


def test_memorized_preset():
    r = ConceptRouter(None, None, "cpu").add_memorized(["The caption", "another one"], label="memorize")
    r.bind(["naked", "memorize"])
    prompts = ["the caption", "The caption", "x", "another one"]  # membership is exact, as the reference's `in`
    assert r.preset_words(prompts).tolist() == [0, 2, 0, 2]
    sel = r.select(prompts)  # no bank: nothing to launch, the preset is the answer
    assert sel.dtype == torch.int32 and sel.tolist() == [0, 2, 0, 2]
    assert r.names(sel) == [[], ["memorize"], [], ["memorize"]]
    r.bind(["naked"])  # the remover has no 'memorize': nothing is preset
    assert r.preset_words(prompts).tolist() == [0, 0, 0, 0]


def test_concept_groups_layout_and_checks():
    t = ops.concept_groups([(0, 3, 3, None, 0.55), (4, 6, 6, 7, None)], 8)
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, 6)  # sdmoe_concept_group: 4 ints + a double = 24 bytes
    assert t[:, :4].tolist() == [[0, 3, 3, -1], [4, 6, 6, 7]]
    thr = t[:, 4:].contiguous().numpy().view(np.float64).ravel()
    assert thr[0] == 0.55 and thr[1] == -np.inf
    assert tuple(ops.concept_groups([], 3).shape) == (0, 6)
    for bad in [(0, 0, 1, -1, None), (-1, 2, 2, -1, None), (0, 9, 2, -1, None), (0, 2, 8, -1, None),
                (0, 2, 2, 8, None), (0, 2, 2, -2, None)]:
        with pytest.raises(ValueError):
            ops.concept_groups([bad], 8)


def test_ops_validate_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    x = torch.zeros((4 * 77, 64), dtype=torch.float16)
    bank = torch.zeros((3, 64), dtype=torch.float64)
    with pytest.raises(_lib.SdmoeError):
        ops.text_pool(x, 4)  # not on a GPU: there is no CPU path
    with pytest.raises(ValueError):
        ops.text_pool(x[None], 4)
    with pytest.raises(_lib.SdmoeError):
        ops.concept_route(x, 4, bank, [0, 1, -1], [(0, 2, 2, -1, None)])
    with pytest.raises(ValueError):
        ops.concept_route(x, 4, bank, [0, 1], [(0, 2, 2, -1, None)])       # one bit per bank row
    with pytest.raises(ValueError):
        ops.concept_route(x, 4, bank, [0, 32, -1], [(0, 2, 2, -1, None)])  # bits 0..31
    with pytest.raises(ValueError):
        ops.concept_route(x, 4, bank, [0, 1, -1], [(0, 4, 2, -1, None)])   # rows outside the bank
    with pytest.raises(ValueError):
        ops.concept_route(x, 4, bank.float(), [0, 1, -1], [])
    with pytest.raises(ValueError):
        ops.concept_route(x, 4, bank, torch.zeros(3, dtype=torch.int64), [])
    with pytest.raises(ValueError):
        ops.concept_route(x, 4, bank, [0, 1, -1], torch.zeros((1, 5), dtype=torch.int32))


def test_abi_refuses_bad_arguments_without_gpu():
    lib = _lib.load()
    assert len(_lib.SIGNATURES["sdmoe_text_pool"]) == 10 and len(_lib.SIGNATURES["sdmoe_concept_route"]) == 15
    assert lib.sdmoe_text_pool(None, 0, 0, 77, 64, 1, 0, None, 0, None) == 0       # empty: a no-op
    assert lib.sdmoe_text_pool(None, 64, 2, 77, 64, 1, 0, None, 64, None) == -1
    assert lib.sdmoe_text_pool(16, 64, 3, 77, 64, 2, 0, 16, 64, None) == -1        # 3 sequences, groups of 2
    assert lib.sdmoe_text_pool(16, 32, 2, 77, 64, 1, 0, 16, 64, None) == -1        # ldx < D
    assert lib.sdmoe_text_pool(16, 4096, 2, 77, 2049, 1, 0, 16, 4096, None) == -3  # D > 2048
    assert lib.sdmoe_text_pool(17, 64, 2, 77, 64, 1, 0, 16, 64, None) == -2        # odd fp16 pointer
    assert lib.sdmoe_concept_route(None, 0, 0, 77, 64, None, 0, 1, None, None, 0, None, None, None, None) == 0
    assert lib.sdmoe_concept_route(16, 64, 2, 77, 64, 16, 64, 0, 16, None, 0, None, 16, None, None) == -1   # R = 0
    assert lib.sdmoe_concept_route(16, 64, 2, 77, 64, 16, 64, 3, 16, None, 1, None, 16, None, None) == -1   # G, no table
    assert lib.sdmoe_concept_route(16, 4096, 2, 77, 2049, 16, 4096, 3, 16, None, 0, None, 16, None, None) == -3
    assert lib.sdmoe_concept_route(16, 64, 2, 77, 64, 20, 64, 3, 16, None, 0, None, 16, None, None) == -2   # bank % 8


def _removers(names, T=1, L=1, C_=8):
    from neuron_receivers import WandaRemoveNeuronsFast
    rng = np.random.default_rng(0)
    return {n: WandaRemoveNeuronsFast(0, None, T, L, masks={t: {l: (rng.random((C_, 4 * C_)) < 0.3).astype(np.int64)
                                                                for l in range(L)} for t in range(T)},
                                      store_gates=False) for n in names}


def test_receiver_select_seam_host_side():
    from neuron_receivers import WandaRemovePerPrompt
    rec = WandaRemovePerPrompt(_removers(["a", "b"]), store_gates=False)
    assert rec.router is None and rec.last_select is None
    for bad in ([1, 2], torch.zeros(3, dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32),
                torch.zeros(0, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)):  # the last: not on a GPU
        with pytest.raises(_lib.SdmoeError):
            rec.set_prompt_select(bad)
    assert rec.set_prompt_concepts([["a"], [], ["a"]]) == [0, 1, 0] and rec.select == [1, 0]  # unchanged
    rec.clear_prompt_sets()
    assert rec.prompt_sets == [] and rec.select == []


def test_prompt_hook_handle():
    from sdmoe.pipeline import StableDiffusionPipeline
    pipe = StableDiffusionPipeline.__new__(StableDiffusionPipeline)
    pipe._prompt_hooks = []
    seen = []
    h = pipe.register_prompt_hook(lambda prompts, ctx, B: seen.append(B))
    assert len(pipe._prompt_hooks) == 1
    h.remove()
    h.remove()
    assert pipe._prompt_hooks == []


def test_checker_shells_keep_the_reference_names():
    from benchmarks import concept_checkers as cc
    for name in ("BaseConceptChecker", "ArtStyleChecker", "NudityChecker", "MemorizedPromptChecker"):
        assert hasattr(cc, name)
    assert cc.preprocess_concepts(["Van Gogh", "", "Alex Alemany,painter", "Monet"]) == (
        ["Van Gogh", "Alex Alemany,painter", "Monet"], ["Vincent Van Gogh", "Alex Alemany", "Claude Monet"])
    m = cc.MemorizedPromptChecker("cpu", None, None, prompts=["p1"])
    assert (m.decide("p1"), m.decide("p2")) == ("memorize", "none")
