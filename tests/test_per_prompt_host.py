"""Per-prompt concept sets, host side (no GPU): the launch plans of sdmoe_linear_masked_sets over every FFN down
projection of SD-1.4 and SDXL, their agreement with sdmoe_linear_masked's plans, the refusals, and the set
bookkeeping of WandaRemovePerPrompt."""
import numpy as np
import pytest

from unet_shapes import PROMPTS_PER_CALL, down_projection_shapes


def _cases():
    """(M, K, N, rows_per_img) of every down projection at 1 / 2 / 8 / 16 prompts per call (CFG: 2 images a prompt)."""
    out = []
    for model in ("sd14", "sdxl"):
        for b in PROMPTS_PER_CALL:
            for M, K, N in down_projection_shapes(model, prompts=(b,)):
                assert M % (2 * b) == 0
                out.append((M, K, N, M // (2 * b)))
    return sorted(set(out))


def test_plan_covers_every_unet_down_projection():
    from sdmoe import ops
    cases = _cases()
    assert (1024, 5120, 1280, 64) in cases      # SD-1.4 mid block at 8 prompts
    assert (131072, 2560, 640, 4096) in cases   # SDXL 64x64 level at 16 prompts
    for M, K, N, rpi in cases:
        for keep in (False, True):
            for res in (False, True):
                pl = ops.gemm_plan_sets(M, N, K, rpi, keep=keep, residual=res)
                assert rpi % pl["tile"][0] == 0, (M, K, N, rpi, keep, pl)
                assert pl["ksplit"] >= 1, (M, K, N, rpi, keep, pl)


def test_plan_agrees_with_the_masked_plan_where_its_tile_divides_an_image():
    """Tile and split of sdmoe_linear_masked itself wherever that tile's rows divide rows_per_img (a uniform table then
    gives its bits); elsewhere a 64-row tile. Compared against the sdmoe_gemm_plan query, not a table."""
    from sdmoe import ops
    sweep = [(m * rpi, k, n, rpi) for rpi in (64, 128, 256, 1024, 4096) for m in (1, 2, 6, 16, 32)
             for k in (320, 1280, 5120) for n in (320, 640, 1280, 200)]
    agreed = forced = 0
    for M, K, N, rpi in _cases() + sweep:
        for keep, mode in ((False, "wmask"), (True, "keepw")):
            for res in (False, True):
                ref = ops.gemm_plan(mode, M, N, K, residual=res)
                got = ops.gemm_plan_sets(M, N, K, rpi, keep=keep, residual=res)
                if rpi % ref["tile"][0] == 0:
                    assert got == ref, (M, K, N, rpi, mode, got, ref)
                    agreed += 1
                else:
                    assert got["tile"] == (64, 160 if N % 160 == 0 else 128), (M, K, N, rpi, mode, got, ref)
                    forced += 1
    assert agreed and forced
    # the one U-Net shape on a forced tile: the mid block (one 8x8 image = 64 rows; its own plan is a 256-row tile)
    assert ops.gemm_plan("wmask", 1024, 1280, 5120)["tile"][0] == 256
    assert ops.gemm_plan_sets(1024, 1280, 5120, 64)["tile"] == (64, 160)
    # without a workspace nothing splits
    assert ops.gemm_plan_sets(1024, 1280, 5120, 64, workspace_floats=0)["ksplit"] == 1


def test_plan_refuses_images_no_tile_divides():
    from sdmoe import _lib, ops
    for rpi in (16, 4):
        for keep in (False, True):
            with pytest.raises(_lib.SdmoeError, match=r"\(-3\)"):
                ops.gemm_plan_sets(6 * rpi, 320, 1280, rpi, keep=keep)
    with pytest.raises(_lib.SdmoeError, match=r"\(-2\)"):
        ops.gemm_plan_sets(100, 320, 1280, 64)       # not whole images
    lib = _lib.load()
    # the launch refuses the same shapes before it touches a pointer
    assert lib.sdmoe_linear_masked_sets(1, 1280, None, 1, 1280, 1, 20 * 320, 1, 2, 16, None, None, 0, 1, 320, 96, 320,
                                        1280, None, 0, None) == -3
    assert lib.sdmoe_linear_masked_sets(1, 1280, None, 1, 1280, None, 20 * 320, 1, 2, 64, None, None, 0, 1, 320, 128,
                                        320, 1280, None, 0, None) == -1
    assert lib.sdmoe_linear_masked_sets(1, 1280, None, 1, 1280, 1, 20 * 320 - 1, 1, 2, 64, None, None, 0, 1, 320, 128,
                                        320, 1280, None, 0, None) == -1  # overlapping sets
    assert lib.sdmoe_wmask_union_sets(1, 8, 33, 1, 2, 8, 1, None) == -1
    assert lib.sdmoe_wmask_union_sets(1, 4, 3, 1, 2, 8, 1, None) == -1   # stride under the mask's words


def _removers(names, T=2, L=3, C=8):
    from neuron_receivers import WandaRemoveNeuronsFast
    rng = np.random.default_rng(0)
    out = {}
    for n in names:
        packed = {t: {l: rng.integers(0, 256, (C, 4 * C // 8), dtype=np.uint8) for l in range(L)} for t in range(T)}
        out[n] = WandaRemoveNeuronsFast.from_packed(0, packed, T, L)
    return out


def test_set_bookkeeping():
    from sdmoe._lib import SdmoeError
    from neuron_receivers import WandaRemovePerPrompt
    rec = WandaRemovePerPrompt(_removers(["a", "b", "c"]))
    assert (rec.T, rec.n_layers) == (2, 3) and rec._sdmoe_receiver
    ids = rec.set_prompt_concepts([["a"], [], ["c", "a"], ["a"], ["a", "c"], []])
    assert ids == [0, 1, 2, 0, 2, 1] == rec.prompt_sets               # distinct sets deduplicated, order of first use
    assert rec.sets == [frozenset({"a"}), frozenset(), frozenset({"a", "c"})]
    assert rec.select == [0b001, 0, 0b101]                            # the empty set selects nothing
    assert rec.image_table(6) == ids                                  # no guidance: one image per prompt
    assert rec.image_table(12) == ids + ids                           # CFG: [uncond x B ; cond x B]
    for nimg in (5, 7, 18, 0):
        with pytest.raises(SdmoeError):
            rec.image_table(nimg)
    with pytest.raises(SdmoeError, match="unknown concept"):
        rec.set_prompt_concepts([["a"], ["nope"]])
    with pytest.raises(SdmoeError):
        rec.set_prompt_concepts(["a"])                                # a bare string is not a list of concepts
    with pytest.raises(SdmoeError, match="2 prompts"):                # prompt-count mismatch, before anything runs
        rec.observe_activation(None, ["p0", "p1"])
    with pytest.raises(SdmoeError, match="at most 32"):
        WandaRemovePerPrompt(_removers([f"c{i}" for i in range(33)], T=1, L=1))
    rec32 = WandaRemovePerPrompt(_removers([f"c{i}" for i in range(32)], T=1, L=1))
    rec32.set_prompt_concepts([["c31"], ["c0", "c31"]])
    assert rec32.select == [1 << 31, (1 << 31) | 1]
    with pytest.raises(SdmoeError):
        WandaRemovePerPrompt(_removers(["a"]), hook_module='text')
    with pytest.raises(SdmoeError):
        rec.hook_fn(None, None, None)                                 # the GEGLU-gate variant
    with pytest.raises(SdmoeError):
        rec.text_hook_fn(None, None, None)


def test_image_set_runs():
    from sdmoe import ops
    assert ops.image_set_runs([0, 0, 1, 1, 1, 0, 2]) == [(0, 2, 0), (2, 5, 1), (5, 6, 0), (6, 7, 2)]
    assert ops.image_set_runs([]) == []
