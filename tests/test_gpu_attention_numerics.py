"""sdmoe_attention at realistic logit ranges, on every kernel variant, and with a guarded output.

The other attention tests draw q, k, v from N(0,1): logits of std 1, a nearly flat softmax, and after tile 0 a
running maximum that never moves by more than the deferred-rescale threshold. Here the inputs (attention_cases.py)
have logits of +-20 to +-60, maxima that move at every tile, at every second tile, for one row of a wave only, or
just before a tile of equal weight, a maximum on the last valid key beside the first masked one, and a large common
shift; and the output is a view into a sentinel-filled buffer. Reference: attention_cases.exact (fp64). Bar: close(), the suite's own -- max-abs 1e-2
(scaled) and relative L2 2e-3; test_attention_cases.py shows on the CPU that the fp16 formats alone stay within half
of it on each of these inputs.

Variants (sdmoe_tune knob `attn`): 0 by shape, 1 = 32x32x16, 2 / 4 = 16x16x32 with 32 / 64 queries per wave,
8 / 9 = 16x16x32 / 32x32x16 in 8-wave workgroups. All six at d = 40, 64, 80; the shape-chosen one at d = 32, 160; and
one pass of every forced variant at d = 160, whose launch falls through to the 4-wave kernels."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from sdmoe import ops, tune  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as ac  # noqa: E402
from test_gpu_kernels import close  # noqa: E402

DEV = "cuda"
COMBOS = [(variant, d) for d in ac.DIMS_ALL_VARIANTS for variant in ac.VARIANTS] + \
         [(0, d) for d in ac.DIMS_DEFAULT_ONLY]
COMBO_IDS = [f"d{d}-attn{variant}" for variant, d in COMBOS]
FAMILIES = ac.families()


@functools.lru_cache(maxsize=None)
def _case(family, cid, d):
    """inputs on the device and the fp64 reference, built once and shared by the variants (read-only)"""
    fn, args = next((fn, args) for c, fn, args in FAMILIES[family] if c == cid)
    q, k, v, nimg, Nq, Nk, heads = fn(d, *args)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    return q, k, v, nimg, Nq, Nk, heads, ac.exact(q, k, v, nimg, Nq, Nk, heads)


def _run(family, cid, d, variant):
    q, k, v, nimg, Nq, Nk, heads, ref = _case(family, cid, d)
    with tune.tuned(attn=variant):
        out = ops.attention(q, k, v, nimg, Nq, Nk, heads)
    rel, mx = ac.errors(out, ref)
    print(f"ATTN {family} {cid} d={d} attn={variant}: rel L2 {rel:.3e} scaled max err {mx:.3e}")
    close(out, ref)
    return out, ref


def _ids(family):
    return [cid for cid, _, _ in FAMILIES[family]]


@pytest.mark.parametrize("variant,d", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("cid", _ids("logit_scale"))
def test_logit_scale(cid, variant, d):
    """Logit std 4 and 12, several tiles with a ragged tail (200 keys) and the one-tile cross-attention shape."""
    _run("logit_scale", cid, d, variant)


@pytest.mark.parametrize("variant,d", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("cid", _ids("ramps"))
def test_ramps(cid, variant, d):
    """The maximum moves at every tile (+9), at every second one (+5), or never while the later tiles underflow."""
    _run("ramps", cid, d, variant)


@pytest.mark.parametrize("variant,d", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("cid", _ids("staircase"))
def test_staircase(cid, variant, d):
    """The maximum moves at one tile and the next tile sits at the same level, with V of opposite offset: the shift a
    tile is weighed with when it moves m and the shift stored for the tiles after it must be the same number (at
    d = 40 the 32x32x16 kernel keeps -m as an fp16 element of Q~ and takes delta between the ROUNDED shifts)."""
    _run("staircase", cid, d, variant)


@pytest.mark.parametrize("variant,d", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("cid", _ids("mixed"))
def test_mixed_waves(cid, variant, d):
    """One row of each 16-query fragment trips the wave-uniform rescale at every tile; the others must come through
    it with alpha = 1 (and the reverse)."""
    _run("mixed", cid, d, variant)


@pytest.mark.parametrize("variant,d", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("cid", _ids("last_key_spike"))
def test_maximum_on_the_last_valid_key(cid, variant, d):
    """The row maximum on key Nk - 1, beside the first masked key, or on the first key of the ragged tile. The
    spiked rows are one each of eight (image, head) pairs; each is also held to the bar on its own."""
    out, ref = _run("last_key_spike", cid, d, variant)
    q, k, v, nimg, Nq, Nk, heads, _ = _case("last_key_spike", cid, d)
    for b, h, r in ac.spiked_rows(Nq, heads):
        close(out[b * Nq + r, h * d:(h + 1) * d], ref[b * Nq + r, h * d:(h + 1) * d])


@pytest.mark.parametrize("variant,d", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("cid", _ids("key_offset"))
def test_key_offset_invariance(cid, variant, d):
    """A constant vector added to every key: |m| of 23 log2 units on a typical row, past 100 on the extreme ones,
    with the logit differences of std 4."""
    _run("key_offset", cid, d, variant)


@pytest.mark.parametrize("variant", [v for v in ac.VARIANTS if v])
@pytest.mark.parametrize("family,cid", [("logit_scale", "std4-200x200"), ("ramps", "slope+9")])
def test_forced_variants_fall_through_at_d160(family, cid, variant):
    """launch<160> has no 8-wave and no 64-query kernel: attn = 4, 8 fall through to the 4-wave 16x16x32 kernel,
    attn = 9 likewise, attn = 1 runs the 4-wave 32x32x16 one."""
    _run(family, cid, 160, variant)


SENTINEL = 0x7B2D  # a finite fp16 bit pattern (~58,784) the kernels do not produce here
JUNK = 1.0e4


@pytest.mark.parametrize("variant", ac.VARIANTS)
@pytest.mark.parametrize("d", ac.GUARD_DIMS)
@pytest.mark.parametrize("Nq", ac.GUARD_NQ)
def test_guarded_output(Nq, d, variant):
    """out is rows [g, g + nimg Nq) x columns [8, 8 + C) of a sentinel-filled [nimg Nq + 2g, C + 16] buffer
    (ldo = C + 16): the interior meets the bar and no sentinel changes a bit. q, k, v are column slices of one fused
    buffer whose other columns hold 1e4: a read from beside a head or tensor shows as a large error."""
    q, k, v, nimg, Nq, Nk, heads = ac.guarded(d, Nq)
    C, rows, g = heads * d, nimg * Nq, 5
    fused = torch.full((rows, 3 * C + 32), JUNK, dtype=torch.float16, device=DEV)
    views = []
    for i, t in enumerate((q, k, v)):
        c0 = 8 + i * (C + 8)
        fused[:, c0:c0 + C] = t.to(DEV)
        views.append(fused[:, c0:c0 + C])
    qv, kv, vv = views
    buf = torch.full((rows + 2 * g, C + 16), SENTINEL, dtype=torch.int16, device=DEV)
    out = buf.view(torch.float16)[g:g + rows, 8:8 + C]
    assert out.stride(0) == C + 16 and out.data_ptr() == buf.data_ptr() + 2 * (g * (C + 16) + 8)
    with tune.tuned(attn=variant):
        ret = ops.attention(qv, kv, vv, nimg, Nq, Nk, heads, out=out)
    assert ret.data_ptr() == out.data_ptr()
    ref = ac.exact(qv, kv, vv, nimg, Nq, Nk, heads)
    rel, mx = ac.errors(out, ref)
    print(f"ATTN guarded Nq{Nq} d={d} attn={variant}: rel L2 {rel:.3e} scaled max err {mx:.3e}")
    close(out, ref)
    guard = torch.ones_like(buf, dtype=torch.bool)
    guard[g:g + rows, 8:8 + C] = False
    assert guard.sum().item() == 2 * g * (C + 16) + 16 * rows
    assert (buf[guard] == SENTINEL).all(), "a store outside the output view"
    assert (fused[:, :8] == JUNK).all() and (fused[:, -8:] == JUNK).all()  # the inputs are only read
