"""Keeps the inputs of test_gpu_attention_numerics.py honest, without a GPU: on every case it uses, the fp16 formats
alone (attention_cases.emulate against attention_cases.exact) stay within HALF the bar the kernels are held to --
relative L2 <= 1e-3 and max |err| <= 5e-3 max(1, max |ref|) -- and each case family drives the kernel branch it is
meant to drive (attention_cases.rescale_rows restates the deferred-rescale rule)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as ac  # noqa: E402

HALF_REL_L2 = 1e-3
HALF_MAX = 5e-3

ALL = ac.cases() + ac.guarded_cases()


@pytest.mark.parametrize("fam,cid,d,fn,args", ALL, ids=[f"{c[0]}-{c[1]}-d{c[2]}" for c in ALL])
def test_formats_alone_within_half_the_bar(fam, cid, d, fn, args):
    case = fn(d, *args)
    q, k, v, nimg, Nq, Nk, heads = case
    assert q.dtype == k.dtype == v.dtype == torch.float16
    assert q.shape == (nimg * Nq, heads * d) and k.shape == v.shape == (nimg * Nk, heads * d)
    assert nimg == 2 and 2 <= heads <= 4 and Nq <= 300 and Nk <= 600
    assert k.abs().max().item() < 20 and torch.isfinite(q).all() and torch.isfinite(v).all()
    rel, mx = ac.errors(ac.emulate(*case), ac.exact(*case))
    print(f"{fam} {cid} d={d}: emulation rel L2 {rel:.3g}, scaled max err {mx:.3g}")
    assert rel <= HALF_REL_L2 and mx <= HALF_MAX, (rel, mx)
    # every builder is a pure function of its arguments
    again = fn(d, *args)
    assert all(torch.equal(a, b) for a, b in zip(case[:3], again[:3]))


def test_exact_is_plain_attention():
    q, k, v, nimg, Nq, Nk, heads = ac.logit_scale(40, 4.0, 130, 77)
    d = 40
    qf, kf, vf = (t.double().reshape(nimg, n, heads, d).transpose(1, 2) for t, n in ((q, Nq), (k, Nk), (v, Nk)))
    ref = F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(nimg * Nq, heads * d)
    assert (ac.exact(q, k, v, nimg, Nq, Nk, heads) - ref).abs().max().item() < 1e-12
    # and the scale argument is the logit scale
    half = ac.exact(q, k, v, nimg, Nq, Nk, heads, scale=0.5 * d ** -0.5)
    ref2 = F.scaled_dot_product_attention(qf * 0.5, kf, vf).transpose(1, 2).reshape(nimg * Nq, heads * d)
    assert (half - ref2).abs().max().item() < 1e-12


def test_emulate_rounds_where_stated():
    """On one key the softmax is 1 and the emulation returns fp16(v) exactly; with two equal keys P = 1, 1, l = 2."""
    q = torch.randn(4, 32, generator=torch.Generator().manual_seed(0)).half()
    v = torch.tensor([[1.0] * 32, [3.0] * 32]).half()
    k = torch.zeros(2, 32).half()
    assert torch.equal(ac.emulate(q, k[:1], v[:1], 1, 4, 1, 1), v[:1].expand(4, 32))
    assert torch.equal(ac.emulate(q, k, v, 1, 4, 2, 1), torch.full((4, 32), 2.0).half())
    # a logit gap of 30 log2 units underflows fp16 P (2^-30 < 2^-24): the second key drops out entirely
    q1 = torch.zeros(1, 32).half()
    q1[0, 0] = 1.0
    k2 = torch.zeros(2, 32).half()
    k2[1, 0] = -30.0 / (ac.LOG2E * 32 ** -0.5)
    assert torch.equal(ac.emulate(q1, k2, v, 1, 1, 2, 1), v[:1])


@pytest.mark.parametrize("group", [16, 32])
@pytest.mark.parametrize("d", ac.ALL_DIMS)
def test_ramps_drive_the_rescale(d, group):
    nfull = ac.RAMP_NK // ac.KB  # the ragged tile after them holds 8 keys: too short a rise to trip anything
    for slope in (9.0, 5.0, -9.0):
        q, k, v, nimg, Nq, Nk, heads = ac.ramps(d, slope)
        own, fired = ac.rescale_rows(q, k, nimg, Nq, Nk, heads, group=group)
        own, fired = own[..., 1:nfull], fired[..., 1:nfull]  # the full tiles after the first
        if slope == 9.0:   # every wave rescales at every tile, and most rows trip it themselves
            assert fired.all()
            assert own.float().mean().item() >= 0.8
        elif slope == 5.0:  # every second tile: the excess builds up under the threshold first
            n = fired.sum(-1)
            assert ((n >= nfull // 2 - 1) & (n <= nfull // 2)).all(), n.unique()
            assert not (fired[..., 1:] & fired[..., :-1]).any()
            assert own.float().mean().item() >= 0.4 * 0.8
        else:
            assert not fired.any()
        if slope < 0:     # the later tiles underflow: their weights are below fp16's smallest subnormal
            s = _log2_logits(q, k, nimg, Nq, Nk, heads)
            assert (s[..., 4 * ac.KB:].amax(-1) - s.amax(-1)).max().item() < -25


def _log2_logits(q, k, nimg, Nq, Nk, heads):
    qh = ac._split(ac._prescaled_q(q, heads, None).double(), nimg, Nq, heads)
    return qh @ ac._split(k.double(), nimg, Nk, heads).transpose(-1, -2)


@pytest.mark.parametrize("d", ac.ALL_DIMS)
def test_staircase_moves_then_stays(d):
    q, k, v, nimg, Nq, Nk, heads = ac.staircase(d)
    own, fired = ac.rescale_rows(q, k, nimg, Nq, Nk, heads)
    assert own[..., 2].all() and own[..., 4].all()       # every row moves its maximum at tiles 2 and 4 ...
    assert not fired[..., [1, 3, 5, 6]].any()            # ... and at no other
    # tiles 4, 5 and 6 share the softmax: 64 : 64 : 16 keys at one level
    s = _log2_logits(q, k, nimg, Nq, Nk, heads)
    p = torch.softmax(s * 0.6931471805599453, dim=-1)
    w = torch.stack([p[..., t * ac.KB:(t + 1) * ac.KB].sum(-1) for t in range(7)], dim=-1).mean(dim=(0, 1, 2))
    assert w[:4].sum().item() < 1e-3 and 0.35 < w[4].item() < 0.55 and 0.35 < w[5].item() < 0.55
    # what an inconsistency of half an fp16 ulp of m = 24 (2^-7 log2 units) between tile 4 and tiles 5, 6 would do:
    # weigh tile 4 by 2^(2^-7) and compare with the bar's relative L2
    vh = ac._split(v.double(), nimg, Nk, heads)
    p2 = p.clone()
    p2[..., 4 * ac.KB:5 * ac.KB] *= 2.0 ** (2.0 ** -7)
    p2 = p2 / p2.sum(-1, keepdim=True)
    ref, off = p @ vh, p2 @ vh
    assert ((off - ref).norm() / ref.norm()).item() > 3 * 2e-3


@pytest.mark.parametrize("d", ac.ALL_DIMS)
def test_mixed_waves_one_row_triggers(d):
    for reverse in (False, True):
        q, k, v, nimg, Nq, Nk, heads = ac.mixed(d, reverse)
        own, fired = ac.rescale_rows(q, k, nimg, Nq, Nk, heads)
        nfull = Nk // ac.KB
        # (nearly) every 16-query fragment rescales at every full tile, on its one loud row's account when not reversed
        assert fired[..., 1:nfull].float().mean().item() >= 0.95
        trig = own[..., 1:nfull].float().mean(-1) >= 0.8  # trips (nearly) every one of them itself
        quiet = ~own.any(-1)              # never trips
        sel = (torch.arange(Nq) % 16) == 5
        loud_rows = ~sel if reverse else sel
        assert trig[..., loud_rows].float().mean().item() >= 0.95
        assert quiet[..., ~loud_rows].all()
        # the quiet rows' shifted scores are negative in every later tile: they pass the rescale with alpha = 1
        s = _log2_logits(q, k, nimg, Nq, Nk, heads)[..., ~loud_rows, :]
        assert (s[..., ac.KB:].amax(-1) < s[..., :ac.KB].amax(-1)).all()


@pytest.mark.parametrize("d", ac.ALL_DIMS)
def test_spike_is_the_row_maximum_at_the_intended_key(d):
    for cid, fn, (Nk, start) in ac.families()["last_key_spike"]:
        q, k, v, nimg, Nq, Nk, heads = fn(d, Nk, start)
        key = ac.KB * ((Nk - 1) // ac.KB) if start else Nk - 1
        s = _log2_logits(q, k, nimg, Nq, Nk, heads)
        for b, h, r in ac.spiked_rows(Nq, heads):
            assert s[b, h, r].argmax().item() == key
            if key >= ac.KB:  # past tile 0 the spike must trip the rescale
                assert s[b, h, r, key] - s[b, h, r, :ac.KB * (key // ac.KB)].max() > ac.RESCALE_THR


@pytest.mark.parametrize("d", ac.ALL_DIMS)
def test_key_offset_makes_the_maximum_large(d):
    for cid, fn, (Nq, Nk) in ac.families()["key_offset"]:
        q, k, v, nimg, Nq, Nk, heads = fn(d, Nq, Nk)
        m = _log2_logits(q, k, nimg, Nq, Nk, heads).amax(-1).abs()
        assert m.median().item() > 12 and m.max().item() > 40
        assert m.max().item() < 128  # log2 units (the few most extreme rows: logits of +-80)
