"""CPU tests of the neuron-level path's host side against the reference's own results (tests/golden/neuron_*.npz,
made by tests/golden/make_neuron_golden.py from the reference's receivers and statistics classes).

Everything here is a deterministic function of stored data, so every comparison is bit-exact: the fp16 running
statistics (sdmoe.discovery.StatMeter / StandardDev / Average), the saved JSON, the t-test and AP selections, the mask
files RemoveNeurons reads, the bit packing, and tests/neuron_ref.py (the checker of the GPU tests) against the
reference's hook outputs.
"""
import json
import os

import numpy as np
import pytest
import torch

import neuron_ref as R
from sdmoe import discovery, ops

PRED = R.golden("neuron_pred")
PRED_BB = R.golden("neuron_pred_bb")
REMOVE = R.golden("remove_neurons")
TTEST = R.golden("neuron_ttest")


def same(a, b):
    """Bit-for-bit equality of two arrays of one dtype (NaNs of equal payload included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fixtures_present():
    assert len(PRED) == 3 and len(PRED_BB) == 3 and len(REMOVE) == 4 and len(TTEST) == 1
    assert any(float(c["gate_bias"]) < 0 and (c["max_gate_base"] < 0).any() for _, c in PRED)
    for _, c in PRED + PRED_BB + REMOVE + TTEST:
        assert "kind" in c and "dtype" in c


def feed(rows, T, L):
    meter = discovery.StatMeter(T, L)
    for p in range(rows.shape[0]):
        for t in range(T):
            for l in range(L):
                meter.update(rows[p, t, l], t, l)
    return meter


def meter_state(meter, T, L):
    cells = meter.results["time_steps"]
    return (np.stack([np.stack([cells[t][l]["avg"].sum for l in range(L)]) for t in range(T)]),
            np.stack([np.stack([cells[t][l]["std"].mean for l in range(L)]) for t in range(T)]),
            np.stack([np.stack([cells[t][l]["std"].M2 for l in range(L)]) for t in range(T)]))


@pytest.mark.parametrize("name,c", PRED + PRED_BB, ids=[n for n, _ in PRED + PRED_BB])
def test_stat_meter_reproduces_reference_state(name, c, tmp_path):
    T, L = int(c["T"]), int(c["L"])
    for side in ("base", "adj"):
        if f"max_gate_{side}" not in c:
            continue
        rows = c[f"max_gate_{side}"]
        assert rows.dtype == np.float16
        meter = feed(rows, T, L)
        s, mean, m2 = meter_state(meter, T, L)
        assert same(s, c[f"sum_{side}"]) and same(mean, c[f"mean_{side}"]) and same(m2, c[f"M2_{side}"])
        assert meter.results["time_steps"][0][0]["std"].n == int(c[f"n_{side}"]) == rows.shape[0]
        if f"json_{side}" in c:
            path = tmp_path / f"{side}.json"
            meter.save(str(path))
            assert path.read_bytes() == c[f"json_{side}"].tobytes()
            again = tmp_path / f"{side}_again.json"
            meter.save(str(again))  # saving does not consume the meter
            assert again.read_bytes() == path.read_bytes()


@pytest.mark.parametrize("name,c", PRED, ids=[n for n, _ in PRED])
def test_paired_standard_dev_reproduces_reference(name, c):
    T, L = int(c["T"]), int(c["L"])
    for t in range(T):
        for l in range(L):
            sd = discovery.StandardDev()
            assert np.isnan(sd.stddev())
            for p in range(int(c["P"])):
                sd.update(c["max_gate_base"][p, t, l] - c["max_gate_adj"][p, t, l])
            assert same(sd.mean, c["diff_mean"][t, l]) and same(sd.M2, c["diff_M2"][t, l])
            assert same(sd.stddev(), c["diff_std"][t, l]) and sd.n == int(c["P"])


def test_average_and_standard_dev_on_scalars():
    a, s = discovery.Average(), discovery.StandardDev()
    for v in (1.0, 2.0, 4.0):
        a.update(v)
        s.update(v)
    assert a.sum == 7.0 and a.count == 3 and a.avg == 7.0 / 3
    assert s.n == 3 and abs(s.mean - 7.0 / 3) < 1e-15 and abs(s.variance() - 7.0 / 3) < 1e-12


def test_t_test_and_ap_selection_reproduce_reference():
    _, g = TTEST[0]
    c = dict(PRED)[str(g["source"])]
    T, L, P = int(g["T"]), int(g["L"]), int(g["P"])
    base = json.loads(c["json_base"].tobytes())["time_steps"]
    adj = json.loads(c["json_adj"].tobytes())["time_steps"]
    for t in range(T):
        for l in range(L):
            for ci, crit in enumerate(g["criticals"]):
                tv, sk = discovery.t_test_neurons(base[str(t)][str(l)]["avg"], adj[str(t)][str(l)]["avg"],
                                                  c["diff_std"][t, l].tolist(), P, float(crit))
                assert same(tv, g["t_value"][t, l]) and same(sk, g["skilled"][t, l, ci])
    assert g["skilled"].any() and not g["skilled"].all()
    mask = discovery.ap_neurons(g["hit_rate"], float(g["ap_ratio"]))
    assert same(mask, g["ap_mask"]) and mask.sum() == int(float(g["ap_ratio"]) * mask.size)


def test_save_neuron_masks_round_trips_through_remove_neurons(tmp_path):
    """The constructor reads the files and needs no device; from_masks takes the same masks in memory."""
    from neuron_receivers import GEGLU, RemoveNeurons
    rng = np.random.default_rng(0)
    T, L, Fn = 2, 3, 64
    masks = {t: {l: (rng.random(Fn) < 0.3) for l in range(L)} for t in range(T)}
    masks[1][1] = np.zeros(0, bool)
    discovery.save_neuron_masks(masks, str(tmp_path / "m"))
    with open(tmp_path / "m" / "predictivity_0_2.json") as f:
        raw = json.load(f)
    assert raw == [1.0 if v else 0.0 for v in masks[0][2]] and all(isinstance(v, float) for v in raw)
    with open(tmp_path / "m" / "predictivity_1_1.json") as f:
        assert json.load(f) == []
    rec = RemoveNeurons(0, str(tmp_path / "m"), T, L, remove_timesteps=20, weights_shape=None)
    mem = RemoveNeurons.from_masks(0, masks, T, L, store_gates=False)
    for r in (rec, mem):
        assert r.replace_fn is GEGLU and (r.timestep, r.layer) == (0, 0)
        for t in range(T):
            for l in range(L):
                assert np.array_equal(r.expert_indices[t][l], masks[t][l])
    assert rec.remove_timesteps == 20 and mem.store_gates is False and rec._bits == {}


def test_neuron_bits_packing():
    rng = np.random.default_rng(1)
    for Fn in (32, 1280, 5120):
        m = (rng.random(Fn) < 0.2).astype(np.float64)
        got = ops.neuron_bits(m.tolist(), "cpu")
        assert got.dtype == torch.int32 and tuple(got.shape) == (Fn // 32,)
        assert np.array_equal(got.numpy(), np.packbits(m.astype(bool), bitorder="little").view(np.int32))
    one = np.zeros(64)
    one[63] = 1
    assert ops.neuron_bits(one, "cpu").tolist() == [0, -(1 << 31)]
    with pytest.raises(ValueError):
        ops.neuron_bits(np.zeros(40), "cpu")
    pb = ops.position_bits([0, 3, 5, 17, 31, 99], 100, "cpu")
    want = np.zeros(128, bool)
    want[[0, 3, 5, 17, 31, 99]] = True
    assert np.array_equal(pb.numpy(), np.packbits(want, bitorder="little").view(np.int32))
    with pytest.raises(ValueError):
        ops.position_bits([100], 100, "cpu")


def test_abi_argument_validation_without_gpu():
    from sdmoe import _lib
    lib = _lib.load()

    def call(ldy, M, F, rpi, colmax, ws, ws_floats):
        return lib.sdmoe_geglu_neurons(16, ldy, M, F, 2, None, 0.0, 16, F, None, 0, rpi, None, 1, None, colmax, ws,
                                       ws_floats, None)

    assert call(656, 64, 328, 0, None, None, 0) == -2       # F % 32
    assert call(644, 64, 320, 0, None, None, 0) == -2       # ldy % 8
    assert call(640, 100, 320, 64, None, None, 0) == -1     # M % rows_per_img
    assert call(640, 128, 320, 64, 16, 16, 10) == -2        # workspace too small for the partial maxima
    assert call(640, 128, 320, 64, 16, None, 0) == -1
    assert lib.sdmoe_geglu_neurons(None, 640, 64, 320, 2, None, 0.0, 16, 320, None, 0, 0, None, 1, None, None, None,
                                   0, None) == -1
    assert call(640, 0, 320, 0, None, None, 0) == 0         # nothing to do


@pytest.mark.parametrize("name,c", PRED + PRED_BB, ids=[n for n, _ in PRED + PRED_BB])
def test_neuron_ref_reproduces_predictivity_goldens(name, c):
    """Every per-prompt maximum of the fixture and the first call's output, bit for bit in fp16."""
    T, L, act = int(c["T"]), int(c["L"]), str(c["act"])
    nmod = 2
    ws = [R.weights(c, l) for l in range(nmod)]
    bb = None
    if "bb" in c and not bool(c["bb_none"]):
        bb = c["bb"].tolist()
    for side, kind in (("base", 0), ("adj", 1)):
        if f"max_gate_{side}" not in c:
            continue
        for p in range(int(c["P"])):
            for call in range(T * L):
                x = R.tokens(c, p, kind, call)
                out, mx = R.pred_hook(x, *ws[call % nmod], act, bb=bb)
                assert same(mx.numpy(), c[f"max_gate_{side}"][p, call // L, call % L])
                if (p, kind, call) == (0, 0, 0):
                    assert same(out.numpy(), c["out0"])


@pytest.mark.parametrize("name,c", REMOVE, ids=[n for n, _ in REMOVE])
def test_neuron_ref_reproduces_remove_neurons_goldens(name, c):
    L, act, Fn = int(c["L"]), str(c["act"]), 4 * int(c["C"])
    ws = [R.weights(c, l) for l in range(L)]
    kinds = set()
    for i, call in enumerate(c["calls"].tolist()):
        t, l = c["call_tl"][i].tolist()
        assert (t, l) == (call // L, call % L)
        mask = np.zeros(0) if c["mask_empty"][t, l] else np.unpackbits(c["mask_bits"][t, l], count=Fn,
                                                                      bitorder="little")
        kinds.add("empty" if mask.size == 0 else "last" if mask.sum() == 1 and mask[-1] else "random")
        out, gate = R.remove_hook(R.tokens(c, 0, 0, call), *ws[l], act, mask)
        assert same(out.numpy(), c["out"][i]) and same(gate.numpy(), c["gate"][i])
        if mask.size:
            on = np.flatnonzero(mask)
            assert np.all(c["gate"][i][..., on] == np.float16(-0.17)) and np.float16(-0.17) == -0.1700439453125
    assert {"last", "random"} <= kinds


def test_out_of_range_box_falls_back_to_all_tokens():
    _, c = PRED_BB[0]
    x, (w, b) = R.tokens(c, 0, 0, 0), R.weights(c, 0)
    full = R.pred_hook(x, w, b, "gelu")[1]
    assert torch.equal(R.pred_hook(x, w, b, "gelu", bb=[0, 3, 40])[1], full)
    assert torch.equal(R.pred_hook(x, w, b, "gelu", bb=[])[1], full)
    assert not torch.equal(R.pred_hook(x, w, b, "gelu", bb=[0, 3, 5])[1], full)


def test_receivers_construct_and_count_without_a_gpu():
    from neuron_receivers import GELU, NeuronPredictivity, NeuronPredictivityBB
    for cls in (NeuronPredictivity, NeuronPredictivityBB):
        r = cls(0, 51, 16)
        assert r._predictivity is None and r._max_gate is None  # nothing built until the statistics are used
        for i in range(16 * 51):
            assert (r.timestep, r.layer) == (i // 16, i % 16)
            r.update_time_layer()
        assert r.max_gate[50][15] == [] and len(r.max_gate) == 51
        r.max_gate[0][0] = np.zeros(4, np.float16)
        r.reset_time_layer()
        assert (r.timestep, r.layer) == (0, 0) and r.max_gate[0][0] == []
        assert isinstance(r.predictivity, discovery.StatMeter) and r.predictivity.T == 51
    r = NeuronPredictivityBB(0, 2, 70)  # the counter wraps at n_layers - 1, not at a hard-coded 15
    for _ in range(70):
        r.update_time_layer()
    assert (r.timestep, r.layer) == (1, 0)
    with pytest.raises(NotImplementedError, match="GELU"):
        NeuronPredictivity(0, 1, 1, replace_fn=GELU).hook_fn(None, (None,), None)


def test_prompt_image_table():
    from neuron_receivers import NeuronPredictivity
    from sdmoe._lib import SdmoeError
    r = NeuronPredictivity(0, 1, 1)
    r.set_prompts(["a", "b", "c"])
    assert r.image_table(3) == [0, 1, 2] and r.image_table(6) == [0, 1, 2, 0, 1, 2]
    with pytest.raises(SdmoeError):
        r.image_table(4)
    r.set_prompts("one prompt")
    assert r._nprompts is None
