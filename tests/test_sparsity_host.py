"""CPU tests of the gate-sparsity measurement's host side against the reference's own results
(tests/golden/sparsity_*.npz, made by tests/golden/make_sparsity_golden.py from the reference's SparsityMeasure and
StatMeter).

The integer counts carry no tolerance. The zero ratio does: the port reports zeros / elements exactly (float64), the
reference the fp32 mean over the tokens of fp32 row ratios; each row ratio is rounded to fp32 (relative 2^-24) and the
blocked fp32 mean over M <= 65536 rows adds about (log2 M + 2) * 2^-24 ~ 1.1e-6 relative on values <= 1, hence 1e-6
(absolute, ratios are <= 1; the fixtures have M = 64 rows).
"""
import json

import numpy as np
import pytest
import torch

import sparsity_ref as R
from sdmoe import discovery

SPARSITY = R.golden("sparsity")
RATIO_TOL = 1e-6


def fake_calls(zeros, negatives, elements, rows=None, neuron_zeros=None):
    out = []
    for i in range(len(zeros)):
        rec = {"zeros": np.asarray(zeros[i], np.int64), "negatives": np.asarray(negatives[i], np.int64),
               "elements": np.asarray(elements[i], np.int64)}
        if rows is not None:
            rec["rows"] = np.asarray(rows[i], np.int64)
        if neuron_zeros is not None:
            rec["neuron_zeros"] = np.asarray(neuron_zeros[i], np.int32)
        out.append(rec)
    return out


def test_fixtures_present():
    assert len(SPARSITY) == 3
    by = {(str(c["act"]), float(c["gate_bias"])): c for _, c in SPARSITY}
    relu, gelu, deep = by[("relu", 0.0)], by[("gelu", 0.0)], by[("gelu", -3.0)]
    assert (relu["negatives"] == 0).all() and (relu["ratio_ref"] > 0.3).all() and (relu["ratio_ref"] < 0.7).all()
    assert (gelu["negatives"] > 0).all()
    assert (deep["zeros"] > 0).any()
    for _, c in SPARSITY:
        assert c["zeros"].shape == (int(c["P"]), int(c["T"]) * int(c["L"])) and "gate" not in c


@pytest.mark.parametrize("name,c", SPARSITY, ids=[n for n, _ in SPARSITY])
def test_sparsity_ref_reproduces_goldens(name, c):
    """Every integer count exactly; the reference's ratio bit for bit with its fp32 formula; the first output."""
    T, L, act = int(c["T"]), int(c["L"]), str(c["act"])
    ws = [R.weights(c, l) for l in range(L)]
    for p in range(int(c["P"])):
        for call in range(T * L):
            out, gate, _ = R.hook(R.tokens(c, p, 0, call), *ws[call % L], act)
            assert gate.numel() == int(c["elements"])
            assert R.counts(gate) == (int(c["zeros"][p, call]), int(c["negatives"][p, call]))
            assert R.ratio_fp32(gate) == float(c["ratio_ref"][p, call])
            if (p, call) == (0, 0):
                assert out.numpy().tobytes() == c["out0"].tobytes()


@pytest.mark.parametrize("name,c", SPARSITY, ids=[n for n, _ in SPARSITY])
def test_sparsity_ratios_agree_with_reference_ratio(name, c):
    P, n = c["zeros"].shape
    for p in range(P):
        calls = fake_calls(c["zeros"][p][:, None], c["negatives"][p][:, None], np.full((n, 1), int(c["elements"])))
        got = discovery.sparsity_ratios(calls)
        assert got.dtype == np.float64 and got.shape == (n, 1)
        assert np.abs(got[:, 0] - c["ratio_ref"][p]).max() <= RATIO_TOL
        assert np.array_equal(got[:, 0], c["zeros"][p] / float(c["elements"]))


@pytest.mark.parametrize("name,c", SPARSITY, ids=[n for n, _ in SPARSITY])
def test_accumulate_sparsity_writes_the_reference_json(name, c, tmp_path):
    """Fed prompt by prompt (the reference's loop) and as one batch of P prompts: the same JSON shape, every avg and
    std within the ratio tolerance of the reference's file."""
    T, L = int(c["T"]), int(c["L"])
    P, n = c["zeros"].shape
    want = json.loads(c["json"].tobytes())
    one = discovery.StatMeter(T, L)
    for p in range(P):
        calls = fake_calls(c["zeros"][p][:, None], c["negatives"][p][:, None], np.full((n, 1), int(c["elements"])))
        assert discovery.accumulate_sparsity(one, discovery.sparsity_ratios(calls), L) is one
    batch = discovery.StatMeter(T, L)
    calls = fake_calls(c["zeros"].T, c["negatives"].T, np.full((n, P), int(c["elements"])))
    discovery.accumulate_sparsity(batch, discovery.sparsity_ratios(calls), L)
    for tag, meter in (("one", one), ("batch", batch)):
        path = tmp_path / f"sparsity_{tag}.json"
        meter.save(str(path))
        got = json.loads(path.read_text())
        assert list(got) == list(want) == ["time_steps"]
        assert list(got["time_steps"]) == list(want["time_steps"]) == [str(t) for t in range(T)]
        for t in want["time_steps"]:
            assert list(got["time_steps"][t]) == list(want["time_steps"][t]) == [str(l) for l in range(L)]
            for l in want["time_steps"][t]:
                g, w = got["time_steps"][t][l], want["time_steps"][t][l]
                assert list(g) == list(w) == ["avg", "std"]
                assert isinstance(g["avg"], float) and isinstance(g["std"], float)
                assert abs(g["avg"] - w["avg"]) <= RATIO_TOL and abs(g["std"] - w["std"]) <= RATIO_TOL
        assert meter.results["time_steps"][T - 1][L - 1]["std"].n == P


def test_accumulate_sparsity_cell_order():
    meter = discovery.StatMeter(2, 3)
    discovery.accumulate_sparsity(meter, [0.0, 0.1, 0.2, 0.3, 0.4, 0.5], 3)  # one prompt: a 1-D list of ratios
    cells = meter.results["time_steps"]
    assert [[cells[t][l]["avg"].avg for l in range(3)] for t in range(2)] == [[0.0, 0.1, 0.2], [0.3, 0.4, 0.5]]
    assert discovery.sparsity_ratios([]).shape == (0, 0)


def test_neuron_zero_fraction_on_a_hand_made_input():
    nz = [[[0, 4, 8, 2]], [[8, 8, 0, 1]], [[1, 2, 3, 4], [6, 0, 6, 3]]]
    rows = [[8], [8], [4, 6]]
    calls = fake_calls([[14], [17], [10, 15]], [[0], [0], [0, 0]], [[32], [32], [16, 24]], rows=rows, neuron_zeros=nz)
    got = discovery.neuron_zero_fraction(calls, 2)
    assert sorted(got) == [0, 1] and sorted(got[0]) == [0, 1] and sorted(got[1]) == [0]
    assert got[0][0].dtype == np.float64
    assert np.array_equal(got[0][0], [[0.0, 0.5, 1.0, 0.25]])
    assert np.array_equal(got[0][1], [[1.0, 1.0, 0.0, 0.125]])
    assert np.array_equal(got[1][0], [[0.25, 0.5, 0.75, 1.0], [1.0, 0.0, 1.0, 0.5]])
    with pytest.raises(ValueError, match="per_neuron"):
        discovery.neuron_zero_fraction(fake_calls([[1]], [[0]], [[4]]), 1)


def test_receiver_constructs_and_checks_counts_without_a_gpu():
    from neuron_receivers import GEGLU, GELU, BaseNeuronReceiver, SparsityMeasure
    from sdmoe._lib import SdmoeError
    rec = SparsityMeasure(3)
    assert isinstance(rec, BaseNeuronReceiver) and rec.seed == 3 and rec.replace_fn is GEGLU
    assert rec.threshold == 0.0 and rec.per_neuron is False and rec.store_gates is True
    assert rec.calls == [] and rec._pending == [] and rec.flush_count == 0
    rec.flush()  # nothing pending: no copy
    assert rec.flush_count == 0
    rec = SparsityMeasure(0, threshold=0.05, per_neuron=True, store_gates=False)
    assert rec.threshold == 0.05 and rec.per_neuron and not rec.store_gates
    with pytest.raises(ValueError):
        SparsityMeasure(0, threshold=-1.0)
    # test()'s condition on fake call records
    rec.calls = fake_calls([[5], [7]], [[0], [0]], [[16], [16]])
    rec.check_no_negatives()
    rec.calls = fake_calls([[5, 1], [7, 2]], [[0, 0], [0, 3]], [[16, 16], [16, 16]])
    with pytest.raises(AssertionError, match="Relu failed"):
        rec.check_no_negatives()
    # prompt groups: the table NeuronPredictivity uses
    rec.set_prompts(["a", "b", "c"])
    assert rec.image_table(6) == [0, 1, 2, 0, 1, 2]
    with pytest.raises(SdmoeError):
        rec.image_table(4)
    with pytest.raises(SdmoeError):
        rec.groups_of(torch.zeros(4, 8, 16))
    rec.set_prompts("one prompt")
    assert rec.groups_of(torch.zeros(4, 8, 16)) == (4, 1, None)
    with pytest.raises(NotImplementedError, match="GELU"):
        SparsityMeasure(0, replace_fn=GELU).hook_fn(None, (None,), None)


def test_abi_argument_validation_without_gpu():
    """Every refusal of sdmoe_geglu_sparsity comes before its first launch (fake pointers, no device)."""
    from sdmoe import _lib
    lib = _lib.load()

    def call(ldy, M, F, rpi, thr=0.0, cz=16, cn=16, tot=16, ws=16, ws_floats=1 << 20, y=16):
        return lib.sdmoe_geglu_sparsity(y, ldy, M, F, 3, thr, 16, F, None, 0, rpi, None, 1, cz, cn, tot, ws, ws_floats,
                                        None)

    assert call(656, 64, 328, 0) == -2                      # F % 32
    assert call(644, 64, 320, 0) == -2                      # ldy % 8
    assert call(640, 100, 320, 64) == -1                    # M % rows_per_img
    assert call(640, 128, 320, 64, thr=-0.5) == -1          # negative threshold
    assert call(640, 128, 320, 64, thr=float("nan")) == -1
    assert call(640, 128, 320, 64, cz=None, tot=None) == -1     # neither totals nor both arrays
    assert call(640, 128, 320, 64, ws_floats=2 * 320 - 1) == -2  # 2 images x 1 slab x F words
    assert call(640, 128, 320, 64, ws=None) == -1
    assert call(640, 128, 320, 64, tot=12) == -2            # int64 totals at a 4-byte address
    assert call(640, 64, 320, 0, y=None) == -1
    assert call(640, 0, 320, 0, y=None) == 0                # nothing to do
