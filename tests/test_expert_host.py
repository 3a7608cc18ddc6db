"""CPU tests of the expert-level discovery path's host side against the reference's own results
(tests/golden/expert_*.npz, made by tests/golden/make_expert_golden.py from the reference's receivers, statistics classes
and accumulate loop).

Everything here is a deterministic function of stored data, so every comparison is exact: the expert t-test lists, the
expert counter and its JSON, the list files RemoveExperts reads, the counters of the two new receivers, FrequencyMeasure's
flush arithmetic, and tests/expert_ref.py (the checker of the GPU tests) against the reference's hook outputs.
"""
import json
import os

import numpy as np
import pytest
import torch

import expert_ref as R
from sdmoe import discovery, mask_io

PRED = R.golden("expert_pred")
FREQ = R.golden("expert_freq")
TTEST = R.golden("expert_ttest")
COUNTER = R.golden("expert_counter")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fixtures_present():
    assert len(PRED) == 4 and len(FREQ) == 4 and len(TTEST) == 1 and len(COUNTER) == 1
    assert sorted((int(c["C"]), str(c["act"]), float(c["gate_bias"])) for _, c in PRED) == [
        (320, "gelu", -3.0), (320, "gelu", 0.0), (320, "relu", 0.0), (1280, "gelu", 0.0)]
    assert sorted((int(c["C"]), str(c["act"])) for _, c in FREQ) == [
        (320, "gelu"), (320, "relu"), (640, "relu"), (1280, "gelu")]
    neg = [c for _, c in PRED if float(c["gate_bias"]) < 0][0]
    assert (neg["max_gate_base"] < 0).any() and (neg["max_gate_adj"] < 0).any()
    for _, c in FREQ:
        # at most 5 % of the image-0 rows of every hooked call sit near a top-k tie
        assert (c["n_near"] <= 0.05 * int(c["N"])).all() and float(c["topk"]) == 0.2
        assert int(c["N"]) & (int(c["N"]) - 1) == 0


def test_import_exposes_both_receivers():
    import neuron_receivers
    from neuron_receivers import ExpertPredictivity, FrequencyMeasure
    assert neuron_receivers.ExpertPredictivity is ExpertPredictivity
    assert neuron_receivers.FrequencyMeasure is FrequencyMeasure
    assert issubclass(ExpertPredictivity, neuron_receivers.NeuronPredictivity)


# ------------------------------------------------------------------------------------------------ t-test
def statistics_of(c):
    T, L = int(c["T"]), int(c["L"])
    base = json.loads(c["json_base"].tobytes())
    adj = json.loads(c["json_adj"].tobytes())
    diff = json.loads(json.dumps({t: {l: c["diff_std"][t][l].tolist() for l in range(L)} for t in range(T)}))
    return base, adj, diff


def test_expert_t_test_matches_reference(tmp_path):
    _, tt = TTEST[0]
    src = dict(PRED)[str(tt["source"])]
    T, L, P, E, crit = int(tt["T"]), int(tt["L"]), int(tt["P"]), int(tt["E"]), float(tt["critical"])
    want = {tuple(map(int, k.split(","))): v for k, v in json.loads(str(tt["lists"])).items()}
    sizes = [len(v) for v in want.values()]
    assert any(sizes) and max(sizes) < E
    finite = tt["t_value"][np.isfinite(tt["t_value"])]
    assert np.all(np.abs(finite + crit) > 1e-6)
    base, adj, diff = statistics_of(src)
    for (t, l), ids in want.items():
        cell_b, cell_a = base["time_steps"][str(t)][str(l)], adj["time_steps"][str(t)][str(l)]
        got = discovery.t_test_experts(cell_b["avg"], cell_a["avg"], diff[str(t)][str(l)], P, crit)
        assert got == ids and got == sorted(got) and all(type(e) is int for e in got)
        tv, _ = discovery.t_test_neurons(cell_b["avg"], cell_a["avg"], diff[str(t)][str(l)], P, crit)
        assert same(tv, tt["t_value"][t, l])
    lists = discovery.expert_lists_from_statistics(base, adj, diff, P, crit)
    assert lists == {t: {l: want[(t, l)] for l in range(L)} for t in range(T)}
    # the same from the files the analysis script writes
    paths = []
    for name, obj in (("predictivity_base_expert.json", base), ("predictivity_adj_expert.json", adj),
                      ("diff_std_expert.json", diff)):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w") as f:
            json.dump(obj, f)
    assert discovery.expert_lists_from_statistics(*paths, P, crit) == lists
    # the default critical value is the reference's 3.579
    strict = discovery.expert_lists_from_statistics(base, adj, diff, P)
    assert strict == discovery.expert_lists_from_statistics(base, adj, diff, P, 3.579)


def test_expert_lists_feed_remove_experts(tmp_path):
    from neuron_receivers import RemoveExperts
    _, tt = TTEST[0]
    src = dict(PRED)[str(tt["source"])]
    T, L, P = int(tt["T"]), int(tt["L"]), int(tt["P"])
    lists = discovery.expert_lists_from_statistics(*statistics_of(src), P, float(tt["critical"]))
    discovery.save_expert_lists(lists, str(tmp_path / "skilled"))
    for t in range(T):
        for l in range(L):
            path = tmp_path / "skilled" / f"timestep_{t}_layer_{l}.json"
            assert mask_io.load_expert_list(str(path)) == lists[t][l]
    rec = RemoveExperts(0, str(tmp_path / "skilled"), T, L)
    assert rec.expert_indices == lists


def test_stat_meter_from_in_memory_statistics():
    """expert_lists_from_statistics also takes StatMeter.to_json() (int keys) without a round trip through a file."""
    _, c = PRED[1]
    T, L, P = int(c["T"]), int(c["L"]), int(c["P"])
    meters = []
    for side in ("base", "adj"):
        m = discovery.StatMeter(T, L)
        for p in range(P):
            for t in range(T):
                for l in range(L):
                    m.update(c[f"max_gate_{side}"][p, t, l], t, l)
        meters.append(m)
        sums = np.stack([np.stack([m.results["time_steps"][t][l]["avg"].sum for l in range(L)]) for t in range(T)])
        assert same(sums, c[f"sum_{side}"])
    diff = {t: {l: discovery.StandardDev() for l in range(L)} for t in range(T)}
    for p in range(P):
        for t in range(T):
            for l in range(L):
                diff[t][l].update(c["max_gate_base"][p, t, l] - c["max_gate_adj"][p, t, l])
    dstd = {t: {l: diff[t][l].stddev().tolist() for l in range(L)} for t in range(T)}
    assert same(np.array([[dstd[t][l] for l in range(L)] for t in range(T)], dtype=np.float16), c["diff_std"])
    got = discovery.expert_lists_from_statistics(meters[0].to_json(), meters[1].to_json(), dstd, P, 1.0)
    want = discovery.expert_lists_from_statistics(*statistics_of(c), P, 1.0)
    assert got == want


# ------------------------------------------------------------------------------------------------ expert counter
def test_expert_counter_matches_reference(tmp_path):
    _, c = COUNTER[0]
    T, num = int(c["T"]), int(c["num_images"])
    names = [str(n) for n in c["names"]]
    counter = None
    for s in range(num):
        lc = {t: {0: c["lc_l0"][s, t], 1: c["lc_l1"][s, t]} for t in range(T)}
        counter = discovery.accumulate_expert_counter(counter, lc, names, num)
    for t in range(T):
        assert same(np.array(counter[t][names[0]], dtype=np.float64), c["ec_l0"][t])
        assert same(np.array(counter[t][names[1]], dtype=np.float64), c["ec_l1"][t])
    ref = json.loads(c["json"].tobytes())
    path = discovery.save_expert_counter(counter, str(tmp_path), float(c["topk"]))
    assert os.path.basename(path) == "expert_counter_0.2.json"
    with open(path) as f:
        saved = json.load(f)
    assert saved == ref and list(saved) == list(ref) and all(list(saved[t]) == list(ref[t]) for t in ref)
    # an explicit start dict (the reference's [0] * E lists) gives the same
    start = {t: {n: [0] * len(counter[t][n]) for n in names} for t in range(T)}
    again = start
    for s in range(num):
        lc = {t: {0: c["lc_l0"][s, t], 1: c["lc_l1"][s, t]} for t in range(T)}
        again = discovery.accumulate_expert_counter(again, lc, names, num)
    assert again is start and again == counter


# ------------------------------------------------------------------------------------------------ receivers, host side
@pytest.mark.parametrize("n_layers", [2, 16, 70])
def test_counters_wrap_at_n_layers(n_layers):
    from neuron_receivers import ExpertPredictivity, FrequencyMeasure
    names = [f"ffn{l}" for l in range(n_layers)]
    recs = [ExpertPredictivity(0, 3, n_layers), FrequencyMeasure(0, 3, n_layers, {n: 8 for n in names}, names)]
    for rec in recs:
        seen = []
        for _ in range(2 * n_layers + 1):
            seen.append((rec.timestep, rec.layer))
            rec.update_time_layer()
        assert seen == [(i // n_layers, i % n_layers) for i in range(2 * n_layers + 1)]
        rec.reset_time_layer()
        assert (rec.timestep, rec.layer) == (0, 0)


def test_constructor_defects_fixed():
    """The reference's ExpertPredictivity takes no replace_fn (its caller passes one) and hands keep_nsfw to the base
    class's replace_fn slot."""
    from neuron_receivers import GEGLU, ExpertPredictivity, FrequencyMeasure
    rec = ExpertPredictivity(3, 2, 2, replace_fn=GEGLU, keep_nsfw=True)
    assert rec.replace_fn is GEGLU and rec.keep_nsfw is True and rec.seed == 3
    rec = ExpertPredictivity(3, 2, 2, keep_nsfw=True)
    assert rec.replace_fn is GEGLU and rec.keep_nsfw is True
    with pytest.raises(ValueError):
        FrequencyMeasure(0, 1, 1, {"a": 4}, ["a"], images="last")


def test_expert_predictivity_reset_semantics():
    """reset_time_layer() only resets the counter (max_gate survives and is overwritten call by call); reset() empties
    max_gate."""
    from neuron_receivers import ExpertPredictivity
    rec = ExpertPredictivity(0, 1, 2)
    rec._pending = [(0, 0, torch.tensor([[1.0, -2.0]], dtype=torch.float16)),
                    (0, 1, torch.tensor([[3.0, 4.0]], dtype=torch.float16))]
    rec.timestep, rec.layer = 1, 0
    rec.flush()
    assert rec.flush_count == 1 and same(rec.max_gate[0][0], np.array([1.0, -2.0], dtype=np.float16))
    rec.reset_time_layer()
    assert (rec.timestep, rec.layer) == (0, 0) and same(rec.max_gate[0][1], np.array([3.0, 4.0], dtype=np.float16))
    assert rec.predictivity.results["time_steps"][0][1]["std"].n == 1
    rec.reset()
    assert rec.max_gate[0][0] == [] and rec.max_gate[0][1] == [] and (rec.timestep, rec.layer) == (0, 0)
    rec.flush()
    assert rec.flush_count == 1  # nothing pending: no copy


def counts(rows):
    return torch.tensor(rows, dtype=torch.int32)


def test_frequency_measure_flush_arithmetic():
    from neuron_receivers import FrequencyMeasure
    names = ["a", "b"]
    rec = FrequencyMeasure(0, 1, 2, {"a": 3, "b": 3}, names)
    assert rec.label_counter[0][0].dtype == np.float64 and rec.images == "first" and rec.store_gates is False
    c0, c1 = [[4, 0, 8], [1, 2, 3]], [[7, 7, 2], [8, 0, 0]]
    rec._pending = [(0, 0, 8, counts(c0)), (0, 1, 8, counts(c1))]
    rec.flush()
    assert same(rec.label_counter[0][0], np.array([0.5, 0.0, 1.0])) and rec.flush_count == 1
    assert same(rec.label_counter[0][1], np.array([7, 7, 2]) / 8)
    rec._pending = [(0, 0, 8, counts(c0))]   # counters accumulate until reset()
    rec.flush()
    assert same(rec.label_counter[0][0], np.array([1.0, 0.0, 2.0])) and rec.flush_count == 2
    rec.reset()
    assert same(rec.label_counter[0][0], np.zeros(3)) and same(rec.label_counter[0][1], np.zeros(3))
    # every image of the prompt: summed, divided by n_images * seq_len
    rec = FrequencyMeasure(0, 1, 2, {"a": 3, "b": 3}, names, images="all")
    rec._pending = [(0, 0, 8, counts(c0))]
    rec.flush()
    assert same(rec.label_counter[0][0], np.array([5, 2, 11]) / 16.0)
    # a prompt list: B rows, image i belongs to prompt i % B
    four = [[1, 0, 0], [0, 2, 0], [0, 0, 4], [8, 8, 8]]
    for mode, want in (("first", np.array([[1, 0, 0], [0, 2, 0]]) / 8.0),
                       ("all", np.array([[1, 0, 4], [8, 10, 8]]) / 16.0)):
        rec = FrequencyMeasure(0, 1, 2, {"a": 3, "b": 3}, names, images=mode)
        rec.set_prompts(["one", "two"])
        rec._pending = [(0, 0, 8, counts(four))]
        rec.flush()
        assert same(rec.label_counter[0][0], want), mode
    # a sequence length that is no power of two: count * (1 / n) against n additions of 1 / n
    rec = FrequencyMeasure(0, 1, 2, {"a": 3, "b": 3}, names)
    rec._pending = [(0, 0, 100, counts([[100, 37, 0]]))]
    rec.flush()
    ref = np.zeros(3)
    for e, n in enumerate([100, 37, 0]):
        for _ in range(n):
            ref[e] += 1.0 / 100
    np.testing.assert_allclose(rec.label_counter[0][0], ref, rtol=1e-12, atol=0)


def test_abi_argument_validation_without_gpu():
    """Every refusal of sdmoe_expert_stats comes before its first launch (fake pointers, no device)."""
    from sdmoe import _lib
    lib = _lib.load()

    def call(ld, sel, M, E, rpi, colmax, count, ws, ws_floats, ngroups=1):
        return lib.sdmoe_expert_stats(16, ld, sel, M, E, rpi, None, ngroups, colmax, count, ws, ws_floats, None)

    assert call(64, None, 0, 64, 0, 16, None, None, 0) == 0         # M == 0: nothing to do
    assert call(64, None, 128, 64, 64, None, 16, 16, 1 << 20) == -1  # count without sel
    assert call(64, 16, 100, 64, 64, 16, 16, 16, 1 << 20) == -1      # M % rows_per_img
    assert call(257, None, 128, 257, 64, 16, None, 16, 1 << 20) == -2  # E > 256
    assert call(32, None, 128, 64, 64, 16, None, 16, 1 << 20) == -2  # ld_score < E
    assert call(64, None, 128, 64, 64, 16, None, 16, 1 << 20, ngroups=0) == -1
    assert call(64, None, 128, 64, 64, 16, None, None, 0) == -1      # no workspace
    cells = 2 * 4 * 64  # images * ceil(64 / 16) * E
    assert call(64, 16, 128, 64, 64, 16, 16, 16, cells + cells // 2 - 1) == -2
    assert call(64, 16, 128, 64, 64, None, 16, 16, cells - 1) == -2
    assert call(64, None, 128, 64, 64, 16, None, 16, cells // 2 - 1) == -2
    assert call(64, 16, 128, 64, 64, None, None, None, 0) == 0       # neither statistic asked for


# ------------------------------------------------------------------------------------------------ the CPU restatement
@pytest.mark.parametrize("name,c", PRED, ids=[n for n, _ in PRED])
def test_expert_ref_pred_hook_matches_reference(name, c):
    T, L, act, pat = int(c["T"]), int(c["L"]), str(c["act"]), R.patterns(c)
    ws = [R.weights(c, l) for l in range(L)]
    for p, kind, key in ((0, 0, "max_gate_base"), (2, 1, "max_gate_adj")):
        for call in range(T * L):
            out, mx = R.pred_hook(R.pred_tokens(c, p, kind, call), *ws[call % L], act, pat)
            assert same(mx.numpy(), c[key][p, call // L, call % L])
            if (p, kind, call) == (0, 0, 0):
                assert same(out.numpy(), c["out0"])


@pytest.mark.parametrize("name,c", FREQ, ids=[n for n, _ in FREQ])
def test_expert_ref_freq_hook_matches_reference(name, c):
    T, L, E, k, act, pat = int(c["T"]), int(c["L"]), int(c["E"]), int(c["k"]), str(c["act"]), R.patterns(c)
    ws = [R.weights(c, l) for l in range(L)]
    lc = np.zeros((T, L, E))
    for call, (t, l) in enumerate(c["call_tl"].tolist()):
        out, score = R.freq_hook(R.tokens(c, c["x_seeds"][call]), *ws[l], act, pat, k, lc[t, l])
        assert same(score[0].numpy(), c["score0"][call])
        if call == 0:
            assert same(out.numpy(), c["out0"])
    assert same(lc, c["label_counter"])
    # a power-of-two seq_len: the counts times 1 / seq_len are the repeated additions exactly
    N = int(c["N"])
    cnt = np.zeros((T, L, E))
    for call, (t, l) in enumerate(c["call_tl"].tolist()):
        np.add.at(cnt[t, l], c["labels0"][call].reshape(-1), 1.0)
    assert same(cnt * (1.0 / N), c["label_counter"])
