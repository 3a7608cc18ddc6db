"""CPU tests of AddExperts' host side against the reference's own hook (tests/golden/add_experts_*.npz, made by
tests/golden/make_add_experts_golden.py from the reference's AddExperts.hook_fn): tests/add_experts_ref.py reproduces
the fixtures' biased scores, indices, output and gate bit for bit; and the bias vector (ops.expert_bias) against the
reference's own torch expression, k' = int(k_fraction * k), the statistics-path derivation, the constructor's overrides, the export and the two new
library entry points. Everything here is a deterministic function of its inputs, so every comparison is exact.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import add_experts_ref as R
from sdmoe import _lib, ops


from test_gpu_route_parity import near_tie_rows  # noqa: E402  (the project's one definition; imports no GPU state)

GOLD = R.golden("add_experts")


def test_fixtures_present_and_within_the_near_tie_cap():
    assert sorted((int(c["C"]), int(c["N"]), str(c["act"]), int(c["E"]), int(c["k"]), int(c["kk"])) for _, c in GOLD) == [
        (320, 32, "gelu", 64, 12, 9), (320, 32, "relu", 64, 12, 9), (1280, 8, "gelu", 256, 51, 40)]
    near = near_tie_rows
    for _, c in GOLD:
        kk, T, L = int(c["kk"]), int(c["T"]), int(c["L"])
        assert T == L == 2 and kk == int(0.8 * int(c["k"]))
        lists = json.loads(str(c["lists"]))
        sizes = sorted(len(v) for v in lists.values())
        assert sizes[0] == 0 and sizes[1] == 1 and sizes[-1] > kk
        assert any(len(set(v)) < len(v) for v in lists.values())
        assert (c["std"] > 0).all()
        for call in range(T * L):
            nr = near(c["score"][call], kk, slack_ulps=8)
            assert int(nr.sum()) == int(c["n_near"][call]) and nr.sum() <= 0.05 * nr.size


@pytest.mark.parametrize("name,c", GOLD, ids=[n for n, _ in GOLD])
def test_restated_hook_reproduces_the_reference(name, c):
    C, E, k, kk, L = (int(c[n]) for n in ("C", "E", "k", "kk", "L"))
    lists = {tuple(map(int, key.split(","))): v for key, v in json.loads(str(c["lists"])).items()}
    pat = R.patterns(c)
    for call, (t, l) in enumerate(c["call_tl"]):
        ids, std = lists[(int(t), int(l))], c["std"][call].tolist()
        w, b = R.weights(c, int(l))
        out, gate, score, labels = R.add_hook(R.tokens(c, call), w, b, str(c["act"]), pat, k, ids, std)
        assert same(score, torch.from_numpy(c["score"][call]))
        assert np.array_equal(labels.numpy(), c["labels_topk"][call]) and labels.shape[1] == kk
        assert same(R.bias_vector(ids, std, E), torch.from_numpy(c["bias"][call]))
        assert same(ops.expert_bias(ids, std, E, "cpu"), torch.from_numpy(c["bias"][call]))
        if call == 0:
            assert same(out, torch.from_numpy(c["out0"])) and same(gate, torch.from_numpy(c["gate0"]))
            y = torch.nn.functional.linear(R.tokens(c, call), w, b).view(-1, 8 * C)
            o2, g2, s2, l2 = R.route_from_y(y, str(c["act"]), pat, k, ids, std)
            assert same(o2, out.view(-1, 4 * C)) and same(g2, gate.view(-1, 4 * C)) and same(s2, score)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_import_exposes_add_experts():
    import neuron_receivers
    from neuron_receivers import AddExperts
    assert neuron_receivers.AddExperts is AddExperts
    assert issubclass(AddExperts, neuron_receivers.NeuronPredictivity)
    assert AddExperts._sdmoe_ln_safe_hook is AddExperts.__dict__["hook_fn"]


def test_library_exports_both_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "sdmoe_score_bias") and hasattr(lib, "sdmoe_geglu_route_bias")
    assert len(_lib.SIGNATURES["sdmoe_score_bias"]) == 8
    assert len(_lib.SIGNATURES["sdmoe_geglu_route_bias"]) == len(_lib.SIGNATURES["sdmoe_geglu_route"]) + 1


def test_expert_bias_is_the_reference_expression():
    rng = np.random.default_rng(1)
    E = 64
    # values whose float64 -> float32 -> float16 double rounding matters, subnormal results, large ones
    std = [float(v) for v in rng.uniform(0, 3, E)]
    std[3], std[4], std[5], std[6] = 1.0 + 2.0 ** -11 + 2.0 ** -30, 1e-8, 13000.0, 0.1
    ids = [3, 4, 5, 6, 10, 63, 0]
    got = ops.expert_bias(ids, std, E, "cpu")
    want = torch.zeros(E, dtype=torch.float16)
    want[ids] = (5.0 * torch.tensor(std).to(torch.float16))[ids]  # add_skilled_experts.py:55
    assert same(got, want) and same(got, R.bias_vector(ids, std, E))
    assert float(got[5]) == 64992.0 and all(float(got[e]) == 0.0 for e in range(E) if e not in ids)
    # a duplicate id is applied once; the order does not matter
    assert same(ops.expert_bias([10, 3, 10, 3, 3], std, E, "cpu"), ops.expert_bias([3, 10], std, E, "cpu"))
    # an empty list: all +0
    z = ops.expert_bias([], std, E, "cpu")
    assert same(z, torch.zeros(E, dtype=torch.float16))
    # another scale
    assert same(ops.expert_bias([6], std, E, "cpu", scale=2.0)[6:7], (2.0 * torch.tensor([0.1]).half()))


def test_expert_bias_raises():
    E = 8
    std = [0.5] * E
    for bad in (-1, E, 1000):
        with pytest.raises(IndexError):
            ops.expert_bias([0, bad], std, E, "cpu")
    with pytest.raises(ValueError):
        ops.expert_bias([0], std[:-1], E, "cpu")
    nan = list(std)
    nan[2] = float("nan")
    with pytest.raises(ValueError):
        ops.expert_bias([1, 2], nan, E, "cpu")
    assert float(ops.expert_bias([1, 3], nan, E, "cpu")[2]) == 0.0  # NaN std of an UNLISTED expert is fine
    inf = list(std)
    inf[4] = float("inf")
    with pytest.raises(ValueError):
        ops.expert_bias([4], inf, E, "cpu")
    big = list(std)
    big[5] = 20000.0  # finite in fp16, 5 * 20000 is not
    with pytest.raises(ValueError):
        ops.expert_bias([5], big, E, "cpu")
    ops.expert_bias([4], big, E, "cpu")


def test_k_selected_is_the_literal_expression():
    from neuron_receivers.add_skilled_experts import k_selected
    for k in range(1, 65):
        assert k_selected(k) == int(0.8 * k) == R.k_selected(k)
        assert k_selected(k, 0.5) == int(0.5 * k)
    assert k_selected(12) == 9 and k_selected(51) == 40 and k_selected(25) == 20 and k_selected(1) == 0


def write_tree(root, T, L, E, lists, std):
    path = os.path.join(str(root), "runs", "adj_violence", "skilled", "experts")
    os.makedirs(path)
    for t in range(T):
        for l in range(L):
            with open(os.path.join(path, f"timestep_{t}_layer_{l}.json"), "w") as f:
                json.dump(lists[t][l], f)
    stats = {"time_steps": {str(t): {str(l): {"avg": [0.0] * E, "std": std[t][l]} for l in range(L)} for t in range(T)}}
    with open(os.path.join(str(root), "runs", "adj_violence", "predictivity_base_expert.json"), "w") as f:
        json.dump(stats, f)
    return path, stats


def test_statistics_path_and_overrides(tmp_path):
    from neuron_receivers import AddExperts, GEGLU
    from neuron_receivers.add_skilled_experts import stats_path
    assert stats_path("/a/b/adj_x/c/d") == "/a/b/adj_x/predictivity_base_expert.json"
    T, L, E = 2, 2, 8
    lists = {t: {l: [(t + l) % E, 5] for l in range(L)} for t in range(T)}
    lists[1][1] = []
    std = {t: {l: [0.25 * (t + 1) + 0.01 * e + l for e in range(E)] for l in range(L)} for t in range(T)}
    path, stats = write_tree(tmp_path, T, L, E, lists, std)
    assert stats_path(path) == os.path.join(str(tmp_path), "runs", "adj_violence", "predictivity_base_expert.json")
    rec = AddExperts(0, path, T, L)
    assert rec.expert_indices == lists and rec.avg_activation == std
    assert rec.replace_fn is GEGLU and rec.keep_nsfw is False and (rec.timestep, rec.layer) == (0, 0)
    assert AddExperts(0, path, T, L, True).keep_nsfw is True  # (not the replace_fn slot)
    assert (rec.bias_scale, rec.k_fraction, rec.count_selected, rec.store_gates) == (5.0, 0.8, False, True)
    # overrides: a dict, a path, lists; the list files and the derived statistics file are then not read
    other = {t: {l: [1.0] * E for l in range(L)} for t in range(T)}
    as_dict = {"time_steps": {str(t): {str(l): {"std": other[t][l]} for l in range(L)} for t in range(T)}}
    r2 = AddExperts(0, path, T, L, activation_stats=as_dict)
    assert r2.avg_activation == other and r2.expert_indices == lists
    int_keys = {t: {l: {"std": other[t][l]} for l in range(L)} for t in range(T)}  # (a dict built in Python, no JSON trip)
    assert AddExperts(0, path, T, L, activation_stats=int_keys).avg_activation == other
    with pytest.raises(KeyError):
        AddExperts(0, path, T, L, activation_stats={"time_steps": {"0": as_dict["time_steps"]["0"]}})
    p2 = tmp_path / "elsewhere.json"
    p2.write_text(json.dumps(as_dict))
    assert AddExperts(0, path, T, L, activation_stats=str(p2)).avg_activation == other
    mine = {t: {l: [7] for l in range(L)} for t in range(T)}
    r3 = AddExperts(0, None, T, L, expert_indices=mine, activation_stats=as_dict, store_gates=False)
    assert r3.expert_indices == mine and r3.store_gates is False
    with pytest.raises(FileNotFoundError):
        AddExperts(0, str(tmp_path / "no" / "such" / "dir" / "x"), T, L, expert_indices=mine)


def test_restated_hook_pieces():
    """add_experts_ref, the GPU tests' checker: the biased score is the reference's indexed assignment, the top-k with
    ties toward the lowest id agrees with torch.topk wherever the k-th score is not tied."""
    g = torch.Generator().manual_seed(0)
    E, rows, kk = 64, 50, 9
    score = (torch.randn(rows, E, generator=g) * 3).half()
    std = [float(v) for v in torch.rand(E, generator=g)]
    ids = [5, 9, 5, 63]
    want = score.clone()
    want[:, ids] = want[:, ids] + 5.0 * torch.tensor(std).to(score.dtype)[ids]
    got = R.biased(score, ids, std)
    assert same(got, want) and same(got, score + R.bias_vector(ids, std, E))
    assert same(R.biased(score, [], std), score)
    on = R.topk_lowest(got.numpy(), kk)
    s = np.sort(got.float().numpy(), axis=1)[:, ::-1]
    clear = s[:, kk - 1] != s[:, kk]
    ref = np.zeros_like(on)
    np.put_along_axis(ref, torch.topk(got, kk, dim=-1)[1].numpy(), True, axis=1)
    assert clear.any() and np.array_equal(on[clear], ref[clear]) and (on.sum(1) == kk).all()
    tied = np.array([[1.0, 2.0, 2.0, 2.0, 0.5, np.inf, np.inf]], dtype=np.float16)
    assert R.topk_lowest(tied, 3).tolist() == [[False, True, False, False, False, True, True]]
