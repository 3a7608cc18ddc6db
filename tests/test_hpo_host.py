"""CPU-only tests of the HPO path's host side: constructors and the HPO file layout, the per-timestep decision logic of
RemoveNeuronsHPO under a fake trial, the float64 restatement of the noise objective (tests/noise_ref.py) against the
reference driver's own arithmetic (tests/golden/noise_objective_*.npz, the float64 variant), and NoiseObjective's
bookkeeping against a hand computation. No GPU compute is launched here."""
import json
import os

import numpy as np
import pytest
import torch

import neuron_ref as R
import noise_ref as NR

DOF, CONF = 9, 0.95


class FakeTrial:
    def __init__(self, answers):
        self.answers, self.asked = answers, []

    def suggest_categorical(self, name, choices):
        assert choices == [0, 1]
        self.asked.append(name)
        return self.answers[name]


def write_layout(root, masks, dof=DOF, conf=CONF):
    folder = os.path.join(root, f"dof_{dof}_conf_{conf}")
    os.makedirs(folder)
    for t, row in masks.items():
        for l, m in row.items():
            with open(os.path.join(folder, f"timestep_{t}_layer_{l}.json"), "w") as f:
                json.dump([float(v) for v in m], f)


def some_masks(T, L, F=64, empty=()):
    rng = np.random.default_rng(T * 100 + L)
    return {t: {l: ([] if (t, l) in empty else (rng.random(F) < 0.2).astype(np.float64)) for l in range(L)}
            for t in range(T)}


# ------------------------------------------------------------------------------------------------ constructors
def test_constructors_need_no_device_and_are_exported(tmp_path):
    import neuron_receivers as nr
    from neuron_receivers import BaseUNetReceiver, RemoveNeuronsHPO, RemoveNeuronsNoiseHPO, SaveStates
    for name in ("BaseUNetReceiver", "RemoveNeuronsHPO", "RemoveNeuronsNoiseHPO", "SaveStates"):
        assert hasattr(nr, name)
    T, L = 3, 2
    masks = some_masks(T, L)
    write_layout(str(tmp_path), masks)
    base = BaseUNetReceiver(seed=1, T=T, n_layers=L)
    assert base.unet_output == {t: [] for t in range(T)} and base.timestep == 0 and base.store_outputs
    base.update_timestep()
    assert base.timestep == 1
    base.reset_time()
    assert base.timestep == 0
    assert not BaseUNetReceiver(1, T, L, store_outputs=False).store_outputs
    for cls in (RemoveNeuronsHPO, RemoveNeuronsNoiseHPO):
        rec = cls(seed=1, path_expert_indx=str(tmp_path), T=T, n_layers=L, dof_val=DOF, conf_val=CONF,
                  trials_per_layer=FakeTrial({}))
        for t in range(T):
            for l in range(L):
                assert np.array_equal(rec.expert_indices[t][l], np.asarray(masks[t][l]) != 0)
        assert rec.update_for_t == {} and rec.gates == [] and (rec.timestep, rec.layer) == (0, 0)
    assert rec.unet_output == {t: [] for t in range(T)}
    with pytest.raises(RuntimeError):
        rec.device_outputs()  # nothing captured yet
    ss = SaveStates(0, T, L)
    assert all(ss.hidden_states[t][l].numel() == 0 for t in range(T) for l in range(L))
    ss.hidden_states[1][1] = torch.arange(6, dtype=torch.float16).view(1, 2, 3)
    ss.save(str(tmp_path / "states.pt"))
    back = torch.load(str(tmp_path / "states.pt"))
    assert torch.equal(back[1][1], ss.hidden_states[1][1]) and back[0][0].numel() == 0


def test_hpo_file_layout(tmp_path):
    """dof_{dof}_conf_{conf}/timestep_{t}_layer_{l}.json; another confidence level is another folder; a missing folder
    is an error; in-memory masks need no files."""
    from neuron_receivers import RemoveNeuronsHPO
    T, L = 2, 2
    m_a, m_b = some_masks(T, L, empty=[(0, 1)]), some_masks(T, L, F=96)
    write_layout(str(tmp_path), m_a, 9, 0.95)
    write_layout(str(tmp_path), m_b, 9, 0.99)
    a = RemoveNeuronsHPO(0, str(tmp_path), T, L, 9, 0.95)
    b = RemoveNeuronsHPO(0, str(tmp_path), T, L, 9, 0.99)
    assert a.expert_indices[0][1].size == 0 and a.expert_indices[1][1].size == 64
    assert b.expert_indices[0][1].size == 96
    assert np.array_equal(b.expert_indices[1][0], m_b[1][0] != 0)
    with pytest.raises(FileNotFoundError):
        RemoveNeuronsHPO(0, str(tmp_path), T, L, 9, 0.9)
    c = RemoveNeuronsHPO(0, None, T, L, 9, 0.9, masks=m_a)
    assert np.array_equal(c.expert_indices[1][1], m_a[1][1] != 0)


# ------------------------------------------------------------------------------------------------ decisions
def walk(rec, T, L):
    """The (t, l) order of a pipeline call."""
    return [[rec.decide(t, l) for l in range(L)] for t in range(T)]


def test_decisions_with_a_fake_trial():
    from neuron_receivers import RemoveNeuronsHPO
    T, L = 13, 3
    masks = some_masks(T, L, empty=[(2, 0), (11, 0), (12, 0), (12, 1)])
    trial = FakeTrial({"timestep_10": 0, "timestep_11": 1, "timestep_12": 0})
    rec = RemoveNeuronsHPO(0, None, T, L, DOF, CONF, trials_per_layer=trial, masks=masks)
    got = walk(rec, T, L)
    # t < 10 never asks and always removes (an empty list removes nothing)
    assert all(got[t] == [True] * L for t in range(10) if t != 2) and got[2] == [False, True, True]
    # t >= 10 asks exactly once per timestep, under the name timestep_{t}; an empty layer 0 asks at the first non-empty
    # layer (the reference raises KeyError there)
    assert trial.asked == ["timestep_10", "timestep_11", "timestep_12"]
    assert got[10] == [False] * L and got[11] == [False, True, True] and got[12] == [False] * L
    assert rec.update_for_t == {**{t: 1 for t in range(10)}, 10: 0, 11: 1, 12: 0}
    # a new run asks again, once per timestep
    rec.reset_time_layer()
    assert rec.update_for_t == {} and (rec.timestep, rec.layer) == (0, 0)
    walk(rec, T, L)
    assert trial.asked == ["timestep_10", "timestep_11", "timestep_12"] * 2


def test_decisions_from_a_sequence_and_without_a_trial():
    from neuron_receivers import RemoveNeuronsHPO, RemoveNeuronsNoiseHPO
    T, L = 12, 2
    masks = some_masks(T, L)
    seq = [0] * 10 + [1, 0]  # entries below timestep 10 are not consulted
    rec = RemoveNeuronsHPO(0, None, T, L, DOF, CONF, trials_per_layer=seq, masks=masks)
    got = walk(rec, T, L)
    assert all(got[t] == [True, True] for t in range(11)) and got[11] == [False, False]
    none = RemoveNeuronsHPO(0, None, T, L, DOF, CONF, masks=masks)
    assert none.decide(9, 0) is True
    with pytest.raises(ValueError, match="trials_per_layer"):
        none.decide(10, 0)
    # the noise receiver's switch is commented out in the reference: every timestep removes, the trial is never asked
    trial = FakeTrial({})
    noise = RemoveNeuronsNoiseHPO(0, None, T, L, DOF, CONF, trials_per_layer=trial,
                                  masks=some_masks(T, L, empty=[(11, 1)]))
    got = walk(noise, T, L)
    assert all(got[t] == [True, True] for t in range(11)) and got[11] == [True, False]
    assert trial.asked == [] and noise.update_for_t == {}


def test_decisions_match_the_reference_fixture():
    """The recorded run of the reference's hook under its fake trial: same questions, same update_for_t."""
    from neuron_receivers import RemoveNeuronsHPO
    cases = R.golden("hpo_remove")
    assert len(cases) == 2
    for _, c in cases:
        T, L, Fn = int(c["T"]), int(c["L"]), 4 * int(c["C"])
        masks = {t: {l: ([] if c["mask_empty"][t, l] else np.unpackbits(c["mask_bits"][t, l], count=Fn,
                                                                          bitorder="little")) for l in range(L)}
                 for t in range(T)}
        trial = FakeTrial({"timestep_10": int(c["answers"][0]), "timestep_11": int(c["answers"][1])})
        rec = RemoveNeuronsHPO(0, None, T, L, float(c["dof"]), float(c["conf"]), trials_per_layer=trial, masks=masks)
        walk(rec, T, L)
        assert trial.asked == c["asked"].tolist()
        assert [rec.update_for_t[t] for t in range(T)] == c["update_for_t"].tolist()
        assert sorted(set(c["answers"].tolist())) == [0, 1]


# ------------------------------------------------------------------------------------------------ noise objective
def noise_case():
    (_, c), = R.golden("noise_objective")
    return c


def test_noise_ref_equals_the_float64_fixture():
    c = noise_case()
    P, T = int(c["P"]), int(c["T"])
    assert c["a"].dtype == np.float16 and c["a"].shape == (P, T, 2, 4, 8, 8)
    for p in range(P):
        l2, l1n = NR.distances(c["a"][p], c["b"][p])  # one group: the whole [2, 4, 8, 8] output, as output[0].view(-1)
        assert l2.shape == (T, 1)
        np.testing.assert_allclose(l2[:, 0], c["l2_fp64"][p], rtol=1e-12, atol=0)
        np.testing.assert_allclose(l1n[:, 0], c["l1n_fp64"][p], rtol=1e-12, atol=0)
    assert c["l2_fp64"][0, 1] == 0.0 and c["l1n_fp64"][0, 1] == 0.0           # a == b
    ulp = float(np.abs(c["a"][1, 2].astype(np.float64) - c["b"][1, 2].astype(np.float64)).max())
    assert c["l2_fp64"][1, 2] == ulp and c["l1n_fp64"][1, 2] > 0              # one element moved by one fp16 ulp
    # groups: every image its own group = per-image sums
    s = NR.sums(c["a"][0], c["b"][0], img_group=[0, 1], ngroups=2)
    one = NR.sums(c["a"][0][:, 1:], c["b"][0][:, 1:])
    assert np.array_equal(s[:, 1], one[:, 0])


def test_noise_objective_bookkeeping(tmp_path):
    from sdmoe.discovery import NoiseObjective, noise_distances
    c = noise_case()
    P, T = int(c["P"]), int(c["T"])
    l2, l1n = c["l2_fp64"], c["l1n_fp64"]
    # the hand computation
    step_avg = [sum(l2[p, t] for p in range(P)) / P for t in range(T)]
    score = sum(step_avg) / T
    per_sample = [sum(l1n[p, t] for t in range(T)) / T for p in range(P)]
    np.testing.assert_allclose(step_avg, c["step_avg_fp64"], rtol=1e-14)
    np.testing.assert_allclose(score, float(c["avg_noise_diff_fp64"]), rtol=1e-14)
    np.testing.assert_allclose(per_sample, c["per_sample_fp64"], rtol=1e-14)
    ref = NR.objective(l2, l1n)
    np.testing.assert_allclose(ref[0], step_avg, rtol=1e-14)
    # sample by sample, as the reference's loop ...
    obj = NoiseObjective(T)
    for p in range(P):
        stats = torch.from_numpy(NR.sums(c["a"][p], c["b"][p]))
        obj.update(*noise_distances(stats))
    # ... and as one prompt batch: [T, P] arrays
    batch = NoiseObjective(T)
    batch.update(l2.T, l1n.T)
    for o in (obj, batch):
        np.testing.assert_allclose([o.noise_diff[t].avg for t in range(T)], step_avg, rtol=1e-12)
        np.testing.assert_allclose(o.avg_noise_diff, score, rtol=1e-12)
        assert sorted(o.noise_diff_per_sample) == list(range(P))
        np.testing.assert_allclose([o.noise_diff_per_sample[p] for p in range(P)], per_sample, rtol=1e-12)
        assert o.noise_diff[0].count == P
    fname = obj.save(str(tmp_path))
    assert os.path.basename(fname) == "noise_diff_per_sample.json"
    with open(fname) as f:
        saved = json.load(f)
    assert sorted(saved) == [str(p) for p in range(P)]
    np.testing.assert_allclose([saved[str(p)] for p in range(P)], per_sample, rtol=1e-12)
    with pytest.raises(ValueError):
        noise_distances(np.zeros((3, 4)))


def test_pipeline_hook_registration_needs_no_device():
    """The seam's list and handle are plain host objects."""
    from sdmoe.pipeline import StableDiffusionPipeline
    pipe = StableDiffusionPipeline.__new__(StableDiffusionPipeline)
    pipe._unet_output_hooks = []
    calls = []
    h1 = pipe.register_unet_output_hook(lambda *a: calls.append(("one",) + a))
    h2 = pipe.register_unet_output_hook(lambda *a: calls.append(("two",) + a))
    eps = torch.zeros((2 * 16, 8), dtype=torch.float16)
    pipe._after_unet(3, eps, 16)
    assert [(c[0], c[1], c[3], c[4]) for c in calls] == [("one", 3, 2, 16), ("two", 3, 2, 16)]
    assert calls[0][2] is eps
    h1.remove()
    h1.remove()  # idempotent
    assert len(pipe._unet_output_hooks) == 1
    h2.remove()
    assert pipe._unet_output_hooks == []
