"""Skill discovery on the HIP kernels: the statistics that PRODUCE the removal lists and Wanda
masks the hot-path receivers consume.

  * ColumnNormCalculator / TimeLayerColumnNorm — utils.py:321-370 of the reference. The running column norm
    sqrt(c^2 + n^2) is kept on the device as a squared fp32 sum per (t, l) (sdmoe_colnorm_accum), so a hooked
    call costs one streaming pass over the GEGLU output instead of a device->host copy of it (the reference's
    `.detach().cpu()` per call, wanda_receiver.py:50).
  * wanda_masks — modularity/wanda.py:140-173: metric = |W_down| * act_norm per (t, l), per row the top
    `sparsity_ratio` adjusted-prompt metrics that also beat the base-prompt metric -> bit-packed masks on device
    (sdmoe_wanda_mask), saved in the reference's pickle format or the native .npz.
  * update_set_diff / select_skilled_experts / save_expert_lists — the host bookkeeping of
    modularity/moefy_skilled_experts.py:97-124 and mod_utils.py:178-182 that turns GetExperts label lists into
    the timestep_{t}_layer_{l}.json files RemoveExperts reads.
  * Average / StandardDev / StatMeter — the running per-neuron statistics of NeuronPredictivity (utils.py:233-317):
    host-side numpy on the fp16 maxima the receivers copy back once per pipeline call, one numpy operation per
    step so every intermediate is rounded to fp16 exactly where the reference's is.
  * t_test_neurons / ap_neurons / save_neuron_masks — modularity/paired_t_test.py:66-79,142 and
    modularity/skilled_neuron_ap.py:166-177: statistics -> the predictivity_{t}_{l}.json 0/1 masks RemoveNeurons reads.
  * t_test_experts / expert_lists_from_statistics — modularity/paired_t_test_experts.py:47-65: the ExpertPredictivity
    statistics (predictivity_{base,adj}_expert.json, diff_std_expert.json) -> expert id lists for save_expert_lists.
  * accumulate_expert_counter / save_expert_counter — moefication/freq_expert_select.py:43-72 (and
    modularity/moefy_skilled_experts.py:23-36): FrequencyMeasure label counters averaged over the images of a dataset
    -> expert_counter_{topk}.json.
  * sparsity_ratios / accumulate_sparsity / neuron_zero_fraction — sparsity/check_sparsity.py:34-46 from the device
    counts of SparsityMeasure: the per-call zero ratio, the StatMeter behind sparsity.json, and per-neuron zero
    fractions.
  * noise_distances / NoiseObjective — modularity/remove_experts_noise_hpo.py:39-45, 73-87, 124-131: the float64 sums
    of sdmoe_noise_distance -> the driver's two distances per step and prompt, its per-step averages, the trial's score
    and noise_diff_per_sample.json.
"""
from __future__ import annotations

import json
import os
import pickle
from collections import Counter

import numpy as np
import torch

from . import mask_io, ops


class ColumnNormCalculator:
    """Column L2 norms of a growing stack of (row-normalised) fp16 rows, accumulated on the device."""

    def __init__(self, device=None):
        self.device = device
        self.sumsq = None
        self.rows = 0

    def add_rows(self, rows: torch.Tensor):
        """rows: [M, F] fp16 device view of the RAW activations; each row is L2-normalised in the kernel
        (F.normalize(p=2, dim=1), wanda_receiver.py:52) before its squares are added."""
        if self.sumsq is None:
            self.sumsq = torch.zeros(rows.shape[1], dtype=torch.float32, device=rows.device)
        ops.colnorm_accum(rows, self.sumsq)
        self.rows += rows.shape[0]

    def get_column_norms(self) -> torch.Tensor:
        """fp16 CPU tensor [F] (the reference's norms are fp16 CPU tensors); empty if nothing was added."""
        if self.sumsq is None:
            return torch.tensor([])
        return self.sumsq.sqrt().to(torch.float16).cpu()


class TimeLayerColumnNorm:
    def __init__(self, T, n_layers):
        self.T = T
        self.n_layers = n_layers
        self.column_norms = {t: {i: ColumnNormCalculator() for i in range(n_layers)} for t in range(T)}

    def update(self, rows, t, n_layer):
        self.column_norms[t][n_layer].add_rows(rows)

    def get_column_norms(self):
        return {t: {i: self.column_norms[t][i].get_column_norms() for i in range(self.n_layers)}
                for t in range(self.T)}

    def save(self, path):
        torch.save(self.get_column_norms(), path)


def wanda_masks(gate_weights, layer_names, act_norms_base, act_norms_adj, sparsity_ratio, timesteps, device="cuda"):
    """modularity/wanda.py:140-160 for every (t, l): returns {t: {l: np.uint8 [C, F/8]}} bit-packed masks.
    gate_weights[name] = |W_down| (or W_down: the kernel takes |.|) [C, F]; norms [F] (any float dtype, used
    as fp16 like the reference's); kprune = int(sparsity_ratio * F)."""
    names = sorted(layer_names)  # wanda.py:131 sorts the layer names
    out = {}
    wdev = {}
    for t in range(timesteps):
        out[t] = {}
        for l, name in enumerate(names):
            if name not in wdev:
                wdev[name] = gate_weights[name].to(device, torch.float16).contiguous()
            W = wdev[name]
            F = W.shape[1]
            nb = act_norms_base[t][l].to(device, torch.float16).contiguous()
            na = act_norms_adj[t][l].to(device, torch.float16).contiguous()
            bits = ops.wanda_mask(W, nb, na, int(sparsity_ratio * F))
            out[t][l] = bits
    torch.cuda.synchronize()
    return {t: {l: out[t][l].cpu().numpy() for l in out[t]} for t in out}


def save_wanda_masks(masks, path, fmt="pkl"):
    """Write timestep_{t}_layer_{l}.pkl (scipy csr_matrix int64, wanda.py:169-173) or .npz (bit-packed)."""
    os.makedirs(path, exist_ok=True)
    for t, layers in masks.items():
        for l, bits in layers.items():
            if fmt == "npz":
                np.savez_compressed(os.path.join(path, f"timestep_{t}_layer_{l}.npz"), bits=bits)
                continue
            import scipy.sparse
            dense = mask_io.unpack_mask(bits, bits.shape[-1] * 8)
            with open(os.path.join(path, f"timestep_{t}_layer_{l}.pkl"), "wb") as f:
                pickle.dump(scipy.sparse.csr_matrix(dense), f)


def update_set_diff(set1, set2, symm=False):
    """mod_utils.py:178-182."""
    return set1.symmetric_difference(set2) if symm else set1.difference(set2)


def select_skilled_experts(set_diff, n_prompts, skill_ratio):
    """moefy_skilled_experts.py:110-121: experts that appear in the per-prompt set differences of at least
    int(skill_ratio * n_prompts) prompts, most common first."""
    out = {}
    for t, layers in set_diff.items():
        out[t] = {}
        for l, diffs in layers.items():
            counter = Counter(diffs).most_common(len(Counter(diffs)))
            thr = int(skill_ratio * n_prompts)
            out[t][l] = [int(e) for e, c in counter if c >= thr]
    return out


def save_expert_lists(lists, path):
    """timestep_{t}_layer_{l}.json files (moefy_skilled_experts.py:106-124) for RemoveExperts."""
    os.makedirs(path, exist_ok=True)
    for t, layers in lists.items():
        for l, ids in layers.items():
            with open(os.path.join(path, f"timestep_{t}_layer_{l}.json"), "w") as f:
                json.dump([int(e) for e in ids], f)


class Average:
    """Running mean: sum += val, avg = sum / count (in the dtype of val: fp16 rows give fp16 sums)."""

    def __init__(self):
        self.val = 0
        self.sum = 0
        self.count = 0
        self.avg = 0

    def update(self, val, n=1):
        self.val = val
        self.sum = self.sum + val * n
        self.count += n
        self.avg = self.sum / self.count


class StandardDev:
    """Welford's running variance: n, mean and M2 (the sum of squared deviations), element-wise in the dtype of x."""

    def __init__(self):
        self.n = 0
        self.mean = 0
        self.M2 = 0

    def update(self, x):
        self.n += 1
        delta = x - self.mean
        self.mean = self.mean + delta / self.n
        self.M2 = self.M2 + delta * (x - self.mean)

    def variance(self):
        return float("nan") if self.n < 2 else self.M2 / (self.n - 1)

    def stddev(self):
        return self.variance() ** 0.5


class StatMeter:
    """An Average and a StandardDev per (timestep, layer); save() writes the reference's predictivity JSON."""

    def __init__(self, T, n_layers):
        self.T = T
        self.n_layers = n_layers
        self.results = {"time_steps": {t: {l: {"avg": Average(), "std": StandardDev()} for l in range(n_layers)}
                                       for t in range(T)}}

    def update(self, val, t, n_layer):
        cell = self.results["time_steps"][t][n_layer]
        cell["avg"].update(val)
        cell["std"].update(val)

    def to_json(self):
        """{"time_steps": {t: {l: {"avg": [...], "std": [...]}}}} (a cell never updated: avg 0, std NaN)."""
        def plain(v):
            return v.tolist() if isinstance(v, np.ndarray) else v
        return {"time_steps": {t: {l: {"avg": plain(c["avg"].avg), "std": plain(c["std"].stddev())}
                                   for l, c in layers.items()} for t, layers in self.results["time_steps"].items()}}

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_json(), f)


def t_test_neurons(base_avg, adj_avg, diff_std, n_prompts, critical_value):
    """Paired t-test of one (t, l) (modularity/paired_t_test.py:72-79,142): t = (base - adj) / (diff_std /
    sqrt(n_prompts)) in float64; returns (t, t < -critical_value) -- neurons that fire more on the concept prompts."""
    base = np.asarray(base_avg, dtype=np.float64)
    adj = np.asarray(adj_avg, dtype=np.float64)
    diff = np.asarray(diff_std, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (base - adj) / (diff / (n_prompts ** 0.5))
    return t, t < -critical_value


def ap_neurons(hit_rate, ratio=0.05):
    """modularity/skilled_neuron_ap.py:166-172: the int(ratio * F) best-ranked neurons of argsort()[::-1] as a 0/1
    float mask."""
    pred = np.asarray(hit_rate)
    mask = np.zeros(len(pred))
    mask[pred.argsort()[::-1][:int(ratio * len(pred))]] = 1
    return mask


def save_neuron_masks(masks, path):
    """predictivity_{t}_{l}.json files (lists of 0.0 / 1.0) for RemoveNeurons; masks[t][l]: 0/1 (or bool) [F]."""
    os.makedirs(path, exist_ok=True)
    for t, layers in masks.items():
        for l, m in layers.items():
            with open(os.path.join(path, f"predictivity_{t}_{l}.json"), "w") as f:
                json.dump([float(v) for v in np.asarray(m).reshape(-1) != 0], f)


def t_test_experts(base_avg, adj_avg, diff_std, n_prompts, critical_value=3.579):
    """Paired t-test of one (t, l) over experts (modularity/paired_t_test_experts.py:51-61): the sorted ids of the
    experts with t < -critical_value, t as in t_test_neurons -- experts that score higher on the concept prompts."""
    _, skilled = t_test_neurons(base_avg, adj_avg, diff_std, n_prompts, critical_value)
    return [int(e) for e in np.flatnonzero(skilled)]


def _json_or_path(obj):
    if isinstance(obj, (str, os.PathLike)):
        with open(obj) as f:
            return json.load(f)
    return obj


def _cell(d, key):
    """d[key] of a dict keyed by ints (in memory) or by their strings (read back from JSON)."""
    return d[key] if key in d else d[str(key)]


def expert_lists_from_statistics(base_json, adj_json, diff_std_json, n_prompts, critical_value=3.579):
    """paired_t_test_experts.py:47-65 over every (t, l): base_json / adj_json are ExpertPredictivity's saved statistics
    ({"time_steps": {t: {l: {"avg": [...], "std": [...]}}}}: StatMeter.save / to_json), diff_std_json the paired
    {t: {l: [...]}} standard deviations of base - adj maxima; each a dict or the path of its JSON file. Returns
    {t: {l: [expert ids]}} with int keys, ready for save_expert_lists."""
    base, adj, diff = (_json_or_path(o) for o in (base_json, adj_json, diff_std_json))
    out = {}
    for tk, layers in base["time_steps"].items():
        t = int(tk)
        out[t] = {}
        for lk in layers:
            l = int(lk)
            b = _cell(_cell(base["time_steps"], t), l)["avg"]
            a = _cell(_cell(adj["time_steps"], t), l)["avg"]
            out[t][l] = t_test_experts(b, a, _cell(_cell(diff, t), l), n_prompts, critical_value)
    return out


def accumulate_expert_counter(expert_counter, label_counter, layer_names, num_images):
    """freq_expert_select.py:43-47,61-64 (moefy_skilled_experts.py:23-36): expert_counter[t][name][e] +=
    label_counter[t][layer_names.index(name)][e] / num_images, in the reference's order (one division, one addition
    per element and image). expert_counter None starts the {t: {name: [0] * E}} dict of the reference. Returns it."""
    if expert_counter is None:
        expert_counter = {t: {name: [0] * len(label_counter[t][layer_names.index(name)]) for name in layer_names}
                          for t in label_counter}
    for t in expert_counter:
        for name in layer_names:
            row = label_counter[t][layer_names.index(name)]
            acc = expert_counter[t][name]
            for e in range(len(acc)):
                acc[e] += float(row[e]) / num_images
    return expert_counter


def save_expert_counter(expert_counter, path, topk):
    """freq_expert_select.py:70-72: expert_counter_{topk}.json under `path` (the reference's JSON shape: timestep ->
    layer name -> list of floats). Returns the file's path."""
    os.makedirs(path, exist_ok=True)
    fname = os.path.join(path, f"expert_counter_{topk}.json")
    with open(fname, "w") as f:
        json.dump(expert_counter, f)
    return fname


def sparsity_ratios(calls):
    """SparsityMeasure.calls -> float64 [calls, groups]: zeros / elements per hooked call and group of images, the
    exact value of check_sparsity.py:41-45's "mean over tokens of (zeros in the row / F)" (every row has F elements, so
    the mean of the row ratios is the ratio of the sums; the reference evaluates it in fp32 and differs by rounding)."""
    if not len(calls):
        return np.zeros((0, 0), dtype=np.float64)
    zeros = np.stack([np.asarray(c["zeros"], dtype=np.int64) for c in calls])
    elements = np.stack([np.asarray(c["elements"], dtype=np.int64) for c in calls])
    return zeros.astype(np.float64) / elements.astype(np.float64)


def accumulate_sparsity(meter, ratios, num_geglu):
    """check_sparsity.py:34-46: hooked call i of a pipeline call updates StatMeter cell (i // num_geglu, i % num_geglu)
    with its zero ratio, once per prompt (column of `ratios`, [calls] or [calls, prompts]), prompt by prompt as the
    reference's dataset loop does. StatMeter.save then writes sparsity.json. Returns the meter."""
    r = np.asarray(ratios, dtype=np.float64)
    r = r[:, None] if r.ndim == 1 else r
    for p in range(r.shape[1]):
        for i in range(r.shape[0]):
            meter.update(float(r[i, p]), i // num_geglu, i % num_geglu)
    return meter


def neuron_zero_fraction(calls, num_geglu):
    """Per (timestep, layer) and neuron, the fraction of a group's rows whose gate counted as zero, from the
    per_neuron=True records of SparsityMeasure.calls: {t: {l: float64 [groups, F]}} (this port's addition: a neuron at
    1.0 is dead on that prompt, and neurons that are zero together are candidates for one expert)."""
    out = {}
    for i, c in enumerate(calls):
        if "neuron_zeros" not in c:
            raise ValueError("neuron_zero_fraction needs the records of SparsityMeasure(per_neuron=True)")
        nz = np.asarray(c["neuron_zeros"], dtype=np.float64)
        rows = np.asarray(c["rows"], dtype=np.float64).reshape(-1, 1)
        out.setdefault(i // num_geglu, {})[i % num_geglu] = nz / rows
    return out


def noise_distances(stats):
    """ops.noise_distance's [T, G, 4] sums (a device or host tensor, or an array) -> (l2 [T, G], l1n [T, G]) float64
    arrays: l2 = sqrt(S (a - b)^2), the driver's torch.norm(a - b) (remove_experts_noise_hpo.py:75), and l1n =
    sqrt(S (a / max(|a|_1, 1e-12) - b / max(|b|_1, 1e-12))^2), its distance of the F.normalize(p = 1)'d vectors (:78-84).
    One device->host copy of 4 T G doubles when stats is on a device."""
    s = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    s = s.astype(np.float64, copy=False)
    if s.ndim != 3 or s.shape[2] != 4:
        raise ValueError(f"noise_distances: expected [T, G, 4] sums, got {s.shape}")
    return np.sqrt(s[:, :, 0]), np.sqrt(s[:, :, 3])


class NoiseObjective:
    """The bookkeeping of the noise-HPO driver's remove_experts (modularity/remove_experts_noise_hpo.py:39-45, 73-87,
    124-131) over the samples (prompt pairs) of one trial: noise_diff[t] is an Average of l2 over the samples,
    avg_noise_diff the mean over the steps of those averages (the trial's score, minimised), noise_diff_per_sample[i]
    the mean over the steps of sample i's l1n."""

    def __init__(self, T):
        self.T = int(T)
        self.noise_diff = {t: Average() for t in range(self.T)}
        self.noise_diff_per_sample = {}

    def update(self, l2, l1n):
        """One sample ([T] arrays) or, from a prompt batch, G samples in prompt order ([T, G] arrays, the two outputs of
        noise_distances)."""
        l2 = np.asarray(l2, dtype=np.float64).reshape(self.T, -1)
        l1n = np.asarray(l1n, dtype=np.float64).reshape(self.T, -1)
        if l2.shape != l1n.shape:
            raise ValueError(f"NoiseObjective.update: l2 {l2.shape} and l1n {l1n.shape} differ")
        for g in range(l2.shape[1]):
            i = len(self.noise_diff_per_sample)
            per_sample = 0.0
            for t in range(self.T):
                self.noise_diff[t].update(float(l2[t, g]))
                per_sample += float(l1n[t, g])
            self.noise_diff_per_sample[i] = per_sample / self.T

    @property
    def avg_noise_diff(self):
        return sum(self.noise_diff[t].avg for t in range(self.T)) / self.T

    def save(self, path):
        """noise_diff_per_sample.json (:189-190) in `path` (a directory) or at `path` (a .json file name)."""
        fname = path if path.endswith(".json") else os.path.join(path, "noise_diff_per_sample.json")
        with open(fname, "w") as f:
            json.dump(self.noise_diff_per_sample, f)
        return fname
