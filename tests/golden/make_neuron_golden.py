"""Golden vectors for the neuron-level path, made by running the REFERENCE's own receivers and statistics classes.

Runs only in the build container (the reference tree is not present on the GPU box). Through make_golden's stub of
the absent `diffusers` package it imports, from the reference tree,
  * NeuronPredictivity.hook_fn     neuron_receivers/predictivity.py:42-53
  * NeuronPredictivityBB.hook_fn   neuron_receivers/neuron_predictivity_bb.py:43-63
  * RemoveNeurons.hook_fn          neuron_receivers/remove_skilled_neurons.py:26-42
  * utils.StatMeter / StandardDev / Average (utils.py:233-317), driven as modularity/modularity_analysis.py:63-110
    drives them (reset_time_layer per prompt, a paired StandardDev over base - adj maxima, StatMeter.save)
and runs them on the CPU in fp16 on seeded inputs. Only data is written (seeds, recorded outputs, statistics); the
tests regenerate x and the weights from the seeds with synth.py. The t-test values follow the one formula of
modularity/paired_t_test.py:72-79 on the saved JSON, the AP mask modularity/skilled_neuron_ap.py:166-172 on a stored
hit-rate vector (tie-free, so the ranking does not depend on the sort implementation).

Fixture kinds: neuron_pred, neuron_pred_bb, remove_neurons, neuron_ttest. index.json is left alone.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_neuron_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402
import synth  # noqa: E402


def x_seed(seed, prompt, kind, call):
    """Seed of the tokens of hooked call `call` of prompt `prompt` (kind 0 = base, 1 = adj)."""
    return seed + 1000 + (prompt * 2 + kind) * 100 + call


def modules(C, seed, L, act, gate_bias, dtype=torch.float16):
    mods = [MG.make_geglu(C, seed + l, dtype, gate_bias=gate_bias) for l in range(L)]
    for m in mods:
        m.bounding_box = None
        if act == "relu":
            m.gelu = F.relu
    return mods


def meter_state(meter, T, L):
    """(Average.sum, StandardDev.mean, StandardDev.M2) as [T, L, F] arrays, StandardDev.n."""
    cells = meter.results['time_steps']
    s = np.stack([np.stack([cells[t][l]['avg'].sum for l in range(L)]) for t in range(T)])
    mean = np.stack([np.stack([cells[t][l]['std'].mean for l in range(L)]) for t in range(T)])
    m2 = np.stack([np.stack([cells[t][l]['std'].M2 for l in range(L)]) for t in range(T)])
    return s, mean, m2, cells[0][0]['std'].n


def saved_json(meter):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "predictivity.json")
        meter.save(p)
        with open(p, "rb") as f:
            return np.frombuffer(f.read(), dtype=np.uint8).copy()


def run_prompts(recs, mods, seed, P, T, L, N, C, utils):
    """modularity_analysis.py:72-93 with tensors for prompts: returns per-prompt maxima [kind][P, T, L, F], the
    paired StandardDev grid and the first hooked call's output."""
    diff = {t: {l: utils.StandardDev() for l in range(L)} for t in range(T)}
    maxima = [[], []]
    out0 = None
    for p in range(P):
        for kind, rec in enumerate(recs):
            rec.reset_time_layer()
            for call in range(T * L):
                x = torch.from_numpy(synth.tokens((2, N, C), x_seed(seed, p, kind, call))).half()
                with torch.no_grad():
                    o = rec.hook_fn(mods[call % L], (x,), None)
                if out0 is None:
                    out0 = o.numpy()
            maxima[kind].append(np.stack([np.stack([rec.max_gate[t][l] for l in range(L)]) for t in range(T)]))
        if len(recs) == 2:
            for t in range(T):
                for l in range(L):
                    diff[t][l].update(recs[0].max_gate[t][l] - recs[1].max_gate[t][l])
    return [np.stack(m) for m in maxima if m], diff, out0


def gen_neuron_pred(pred_mod, utils):
    cases = []
    C, N, T, L, P = 320, 32, 2, 2, 5
    for i, (act, gb) in enumerate([("gelu", 0.0), ("relu", 0.0), ("gelu", -3.0)]):
        seed = 7000 + 10 * i
        mods = modules(C, seed, L, act, gb)
        recs = [MG.quiet(pred_mod.NeuronPredictivity, 0, T, L) for _ in range(2)]
        (mb, ma), diff, out0 = run_prompts(recs, mods, seed, P, T, L, N, C, utils)
        assert mb.dtype == np.float16
        if gb < 0:
            assert (mb < 0).any() and (mb > 0).any()  # columns whose gate is negative on every row, and others
        sb, meanb, m2b, nb = meter_state(recs[0].predictivity, T, L)
        sa, meana, m2a, na = meter_state(recs[1].predictivity, T, L)
        dmean = np.stack([np.stack([diff[t][l].mean for l in range(L)]) for t in range(T)])
        dm2 = np.stack([np.stack([diff[t][l].M2 for l in range(L)]) for t in range(T)])
        dstd = np.stack([np.stack([diff[t][l].stddev() for l in range(L)]) for t in range(T)])
        counter = np.array([recs[0].timestep, recs[0].layer])
        jb, ja = saved_json(recs[0].predictivity), saved_json(recs[1].predictivity)  # (save() consumes the meter)
        cases.append(dict(
            name=f"neuron_pred_C{C}_{act}_gb{gb}", kind="neuron_pred", dtype="float16", C=C, N=N, T=T, L=L, P=P,
            act=act, seed=seed, gate_bias=gb, max_gate_base=mb, max_gate_adj=ma, sum_base=sb, mean_base=meanb,
            M2_base=m2b, n_base=nb, sum_adj=sa, mean_adj=meana, M2_adj=m2a, n_adj=na, json_base=jb, json_adj=ja,
            diff_mean=dmean, diff_M2=dm2, diff_std=dstd, out0=out0, counter_after=counter))
    return cases


def gen_neuron_pred_bb(bb_mod, utils):
    """The reference's BB receiver wraps its counter at layer 15 whatever n_layers is, so these run 16 layers (two
    distinct modules, layer l -> module l % 2) and one timestep. Its try/except turns a missing or an empty box into
    the all-token maximum; an out-of-range index raises there (the indexing sits outside the try), so that rule of
    this port (fall back, as GetExperts does) has no golden and is tested against the all-token result instead."""
    cases = []
    C, N, T, L, P = 320, 32, 1, 16, 3
    for i, (tag, bb) in enumerate([("box", [0, 3, 5, 17, 31]), ("none", None), ("empty", [])]):
        seed = 7100 + 10 * i
        mods = modules(C, seed, 2, "gelu", 0.0)
        for m in mods:
            m.bounding_box = bb
        rec = MG.quiet(bb_mod.NeuronPredictivityBB, 0, T, L)
        maxima, out0 = [], None
        for p in range(P):
            rec.reset_time_layer()
            for call in range(T * L):
                x = torch.from_numpy(synth.tokens((2, N, C), x_seed(seed, p, 0, call))).half()
                with torch.no_grad():
                    o = rec.hook_fn(mods[call % 2], (x,), None)
                if out0 is None:
                    out0 = o.numpy()
            maxima.append(np.stack([np.stack([rec.max_gate[t][l] for l in range(L)]) for t in range(T)]))
        s, mean, m2, n = meter_state(rec.predictivity, T, L)
        cases.append(dict(
            name=f"neuron_pred_bb_C{C}_{tag}", kind="neuron_pred_bb", dtype="float16", C=C, N=N, T=T, L=L, P=P,
            act="gelu", seed=seed, gate_bias=0.0, bb=np.array(bb if bb is not None else [], dtype=np.int64),
            bb_none=bb is None, max_gate_base=np.stack(maxima), sum_base=s, mean_base=mean, M2_base=m2, n_base=n,
            out0=out0, counter_after=np.array([rec.timestep, rec.layer])))
    return cases


def gen_remove_neurons(rem_mod):
    cases = []
    T, L = 2, 2
    spec = [(320, 16, "gelu", [0, 1, 2, 3]), (320, 16, "relu", [0, 1, 2, 3]),
            (1280, 8, "gelu", [0, 2]), (1280, 8, "relu", [0, 2])]  # (C, N, act, stored calls)
    for i, (C, N, act, keep) in enumerate(spec):
        seed = 7200 + 10 * i
        Fn = 4 * C
        rng = np.random.default_rng(seed)
        masks = {(t, l): (rng.random(Fn) < 0.05).astype(np.float64) for t in range(T) for l in range(L)}
        masks[(0, 1)] = np.zeros(0)               # empty list: no override in that call
        masks[(1, 0)] = np.zeros(Fn)
        masks[(1, 0)][Fn - 1] = 1.0               # only the last neuron
        mods = modules(C, seed, L, act, 0.0)
        with tempfile.TemporaryDirectory() as d:
            for (t, l), m in masks.items():
                with open(os.path.join(d, f"predictivity_{t}_{l}.json"), "w") as f:
                    json.dump(m.tolist(), f)
            rec = MG.quiet(rem_mod.RemoveNeurons, 0, d, T, L)
        outs, gates, tl = [], [], []
        for call in range(T * L):
            tl.append((rec.timestep, rec.layer))
            x = torch.from_numpy(synth.tokens((2, N, C), x_seed(seed, 0, 0, call))).half()
            with torch.no_grad():
                outs.append(rec.hook_fn(mods[call % L], (x,), None).numpy())
            gates.append(rec.gates[-1].numpy())
        full = {k: (m if m.size else np.zeros(Fn)) for k, m in masks.items()}
        mask_bits = np.stack([np.packbits(full[(t, l)].astype(bool), bitorder="little") for t in range(T)
                              for l in range(L)])
        cases.append(dict(
            name=f"neuron_remove_C{C}_{act}", kind="remove_neurons", dtype="float16", C=C, N=N, T=T, L=L, act=act,
            seed=seed, gate_bias=0.0, mask_bits=mask_bits.reshape(T, L, Fn // 8),
            mask_empty=np.array([[masks[(t, l)].size == 0 for l in range(L)] for t in range(T)]),
            calls=np.array(keep), call_tl=np.array([tl[c] for c in keep]), out=np.stack([outs[c] for c in keep]),
            gate=np.stack([gates[c] for c in keep]), counter_after=np.array([rec.timestep, rec.layer])))
    return cases


def gen_ttest(pred_case):
    """modularity/paired_t_test.py:72-79,142 on the neuron_pred statistics as that script reads them (JSON lists),
    and modularity/skilled_neuron_ap.py:166-172 on a hit-rate vector."""
    T, L, P = pred_case["T"], pred_case["L"], pred_case["P"]
    base = json.loads(pred_case["json_base"].tobytes())
    adj = json.loads(pred_case["json_adj"].tobytes())
    diff_std = json.loads(json.dumps({t: {l: pred_case["diff_std"][t][l].tolist() for l in range(L)}
                                      for t in range(T)}))
    criticals = [1.0, 2.132]  # 2.132: one-sided 95 % at 4 degrees of freedom
    tv, sk = [], []
    for t in range(T):
        for l in range(L):
            b = np.array(base['time_steps'][str(t)][str(l)]['avg'])
            a = np.array(adj['time_steps'][str(t)][str(l)]['avg'])
            d = np.array(diff_std[str(t)][str(l)])
            with np.errstate(divide="ignore", invalid="ignore"):
                t_value = (b - a) / (d / (P ** 0.5))
            tv.append(t_value)
            sk.append(np.stack([t_value < -c for c in criticals]))
    Fn = 4 * pred_case["C"]
    rng = np.random.default_rng(7300)
    hit = rng.permutation(Fn).astype(np.float64) / Fn  # distinct values: no ties for argsort to break
    pred_indices = hit.argsort()[::-1]
    mask = np.zeros(len(hit))
    mask[pred_indices[:int(0.05 * len(hit))]] = 1
    return [dict(name="neuron_ttest_C320_gelu", kind="neuron_ttest", dtype="float64", source=pred_case["name"], T=T,
                 L=L, P=P, criticals=np.array(criticals), t_value=np.stack(tv).reshape(T, L, Fn),
                 skilled=np.stack(sk).reshape(T, L, len(criticals), Fn), hit_rate=hit, ap_mask=mask, ap_ratio=0.05)]


def save(cases):
    for c in cases:
        name = c.pop("name")
        arrays = {k: (v if isinstance(v, np.ndarray) else np.array(v)) for k, v in c.items()}
        arrays["name"] = np.array(name)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}.npz  {os.path.getsize(path)} bytes")
        c["name"] = name


def main():
    MG.install_stubs()
    MG.load_ref("neuron_receivers.base_receiver", "neuron_receivers/base_receiver.py")
    utils = MG.load_ref("utils", "utils.py")
    pred = MG.load_ref("neuron_receivers.predictivity", "neuron_receivers/predictivity.py")
    bb = MG.load_ref("neuron_receivers.neuron_predictivity_bb", "neuron_receivers/neuron_predictivity_bb.py")
    rem = MG.load_ref("neuron_receivers.remove_skilled_neurons", "neuron_receivers/remove_skilled_neurons.py")
    pred_cases = gen_neuron_pred(pred, utils)
    cases = pred_cases + gen_neuron_pred_bb(bb, utils) + gen_remove_neurons(rem) + gen_ttest(pred_cases[0])
    save(cases)


if __name__ == "__main__":
    main()
