"""Golden vectors for the HPO path, made by running the REFERENCE's own receivers.

Runs only in the build container (the reference tree is not present on the GPU box). Through make_golden's stub of
the absent `diffusers` package it imports, from the reference tree,
  * RemoveNeuronsHPO.hook_fn                       neuron_receivers/remove_skilled_neurons_hpo.py:28-73
  * RemoveNeuronsNoiseHPO.hook_fn / unet_hook_fn   neuron_receivers/remove_skilled_neurons_noise_hpo.py:41-82
  * BaseUNetReceiver.unet_hook_fn                  neuron_receivers/base_unet_receiver.py:25-29
  * SaveStates.hook_fn                             neuron_receivers/save_states.py:20-30
  * utils.Average                                  utils.py (the driver's per-step running mean)
and runs them on the CPU in fp16 on seeded inputs (C = 320, a few tokens), the HPO receiver under a fake trial that
answers from a recorded list. Only data is written (seeds, masks, answers, recorded outputs); the tests regenerate x
and the weights from the seeds with synth.py.
The noise fixture applies lines 75-84 of modularity/remove_experts_noise_hpo.py (compiled from the reference tree; the
driver's bookkeeping around them, :40-45, :73-87, :124-128, is restated here) to seeded [2, 4, 8, 8] fp16 tensors
twice: (i) literally, on the fp16 CPU tensors, and (ii) on the same tensors upcast to float64. Tests assert against
(ii); (i) is recorded to state the size of the reference's fp16 rounding.

Fixture kinds: hpo_remove, hpo_noise_remove, base_unet, save_states, noise_objective. index.json is left alone.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_hpo_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import textwrap

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402
import synth  # noqa: E402
from make_neuron_golden import modules, save, x_seed  # noqa: E402

DOF, CONF = 9, 0.95


class FakeTrial:
    """Stands in for optuna's trial: answers suggest_categorical from a recorded {name: value} list."""

    def __init__(self, answers):
        self.answers = answers
        self.asked = []

    def suggest_categorical(self, name, choices):
        self.asked.append(name)
        assert self.answers[name] in choices
        return self.answers[name]


def write_masks(d, masks):
    folder = os.path.join(d, f"dof_{DOF}_conf_{CONF}")
    os.makedirs(folder)
    for (t, l), m in masks.items():
        with open(os.path.join(folder, f"timestep_{t}_layer_{l}.json"), "w") as f:
            json.dump(m.tolist(), f)


def random_masks(seed, T, L, Fn, empty=()):
    rng = np.random.default_rng(seed)
    masks = {(t, l): (rng.random(Fn) < 0.05).astype(np.float64) for t in range(T) for l in range(L)}
    for tl in empty:
        masks[tl] = np.zeros(0)
    return masks


def packed(masks, T, L, Fn):
    full = {k: (m if m.size else np.zeros(Fn)) for k, m in masks.items()}
    bits = np.stack([np.packbits(full[(t, l)].astype(bool), bitorder="little") for t in range(T) for l in range(L)])
    empty = np.array([[masks[(t, l)].size == 0 for l in range(L)] for t in range(T)])
    return bits.reshape(T, L, Fn // 8), empty


def run_calls(rec, mods, seed, T, L, N, C, keep, unet_every=None):
    outs, gates, tl = [], [], []
    for call in range(T * L):
        tl.append((rec.timestep, rec.layer))
        x = torch.from_numpy(synth.tokens((2, N, C), x_seed(seed, 0, 0, call))).half()
        with torch.no_grad():
            o = rec.hook_fn(mods[call % L], (x,), None).numpy()
        if call in keep:
            outs.append(o)
            gates.append((rec.gates[-1] if rec.gates else rec.hidden_states[tl[-1][0]][tl[-1][1]]).numpy())
        if unet_every is not None and call % L == L - 1:
            unet_every(call // L)
    return np.stack(outs), np.stack(gates), np.array([tl[c] for c in keep])


def gen_hpo_remove(hpo_mod):
    """T = 12 so that timesteps 10 and 11 ask the trial; two answer lists, each holding a 0 and a 1."""
    cases = []
    C, N, T, L = 320, 4, 12, 2
    Fn = 4 * C
    keep = [0, 1, 18, 20, 21, 22, 23]  # (0, 0), (0, 1) empty, (9, 0), and every call of timesteps 10 and 11
    for i, (act, ans) in enumerate([("gelu", (0, 1)), ("relu", (1, 0))]):
        seed = 7400 + 10 * i
        masks = random_masks(seed, T, L, Fn, empty=[(0, 1)])
        mods = modules(C, seed, L, act, 0.0)
        trial = FakeTrial({"timestep_10": ans[0], "timestep_11": ans[1]})
        with tempfile.TemporaryDirectory() as d:
            write_masks(d, masks)
            rec = MG.quiet(hpo_mod.RemoveNeuronsHPO, 0, d, T, L, DOF, CONF, trials_per_layer=trial)
        out, gate, tl = run_calls(rec, mods, seed, T, L, N, C, keep)
        assert trial.asked == ["timestep_10", "timestep_11"]
        bits, empty = packed(masks, T, L, Fn)
        cases.append(dict(
            name=f"hpo_remove_C{C}_{act}", kind="hpo_remove", dtype="float16", C=C, N=N, T=T, L=L, act=act, seed=seed,
            gate_bias=0.0, dof=DOF, conf=CONF, mask_bits=bits, mask_empty=empty, answers=np.array(ans),
            asked=np.array(trial.asked), update_for_t=np.array([rec.update_for_t[t] for t in range(T)]),
            calls=np.array(keep), call_tl=tl, out=out, gate=gate, counter_after=np.array([rec.timestep, rec.layer])))
    return cases


def unet_tensor(seed, t):
    return torch.from_numpy(synth.tokens((2, 4, 8, 8), seed + 500 + t)).half()


def gen_hpo_noise_remove(noise_mod):
    """The override at every timestep (the trial is never asked); unet_hook_fn after each timestep's last layer stores
    the step under the reference's `timestep - 1`."""
    C, N, T, L = 320, 4, 2, 2
    Fn, seed = 4 * C, 7500
    masks = random_masks(seed, T, L, Fn, empty=[(1, 0)])
    mods = modules(C, seed, L, "gelu", 0.0)
    trial = FakeTrial({})
    with tempfile.TemporaryDirectory() as d:
        write_masks(d, masks)
        rec = MG.quiet(noise_mod.RemoveNeuronsNoiseHPO, 0, d, T, L, DOF, CONF, trials_per_layer=trial)
    keep = list(range(T * L))
    out, gate, tl = run_calls(rec, mods, seed, T, L, N, C, keep,
                              unet_every=lambda t: rec.unet_hook_fn(None, None, (unet_tensor(seed, t),)))
    assert trial.asked == [] and rec.update_for_t == {}
    stored = np.stack([rec.unet_output[t].numpy() for t in range(T)])
    assert stored.dtype == np.float16 and stored.shape == (T, 2, 4, 8, 8)
    bits, empty = packed(masks, T, L, Fn)
    rec.reset_time_layer()
    assert all(rec.unet_output[t] == [] for t in range(T))
    return [dict(name=f"hpo_noise_remove_C{C}_gelu", kind="hpo_noise_remove", dtype="float16", C=C, N=N, T=T, L=L,
                 act="gelu", seed=seed, gate_bias=0.0, dof=DOF, conf=CONF, mask_bits=bits, mask_empty=empty,
                 calls=np.array(keep), call_tl=tl, out=out, gate=gate, unet_output=stored)]


def gen_base_unet(base_mod):
    T, L, seed = 3, 2, 7600
    rec = MG.quiet(base_mod.BaseUNetReceiver, 0, T, L)
    for t in range(T):
        assert rec.timestep == t
        rec.unet_hook_fn(None, None, (unet_tensor(seed, t),))
    stored = np.stack([rec.unet_output[t].numpy() for t in range(T)])
    after = rec.timestep
    rec.reset_time()
    assert rec.timestep == 0 and all(rec.unet_output[t] == [] for t in range(T))
    return [dict(name="base_unet_steps", kind="base_unet", dtype="float16", T=T, L=L, seed=seed, unet_output=stored,
                 timestep_after=after)]


def gen_save_states(ss_mod):
    C, N, T, L, seed = 320, 4, 2, 2, 7700
    mods = modules(C, seed, L, "gelu", 0.0)
    rec = MG.quiet(ss_mod.SaveStates, 0, T, L)
    keep = list(range(T * L))
    out, gate, tl = run_calls(rec, mods, seed, T, L, N, C, keep)
    return [dict(name=f"save_states_C{C}_gelu", kind="save_states", dtype="float16", C=C, N=N, T=T, L=L, act="gelu",
                 seed=seed, gate_bias=0.0, calls=np.array(keep), call_tl=tl, out=out, gate=gate,
                 counter_after=np.array([rec.timestep, rec.layer]))]


def driver_step_code():
    """Lines 75-84 of the reference's modularity/remove_experts_noise_hpo.py (the body of its `for t` loop), compiled
    from the reference tree: the driver itself cannot be imported (it loads a model at import)."""
    with open(os.path.join(MG.REF, "modularity", "remove_experts_noise_hpo.py")) as f:
        lines = f.readlines()[74:84]
    assert lines[0].strip().startswith("diff = torch.norm(") and "noise_diff_per_sample[iter] +=" in lines[-1], lines
    return compile(textwrap.dedent("".join(lines)), "remove_experts_noise_hpo.py:75-84", "exec")


def driver_lines(code, sample, unet_outputs, unet_outputs_adj, noise_diff, T):
    """The driver's loop (:73-87) for one sample: its own lines update noise_diff[t] and noise_diff_per_sample; returns
    (the per-step torch.norm values, the per-step normalised distances, noise_diff_per_sample of the sample)."""
    noise_diff_per_sample = {sample: 0.0}
    l2, l1n = [], []
    for t in range(T):
        ns = dict(torch=torch, unet_outputs=unet_outputs, unet_outputs_adj=unet_outputs_adj, noise_diff=noise_diff,
                  noise_diff_per_sample=noise_diff_per_sample, iter=sample, t=t)
        exec(code, ns)
        l2.append(ns["diff"])
        l1n.append(torch.norm(ns["u1"] - ns["u2"]).item())
    noise_diff_per_sample[sample] /= T
    return l2, l1n, noise_diff_per_sample[sample]


def gen_noise_objective(utils):
    P, T, seed = 3, 4, 7800
    rng = np.random.default_rng(seed)
    a = torch.from_numpy(rng.standard_normal((P, T, 2, 4, 8, 8)).astype(np.float32)).half()
    b = (a.float() + 0.05 * torch.from_numpy(rng.standard_normal((P, T, 2, 4, 8, 8)).astype(np.float32))).half()
    b[0, 1] = a[0, 1]                      # a step without any difference
    b[1, 2] = a[1, 2]
    b[1, 2, 1, 3, 7, 7] = torch.nextafter(a[1, 2, 1, 3, 7, 7], torch.tensor(float("inf")).half())  # one fp16 ulp
    c = dict(name="noise_objective_2x4x8x8", kind="noise_objective", dtype="float64", P=P, T=T, seed=seed,
             a=a.numpy(), b=b.numpy())
    code = driver_step_code()
    for tag, cast in (("fp16", lambda x: x), ("fp64", lambda x: x.double())):
        noise_diff = {t: utils.Average() for t in range(T)}
        l2, l1n, per = [], [], []
        for p in range(P):
            r = driver_lines(code, p, [cast(a[p, t]) for t in range(T)], [cast(b[p, t]) for t in range(T)], noise_diff, T)
            l2.append(r[0])
            l1n.append(r[1])
            per.append(r[2])
        avg = 0.0
        for t in range(T):
            avg += noise_diff[t].avg
        avg /= T
        c[f"l2_{tag}"] = np.array(l2, dtype=np.float64)
        c[f"l1n_{tag}"] = np.array(l1n, dtype=np.float64)
        c[f"per_sample_{tag}"] = np.array(per, dtype=np.float64)
        c[f"avg_noise_diff_{tag}"] = np.float64(avg)
        c[f"step_avg_{tag}"] = np.array([noise_diff[t].avg for t in range(T)], dtype=np.float64)
    rel = np.abs(c["l1n_fp16"] - c["l1n_fp64"]) / np.maximum(c["l1n_fp64"], 1e-300)
    print("normalised distance, fp16 literal vs float64: relative gap per (sample, step)\n", rel)
    print("l1n fp16:\n", c["l1n_fp16"], "\nl1n fp64:\n", c["l1n_fp64"])
    print("torch.norm(a - b), fp16 vs float64: max relative gap",
          np.max(np.abs(c["l2_fp16"] - c["l2_fp64"]) / np.maximum(c["l2_fp64"], 1e-300)))
    return [c]


def main():
    MG.install_stubs()
    MG.load_ref("neuron_receivers.base_receiver", "neuron_receivers/base_receiver.py")
    utils = MG.load_ref("utils", "utils.py")
    MG.load_ref("neuron_receivers.predictivity", "neuron_receivers/predictivity.py")
    hpo = MG.load_ref("neuron_receivers.remove_skilled_neurons_hpo", "neuron_receivers/remove_skilled_neurons_hpo.py")
    noise = MG.load_ref("neuron_receivers.remove_skilled_neurons_noise_hpo",
                        "neuron_receivers/remove_skilled_neurons_noise_hpo.py")
    base = MG.load_ref("neuron_receivers.base_unet_receiver", "neuron_receivers/base_unet_receiver.py")
    ss = MG.load_ref("neuron_receivers.save_states", "neuron_receivers/save_states.py")
    save(gen_hpo_remove(hpo) + gen_hpo_noise_remove(noise) + gen_base_unet(base) + gen_save_states(ss) +
         gen_noise_objective(utils))


if __name__ == "__main__":
    main()
