"""Golden vectors for the expert-level discovery path, made by running the REFERENCE's own receivers and statistics.

Runs only in the build container (the reference tree is not present on the GPU box). Through make_golden's stub of
the absent `diffusers` package it imports, from the reference tree,
  * ExpertPredictivity.hook_fn     neuron_receivers/expert_activation.py:46-63
  * FrequencyMeasure.hook_fn       neuron_receivers/frequency_measure.py:42-64
  * helper.modify_ffn              moefication/helper.py:48-62 (labels -> patterns, k)
  * utils.StatMeter / StandardDev (utils.py:233-317), driven as modularity/modularity_analysis.py:63-110 drives them
    (reset_time_layer per prompt, a paired StandardDev over base - adj maxima, StatMeter.save)
  * update_expert_counter          modularity/moefy_skilled_experts.py:23-36 (the loop of freq_expert_select.py:61-64)
and runs them on the CPU in fp16 on seeded inputs. Only data is written (seeds, recorded outputs, statistics); the
tests regenerate x and the weights from the seeds with synth.py. The expert t-test follows the one formula of
modularity/paired_t_test_experts.py:57-61 on the saved JSON.

Both reference receivers wrap their counter at layer 15 whatever n_layers is, so the generator sets rec.timestep /
rec.layer before every hooked call instead of relying on it.
The token seeds of the expert_freq fixtures are searched per hooked call so that at most 5 % of the image-0 rows are
near-tie rows under test_gpu_route_parity.near_tie_rows(score, k, slack_ulps=8): the device GEMM's summation order may
legitimately reorder such a row's k-th and (k+1)-th experts, and the tests' tolerance is stated in that count.

Fixture kinds: expert_pred, expert_freq, expert_ttest, expert_counter. index.json is left alone.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_expert_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(OUT)
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402
import synth  # noqa: E402
from make_neuron_golden import meter_state, save, saved_json, x_seed  # noqa: E402

TOPK = 0.2
NEAR_CAP = 0.05


def near_tie_rows():
    """tests/test_gpu_route_parity.near_tie_rows (the project's one definition), imported from the test tree."""
    for p in (os.path.join(os.path.dirname(TESTS), "diffusion-models-moe_amd"), TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    import test_gpu_route_parity
    return test_gpu_route_parity.near_tie_rows


def modules(helper, C, seed, L, act, gate_bias):
    """L fp16 GEGLUs MoE-fied by the reference's modify_ffn with one balanced label set (E = 4C / 20, k = int(E *
    TOPK))."""
    E = 4 * C // 20
    labels = synth.balanced_labels(4 * C, E, seed)
    mods = [MG.make_geglu(C, seed + l, torch.float16, gate_bias=gate_bias) for l in range(L)]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "labels")
        torch.save(list(map(int, labels)), path)
        for m in mods:
            if act == "relu":
                m.gelu = F.relu
            MG.quiet(helper.modify_ffn, m, path, TOPK)
    return mods, labels, E


def gen_expert_pred(helper, ea_mod, utils):
    cases = []
    T, L, P = 2, 2, 3
    spec = [(320, 32, "relu", 0.0), (320, 32, "gelu", 0.0), (320, 32, "gelu", -3.0), (1280, 8, "gelu", 0.0)]
    for i, (C, N, act, gb) in enumerate(spec):
        seed = 8000 + 10 * i
        mods, labels, E = modules(helper, C, seed, L, act, gb)
        recs = [MG.quiet(ea_mod.ExpertPredictivity, 0, T, L) for _ in range(2)]
        diff = {t: {l: utils.StandardDev() for l in range(L)} for t in range(T)}
        maxima, out0 = [[], []], None
        for p in range(P):
            for kind, rec in enumerate(recs):
                rec.reset_time_layer()
                for call in range(T * L):
                    rec.timestep, rec.layer = call // L, call % L
                    x = torch.from_numpy(synth.tokens((2, N, C), x_seed(seed, p, kind, call))).half()
                    with torch.no_grad():
                        o = rec.hook_fn(mods[call % L], (x,), None)
                    if out0 is None:
                        out0 = o.numpy()
                maxima[kind].append(np.stack([np.stack([rec.max_gate[t][l] for l in range(L)]) for t in range(T)]))
            for t in range(T):
                for l in range(L):
                    diff[t][l].update(recs[0].max_gate[t][l] - recs[1].max_gate[t][l])
        mb, ma = np.stack(maxima[0]), np.stack(maxima[1])
        assert mb.dtype == np.float16 and mb.shape == (P, T, L, E)
        if gb < 0:
            # experts whose score is negative on every row of a prompt: a zero-initialised maximum would miss them
            assert (mb < 0).any() and (ma < 0).any()
            print(f"  gate_bias {gb}: {float((mb < 0).mean()):.2f} of the base maxima are negative")
        sb, meanb, m2b, nb = meter_state(recs[0].predictivity, T, L)
        sa, meana, m2a, na = meter_state(recs[1].predictivity, T, L)
        dmean = np.stack([np.stack([diff[t][l].mean for l in range(L)]) for t in range(T)])
        dm2 = np.stack([np.stack([diff[t][l].M2 for l in range(L)]) for t in range(T)])
        dstd = np.stack([np.stack([diff[t][l].stddev() for l in range(L)]) for t in range(T)])
        jb, ja = saved_json(recs[0].predictivity), saved_json(recs[1].predictivity)
        cases.append(dict(
            name=f"expert_pred_C{C}_{act}_gb{gb}", kind="expert_pred", dtype="float16", C=C, N=N, T=T, L=L, P=P, E=E,
            act=act, seed=seed, gate_bias=gb, topk=TOPK, labels=labels, max_gate_base=mb, max_gate_adj=ma, sum_base=sb,
            mean_base=meanb, M2_base=m2b, n_base=nb, sum_adj=sa, mean_adj=meana, M2_adj=m2a, n_adj=na, json_base=jb,
            json_adj=ja, diff_mean=dmean, diff_M2=dm2, diff_std=dstd, out0=out0))
    return cases


def gen_expert_freq(helper, fm_mod):
    """Six hooked calls: calls 0-3 fill the (t, l) grid of T = L = 2, calls 4 and 5 hit (0, 0) and (0, 1) again, so
    the counters accumulate."""
    near = near_tie_rows()
    cases = []
    T, L = 2, 2
    tl = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 0), (0, 1)]
    spec = [(320, 32, "relu"), (320, 32, "gelu"), (640, 8, "relu"), (1280, 8, "gelu")]
    for i, (C, N, act) in enumerate(spec):
        seed = 8100 + 10 * i
        mods, labels, E = modules(helper, C, seed, L, act, 0.0)
        k = int(mods[0].k)
        names = [f"ffn{l}" for l in range(L)]
        rec = MG.quiet(fm_mod.FrequencyMeasure, 0, T, L, {n: E for n in names}, names)
        x_seeds, outs, scores, labs, n_near = [], [], [], [], []
        for call, (t, l) in enumerate(tl):
            m = mods[l]
            xs = seed + 1000 + 1000000 * call  # (the searches of two calls never meet)
            while True:  # the first token seed whose image-0 rows stay under the near-tie cap
                x = torch.from_numpy(synth.tokens((2, N, C), xs)).half()
                with torch.no_grad():
                    gate = m.gelu(m.proj(x).chunk(2, dim=-1)[1])
                    score = torch.matmul(gate.view(-1, 4 * C), m.patterns.transpose(0, 1)).view(2, N, E)
                nn_ = int(near(score[0].numpy(), k, slack_ulps=8).sum())
                if nn_ <= NEAR_CAP * N:
                    break
                xs += 1
            rec.timestep, rec.layer = t, l
            with torch.no_grad():
                out = rec.hook_fn(m, (x,), None)
            x_seeds.append(xs)
            n_near.append(nn_)
            scores.append(score[0].numpy())
            labs.append(torch.topk(score, k=k, dim=-1)[1][0].numpy())
            if call == 0:
                outs.append(out.numpy())
        lc = np.stack([np.stack([rec.label_counter[t][l] for l in range(L)]) for t in range(T)])
        assert lc.dtype == np.float64 and np.allclose(lc.sum(-1), [[2 * k, 2 * k], [k, k]])
        cases.append(dict(
            name=f"expert_freq_C{C}_{act}", kind="expert_freq", dtype="float16", C=C, N=N, T=T, L=L, E=E, k=k, act=act,
            seed=seed, gate_bias=0.0, topk=TOPK, labels=labels, call_tl=np.array(tl), x_seeds=np.array(x_seeds),
            n_near=np.array(n_near), label_counter=lc, out0=outs[0], score0=np.stack(scores), labels0=np.stack(labs)))
        print(f"  expert_freq_C{C}_{act}: token seeds {x_seeds}, near-tie rows {n_near}")
    return cases


def gen_ttest(pred_case):
    """paired_t_test_experts.py:51-61 on the expert_pred statistics as that script reads them (JSON lists). The
    critical value is the first of a fixed list that leaves the lists neither all empty nor any of them full."""
    T, L, P, E = (int(pred_case[k]) for k in ("T", "L", "P", "E"))
    base = json.loads(pred_case["json_base"].tobytes())
    adj = json.loads(pred_case["json_adj"].tobytes())
    diff_std = json.loads(json.dumps({t: {l: pred_case["diff_std"][t][l].tolist() for l in range(L)}
                                      for t in range(T)}))
    for critical in (3.579, 2.92, 1.886, 1.0, 0.5):  # 2.92 / 1.886: one-sided 95 % / 90 % at 2 degrees of freedom
        lists, tv = {}, []
        for t in range(T):
            for l in range(L):
                b = np.array(base['time_steps'][str(t)][str(l)]['avg'])
                a = np.array(adj['time_steps'][str(t)][str(l)]['avg'])
                d = np.array(diff_std[str(t)][str(l)])
                with np.errstate(divide="ignore", invalid="ignore"):
                    t_value = (b - a) / (d / P ** 0.5)
                skilled = torch.where(torch.tensor(t_value < -critical))[0]
                lists[f"{t},{l}"] = skilled.tolist()
                tv.append(t_value)
        tv = np.stack(tv)
        sizes = [len(v) for v in lists.values()]
        if any(sizes) and max(sizes) < E and np.all(np.abs(tv[np.isfinite(tv)] + critical) > 1e-6):
            break
    else:
        raise SystemExit("no critical value of the list separates the experts")
    return [dict(name=f"expert_ttest_C{int(pred_case['C'])}_{str(pred_case['act'])}", kind="expert_ttest",
                 dtype="float64", source=pred_case["name"], T=T, L=L, P=P, E=E, critical=critical,
                 t_value=tv.reshape(T, L, E), lists=json.dumps(lists))]


def gen_expert_counter(update_expert_counter):
    T, num = 2, 3
    names = ["down.ffn0", "mid.ffn1"]
    experts = {names[0]: 64, names[1]: 256}
    rng = np.random.default_rng(8300)
    args = types.SimpleNamespace(timesteps=T)
    counter = update_expert_counter(args, names, experts, init=True)
    lcs = []
    for s in range(num):
        # selection fractions as FrequencyMeasure leaves them: multiples of 1 / seq_len, and one odd sequence length
        seq = [64, 100, 1024][s]
        lc = {t: {l: rng.integers(0, seq + 1, experts[n]).astype(np.float64) * (1.0 / seq)
                  for l, n in enumerate(names)} for t in range(T)}
        counter = update_expert_counter(args, names, experts, label_counter=lc, expert_counter=counter,
                                        num_samples=num)
        lcs.append(lc)
    blob = np.frombuffer(json.dumps(counter).encode(), dtype=np.uint8).copy()
    return [dict(name="expert_counter_3x", kind="expert_counter", dtype="float64", T=T, num_images=num,
                 names=np.array(names), topk=TOPK,
                 lc_l0=np.stack([np.stack([lc[t][0] for t in range(T)]) for lc in lcs]),
                 lc_l1=np.stack([np.stack([lc[t][1] for t in range(T)]) for lc in lcs]),
                 ec_l0=np.array([counter[t][names[0]] for t in range(T)], dtype=np.float64),
                 ec_l1=np.array([counter[t][names[1]] for t in range(T)], dtype=np.float64), json=blob)]


def load_update_expert_counter(helper, ge):
    """modularity/moefy_skilled_experts.py imports the whole driver stack at module level; the two modules it cannot
    import here (LLaVA prompts, cluster loading) are stubbed with empty stand-ins, the function itself is the
    reference's."""
    sys.modules["helper"] = helper
    sys.modules["neuron_receivers"].GetExperts = ge.GetExperts
    sys.modules["greater"] = types.SimpleNamespace(load_expert_clusters=None)
    sys.modules["mod_utils"] = types.SimpleNamespace(get_prompts=None, update_set_diff=None)
    return MG.load_ref("moefy_skilled_experts_ref", "modularity/moefy_skilled_experts.py").update_expert_counter


def main():
    MG.install_stubs()
    helper = MG.load_ref("moefication_helper_ref", "moefication/helper.py")
    MG.load_ref("neuron_receivers.base_receiver", "neuron_receivers/base_receiver.py")
    utils = MG.load_ref("utils", "utils.py")
    ea = MG.load_ref("neuron_receivers.expert_activation", "neuron_receivers/expert_activation.py")
    fm = MG.load_ref("neuron_receivers.frequency_measure", "neuron_receivers/frequency_measure.py")
    ge = MG.load_ref("neuron_receivers.get_experts", "neuron_receivers/get_experts.py")
    pred_cases = gen_expert_pred(helper, ea, utils)
    gelu = [c for c in pred_cases if c["act"] == "gelu" and c["gate_bias"] == 0.0 and c["C"] == 320][0]
    cases = pred_cases + gen_expert_freq(helper, fm)
    gelu_arrays = {k: (v if isinstance(v, np.ndarray) else np.array(v)) for k, v in gelu.items()}
    cases += gen_ttest(gelu_arrays) + gen_expert_counter(load_update_expert_counter(helper, ge))
    save(cases)


if __name__ == "__main__":
    main()
