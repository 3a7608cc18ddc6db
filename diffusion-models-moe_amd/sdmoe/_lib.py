"""ctypes binding of libsdmoe_hip.so (the C ABI declared in include/sdmoe.h).

The product path has exactly one compute backend: these HIP kernels. If the shared library is missing or
fails to load, every op raises -- there is no eager-PyTorch or CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsdmoe_hip.so")

_P = ctypes.c_void_p
_L = ctypes.c_long
_I = ctypes.c_int
_F = ctypes.c_float
_FP = ctypes.POINTER(ctypes.c_float)
_IP = ctypes.POINTER(ctypes.c_int)

# name -> argtypes, in the exact order of include/sdmoe.h
SIGNATURES = {
    "sdmoe_linear": [_P, _L, _P, _L, _P, _P, _L, _I, _P, _L, _P, _L, _I, _I, _I, _I, _P, _L, _P],
    "sdmoe_conv3x3": [_P, _L, _I, _I, _I, _I, _P, _P, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _P, _L, _P],
    "sdmoe_conv3x3_sc": [_P, _L, _I, _I, _I, _I, _P, _P, _P, _L, _P, _L, _I, _P, _L, _I, _I, _P, _L, _P],
    "sdmoe_conv3x3_gn": [_P, _L, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _L, _P, _L, _P, _L, _I, _P, _L, _I, _P, _L,
                         _P],
    # (callers probe sdmoe_conv_up2x with has(): an SDMOE_AB=1 library from before it takes sdmoe_conv3x3's upsample path)
    "sdmoe_conv_up2x": [_P, _L, _I, _I, _I, _I, _P, _P, _P, _L, _I, _P, _L, _P],
    "sdmoe_conv_up2x_plan": [_I, _I, _I, _I, _I, _L, _P],
    "sdmoe_groupnorm_apply": [_P, _L, _I, _I, _I, _P, _P, _I, _P, _L, _P],
    "sdmoe_mask_weight": [_P, _P, _L, _L, _P, _P],
    "sdmoe_groupnorm_stats": [_P, _L, _I, _I, _I, _I, _P, _P, _F, _P, _P, _P, _L, _P],
    "sdmoe_groupnorm": [_P, _L, _I, _I, _I, _I, _P, _P, _F, _I, _P, _L, _P, _P, _P, _L, _P],
    "sdmoe_gn_fold": [_P, _L, _I, _I, _P, _P, _P, _I, _P, _P, _P],
    "sdmoe_linear_per_image": [_P, _L, _P, _L, _L, _P, _L, _I, _P, _L, _P, _L, _I, _I, _I, _P, _L, _P],
    "sdmoe_layernorm": [_P, _L, _P, _L, _I, _I, _P, _P, _F, _P],
    "sdmoe_ln_fold": [_P, _L, _I, _I, _P, _P, _P, _P, _L, _P, _P, _P],
    "sdmoe_linear_ln": [_P, _L, _P, _L, _P, _P, _F, _P, _L, _I, _I, _I, _P],
    "sdmoe_linear_geglu_ln": [_P, _L, _P, _L, _P, _P, _F, _P, _L, _I, _I, _I, _I, _P, _L, _I, _P],
    "sdmoe_attention": [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _F, _P],
    "sdmoe_geglu_route": [_P, _L, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P],
    "sdmoe_score_bias": [_P, _L, _I, _I, _P, _P, _L, _P],
    "sdmoe_geglu_route_bias": [_P, _L, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P, _P],
    "sdmoe_linear_geglu": [_P, _L, _P, _L, _P, _P, _L, _I, _I, _I, _I, _P, _L, _I, _P],
    "sdmoe_moe_topk_mask": [_P, _L, _I, _I, _I, _I, _I, _P, _L, _P, _P, _P],
    "sdmoe_moe_topk_keep": [_I, _I, _I, _I, _I, _P, _L, _P, _P, _P, _P],
    "sdmoe_linear_keep": [_P, _L, _P, _P, _L, _P, _P, _L, _P, _L, _I, _I, _I, _P, _L, _P],
    "sdmoe_linear_masked": [_P, _L, _P, _P, _L, _P, _P, _P, _L, _P, _L, _I, _I, _I, _P, _L, _P],
    "sdmoe_linear_masked_sets": [_P, _L, _P, _P, _L, _P, _L, _P, _I, _I, _P, _P, _L, _P, _L, _I, _I, _I, _P, _L, _P],
    "sdmoe_gemm_plan_sets": [_I, _I, _I, _I, _I, _I, _L, _P],
    "sdmoe_wmask_union_sets": [_P, _L, _I, _P, _I, _L, _P, _P],
    "sdmoe_gemm_plan": [_I, _I, _I, _I, _I, _I, _L, _P],
    "sdmoe_conv_plan": [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _L, _P],
    "sdmoe_wmask_kmajor": [_P, _L, _I, _I, _P, _P, _P],
    "sdmoe_timestep_embedding": [_P, _P, _F, _I, _I, _F, _P],
    "sdmoe_cfg_multistep_step": [_P, _L, _P, _I, _I, _I, _F, _P, _P, _P, _P, _P, _L, _P],
    "sdmoe_sqdist_f32": [_P, _L, _P, _L, _I, _I, _I, _P, _L, _P],
    "sdmoe_balanced_assign": [_P, _I, _I, ctypes.c_double, _P, _I, _P],
    "sdmoe_expert_mean_topk": [_P, _L, _I, _I, _I, _P, _I, _I, _P, _P, _P, _L, _P],
    "sdmoe_colnorm_accum": [_P, _L, _I, _I, _P, _P, _L, _P],
    "sdmoe_wanda_mask": [_P, _L, _I, _I, _P, _P, _I, _P, _P],
    "sdmoe_union_over_time": [_P, _L, _I, _L, _F, _P, _P],
    "sdmoe_geglu_neurons": [_P, _L, _I, _I, _I, _P, _F, _P, _L, _P, _L, _I, _P, _I, _P, _P, _P, _L, _P],
    "sdmoe_expert_stats": [_P, _L, _P, _I, _I, _I, _P, _I, _P, _P, _P, _L, _P],
    "sdmoe_geglu_sparsity": [_P, _L, _I, _I, _I, _F, _P, _L, _P, _L, _I, _P, _I, _P, _P, _P, _P, _L, _P],
    "sdmoe_noise_capture": [_P, _L, _P, _L, _L, _P],
    "sdmoe_noise_distance": [_P, _L, _L, _P, _L, _L, _I, _I, _I, _P, _I, _P, _P, _L, _P],
    "sdmoe_clip_quantise": [_P, _I, _I, _I, _I, _P, _P],
    "sdmoe_clip_resample_h": [_P, _L, _I, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P],
    "sdmoe_clip_resample_v": [_P, _I, _I, _I, _P, _P, _I, _I, _I, _FP, _FP, _P, _P, _L, _I, _P],
    "sdmoe_clip_scores": [_P, _L, _P, _L, _P, _L, _I, _I, _P, _P],
    "sdmoe_stem_rows": [_P, _I, _I, _FP, _FP, _P, _L, _I, _P],
    "sdmoe_maxpool3x3s2": [_P, _L, _I, _I, _I, _I, _P, _L, _P],
    "sdmoe_avgpool_rows": [_P, _L, _I, _I, _I, _P, _L, _P],
    "sdmoe_add_relu": [_P, _P, _P, _L, _P],
    "sdmoe_topk_hits": [_P, _L, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P],
    "sdmoe_text_pool": [_P, _L, _I, _I, _I, _I, _I, _P, _L, _P],
    "sdmoe_concept_route": [_P, _L, _I, _I, _I, _P, _L, _I, _P, _P, _I, _P, _P, _P, _P],
    "sdmoe_softmax_rows": [_P, _L, _P, _L, _I, _I, _P],
    "sdmoe_transpose": [_P, _L, _P, _L, _I, _I, _P],
    "sdmoe_gather_rows": [_P, _L, _P, _I, _I, _P, _L, _I, _P, _L, _P],
    "sdmoe_attention_short": [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _F, _I, _P],
    "sdmoe_timestep_embedding_rows": [_P, _L, _P, _I, _I, _I, _I, _F, _P],
    "sdmoe_prepare_input": [_P, _P, _I, _I, _L, _I, _P],
    "sdmoe_cfg_ddim_step": [_P, _L, _P, _I, _I, _I, _F, _F, _F, _P, _L, _P],
    "sdmoe_cfg_x0_step": [_P, _L, _P, _I, _I, _I, _F, _P, _P, _P, _P, _L, _P],
    "sdmoe_prepare_input_scaled": [_P, _P, _I, _I, _L, _I, _F, _F, _P],
    "sdmoe_add": [_P, _P, _P, _L, _P],
    "sdmoe_tune": [_I, _I],
    "sdmoe_tune_knob": [_I, _IP, ctypes.POINTER(ctypes.c_char_p), _IP, _IP],
    "sdmoe_tune_reset": [],
    "sdmoe_set_gelu_table": [_P],
    "sdmoe_version": [],
}

ERRORS = {-1: "bad pointer/size", -2: "unsupported shape/alignment", -3: "unsupported mode"}

_lib = None


class SdmoeError(RuntimeError):
    pass


def load(path: str | None = None):
    """Load (once) and return the library with typed entry points. Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    p = path or os.environ.get("SDMOE_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise SdmoeError(
            f"libsdmoe_hip.so not found at {p}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C diffusion-models-moe_amd/csrc`). There is no CPU fallback."
        )
    lib = ctypes.CDLL(p)
    # same-box A/B against an older build (SDMOE_AB=1, with SDMOE_LIB naming it): entry points it lacks stay unbound
    # and the callers that probe with has() take their older path; otherwise a missing symbol is an error
    ab_lib = os.environ.get("SDMOE_AB", "0") == "1"
    for name, argt in SIGNATURES.items():
        if ab_lib and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes = argt
        fn.restype = ctypes.c_char_p if name == "sdmoe_version" else ctypes.c_int
    # A/B experiments without code changes: SDMOE_TUNE="knob=value,..." (sdmoe_tune, include/sdmoe.h)
    for k, v in parse_tune(os.environ.get("SDMOE_TUNE", ""), lib):
        check(lib.sdmoe_tune(k, v), f"sdmoe_tune({k}={v})")
    _lib = lib
    return lib


def knob_table(lib=None):
    """The library's knob table (sdmoe_tune_knob): [(id, name, default, value)]. An SDMOE_AB=1 library from before the
    table raises: no copy of it is kept here."""
    lib = lib or load()
    if not has(lib, "sdmoe_tune_knob"):
        raise SdmoeError("this library has no sdmoe_tune_knob (an older SDMOE_AB=1 build): its knobs can be set by id "
                         "through sdmoe_tune / SDMOE_TUNE only, not named, read or restored")
    rows = []
    kid, dflt, val, name = _I(), _I(), _I(), ctypes.c_char_p()
    while lib.sdmoe_tune_knob(len(rows), kid, name, dflt, val) == 0:
        rows.append((kid.value, name.value.decode(), dflt.value, val.value))
    return rows


def parse_tune(spec: str, lib=None):
    """SDMOE_TUNE="knob=value,..." -> [(id, value)], knob an id or a name of the library's table (`lib`: the library to
    look names up in, default load()); malformed entries raise SdmoeError (not a bare ValueError)."""
    out = []
    for kv in filter(None, (s.strip() for s in spec.split(","))):
        parts = [s.strip() for s in kv.split("=")]
        if len(parts) != 2:
            raise SdmoeError(f"SDMOE_TUNE entry {kv!r}: expected knob=value")
        try:
            value = int(parts[1])
            knob = int(parts[0]) if not parts[0].isidentifier() else None
        except ValueError:
            raise SdmoeError(f"SDMOE_TUNE entry {kv!r}: knob must be an id or a name, value an integer") from None
        if knob is None:
            ids = {name: kid for kid, name, _, _ in knob_table(lib)}
            if parts[0] not in ids:
                raise SdmoeError(f"SDMOE_TUNE entry {kv!r}: no knob named {parts[0]!r} (known: {', '.join(ids)})")
            knob = ids[parts[0]]
        out.append((knob, value))
    return out


def has(lib, name: str) -> bool:
    """Whether the loaded library exports `name` (only an SDMOE_AB=1 build may lack one)."""
    return hasattr(lib, name)


def check(status: int, what: str):
    if status != 0:
        msg = ERRORS.get(status, f"hipError_t {status}")
        raise SdmoeError(f"{what} failed: {msg} ({status})")
