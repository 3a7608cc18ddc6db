// Per-expert score bias for gfx950: the one line of the reference's AddExperts.hook_fn
//   score[:, expert_indx] = score[:, expert_indx] + 5.0 * std[expert_indx]
//                                                   (neuron_receivers/add_skilled_experts.py:55)
// as a streaming pass over the fp16 score buffer [M, E], between the kernel that produced it (sdmoe_linear_geglu's
// epilogue) and the top-k kernel that ranks it (sdmoe_moe_topk_keep / sdmoe_moe_topk_mask, unchanged, with a
// smaller k):
//   out[m, e] = fp16(score[m, e] + bias[e])      bias [E] fp16: 5 * std at the listed experts, +0 elsewhere
// An fp16 + fp16 sum is exact in fp32 (24 significand bits cover the widest exponent spread of two fp16 values that
// still interact), so the single round-to-nearest-even conversion gives the reference's fp16 add bit for bit.
// 2 M E 2 bytes of traffic and nothing else: no LDS, no atomics, vector stores only.
#include "common.h"
#include "../../include/sdmoe.h"

namespace {

typedef _Float16 half1 __attribute__((ext_vector_type(1)));

template <int V> struct HalfVec;
template <> struct HalfVec<8> { typedef half8 type; };
template <> struct HalfVec<1> { typedef half1 type; };

constexpr int BIAS_THREADS = 256;
constexpr int BIAS_UNROLL = 4;  // rows in flight per thread: 4 independent 16-B loads before the first store

// One thread owns one V-element column chunk (c = tid % C, C = E / V chunks per row) for the whole launch, so its
// slice of `bias` is read once and stays in registers; the workgroup's 256 threads cover RPB = 256 / C whole rows per
// pass (threads past RPB * C idle: at most C - 1 of them), which for contiguous rows are one contiguous, fully
// coalesced span. Grid-stride loop over row groups, BIAS_UNROLL groups per trip. out == score is fine: every thread
// reads exactly the elements it then writes. Columns >= E of a strided row are never touched.
// V = 8: 16-byte loads and stores (E, both leading dimensions multiples of 8, both pointers 16-byte aligned);
// V = 1: the scalar path for everything else.
template <int V>
__global__ __launch_bounds__(BIAS_THREADS) void score_bias_kernel(const half_t* score, long ld_score, int M, int C,
                                                                  const half_t* bias, half_t* out, long ld_out) {
  typedef typename HalfVec<V>::type vec_t;
  const int rpb = BIAS_THREADS / C;
  const int r = threadIdx.x / C, c = threadIdx.x - r * C;
  if (r >= rpb) return;
  const vec_t b = *reinterpret_cast<const vec_t*>(bias + V * c);
  const long step = (long)gridDim.x * rpb;
  for (long m0 = (long)blockIdx.x * rpb + r; m0 < M; m0 += BIAS_UNROLL * step) {
    vec_t v[BIAS_UNROLL];
#pragma unroll
    for (int u = 0; u < BIAS_UNROLL; ++u) {
      const long m = m0 + u * step;
      if (m < M) v[u] = *reinterpret_cast<const vec_t*>(score + m * ld_score + V * c);
    }
#pragma unroll
    for (int u = 0; u < BIAS_UNROLL; ++u) {
      const long m = m0 + u * step;
      if (m >= M) continue;
      vec_t o;
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = (half_t)((float)v[u][j] + (float)b[j]);
      *reinterpret_cast<vec_t*>(out + m * ld_out + V * c) = o;
    }
  }
}

}  // namespace

extern "C" int sdmoe_score_bias(const void* score, long ld_score, int M, int E, const void* bias, void* out,
                                long ld_out, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!score || !bias || !out || M < 0 || E <= 0) return SDMOE_EARG;
  if (ld_score < E || ld_out < E) return SDMOE_ESHAPE;
  if (E > 256) return SDMOE_EUNSUP;
  const bool vec = E % 8 == 0 && ld_score % 8 == 0 && ld_out % 8 == 0 &&
                   (((uintptr_t)score | (uintptr_t)out | (uintptr_t)bias) & 15) == 0;
  const int C = vec ? E / 8 : E;
  const int rpb = BIAS_THREADS / C;
  const long groups = ((long)M + rpb - 1) / rpb;
  const int blocks = (int)(groups < 2048 ? groups : 2048);  // memory-bound: cap the grid, stride over the rest
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    score_bias_kernel<8><<<blocks, BIAS_THREADS, 0, s>>>((const half_t*)score, ld_score, M, C, (const half_t*)bias,
                                                         (half_t*)out, ld_out);
  else
    score_bias_kernel<1><<<blocks, BIAS_THREADS, 0, s>>>((const half_t*)score, ld_score, M, C, (const half_t*)bias,
                                                         (half_t*)out, ld_out);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
