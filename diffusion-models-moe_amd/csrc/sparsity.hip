// Gate sparsity on the GEGLU seam (the reference's SparsityMeasure + sparsity/check_sparsity.py), gfx950:
//   sdmoe_geglu_sparsity  one streaming pass over Y = proj(x) = [value | gate] that serves
//     SparsityMeasure.hook_fn (neuron_receivers/sparsity_measure.py:13-18): the dense value * act(gate) product, and
//     instead of a host copy of every activated gate, the counts its consumers take from it: per neuron and group of
//     images the rows with |act(gate)| <= threshold (check_sparsity.py:41-46, `gate == 0.0` at threshold 0) and the
//     rows with act(gate) < 0 (SparsityMeasure.test, :39-41, `torch.all(gate >= 0)`).
// HBM-streaming, no MFMA: the seam loop, the slab plan and the group walk are geglu_stream.h's. Each lane counts its 8
// columns in 8 registers (zeros in the low half, negatives in the high half), the four waves are summed through LDS
// and the block writes one partial row of packed counts; a second small kernel sums each group's slabs per column and
// adds one integer per block and counter to the totals. Integer sums only: the result does not depend on the order.
#include "geglu_stream.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int SPARSITY_SLAB_MIN = 64;  // smallest slab (the workspace bound is stated for it)

typedef unsigned long long u64_t;

// What a lane keeps of its 8 columns: zeros | negatives << 16 per column (a lane sees at most 64 rows of a slab)
struct SparsityStat {
  uint32_t cnt[8];
  float threshold;
  SDMOE_DEV void row(int, half8 g) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gf = (float)g[j];
      cnt[j] += (__builtin_fabsf(gf) <= threshold ? 1u : 0u) + (gf < 0.f ? 0x10000u : 0u);
    }
  }
  SDMOE_DEV void gate(half8&) const {}
};

// grid (ceil(F / 512), nimg * spi); part: [nslab, F] packed partial counts. totals (nullable, 2 * ngroups words) is
// zeroed by block (0, 0): the combine kernel that adds to it is ordered behind this whole grid by the stream.
template <bool TAB>
__global__ __launch_bounds__(256) void geglu_sparsity_kernel(const GegluSeam sm, float threshold,
                                                             uint32_t* __restrict__ part, u64_t* __restrict__ totals,
                                                             int ngroups) {
  __shared__ __attribute__((aligned(16))) uint32_t red[3][64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = blockIdx.x * 64 + lane;  // 8-column chunk
  const int F = sm.F;
  if (totals && blockIdx.x == 0 && blockIdx.y == 0)
    for (int i = threadIdx.x; i < 2 * ngroups; i += 256) totals[i] = 0;
  SparsityStat st{{0, 0, 0, 0, 0, 0, 0, 0}, threshold};
  geglu_stream_slab<TAB>(sm, st);
  uint32_t* cnt = st.cnt;
  if (wave > 0) {
    *reinterpret_cast<uint4v*>(&red[wave - 1][lane][0]) = uint4v{cnt[0], cnt[1], cnt[2], cnt[3]};
    *reinterpret_cast<uint4v*>(&red[wave - 1][lane][4]) = uint4v{cnt[4], cnt[5], cnt[6], cnt[7]};
  }
  __syncthreads();
  if (wave == 0 && chunk < F / 8) {
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      const uint4v a = *reinterpret_cast<const uint4v*>(&red[w][lane][0]);
      const uint4v b = *reinterpret_cast<const uint4v*>(&red[w][lane][4]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cnt[j] += a[j];
        cnt[4 + j] += b[j];
      }
    }
    uint32_t* prow = part + (long)blockIdx.y * F + 8 * chunk;
    *reinterpret_cast<uint4v*>(prow) = uint4v{cnt[0], cnt[1], cnt[2], cnt[3]};
    *reinterpret_cast<uint4v*>(prow + 4) = uint4v{cnt[4], cnt[5], cnt[6], cnt[7]};
  }
}

// col_zero[g][f] / col_neg[g][f] = sums over the slabs of the images of group g; totals[g] += the block's 64 columns
// (one integer atomic per block and counter). grid (ceil(F / 64), ngroups), 64 columns x 4 slab lanes.
__global__ __launch_bounds__(256) void sparsity_combine_kernel(const uint32_t* __restrict__ part, int nimg, int spi,
                                                               int F, const int* __restrict__ img_group,
                                                               int* __restrict__ col_zero, int* __restrict__ col_neg,
                                                               u64_t* __restrict__ totals) {
  __shared__ int red[3][64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + lane, g = blockIdx.y;
  int zero = 0, neg = 0;
  if (f < F)
    for_group_slabs(img_group, nimg, spi, g, wave, [&](int s) {
      const uint32_t v = part[(long)s * F + f];
      zero += (int)(v & 0xffffu);
      neg += (int)(v >> 16);
    });
  if (wave > 0) {
    red[wave - 1][lane][0] = zero;
    red[wave - 1][lane][1] = neg;
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    zero += red[w][lane][0];
    neg += red[w][lane][1];
  }
  if (f < F) {
    if (col_zero) col_zero[(long)g * F + f] = zero;
    if (col_neg) col_neg[(long)g * F + f] = neg;
  }
  if (!totals) return;
  u64_t tz = (u64_t)zero, tn = (u64_t)neg;  // lanes at or past F hold 0
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    tz += __shfl_xor(tz, o, 64);
    tn += __shfl_xor(tn, o, 64);
  }
  if (lane == 0) {
    atomicAdd(totals + 2 * g, tz);
    atomicAdd(totals + 2 * g + 1, tn);
  }
}

}  // namespace

extern "C" int sdmoe_geglu_sparsity(const void* Y, long ldy, int M, int F, int act, float threshold, void* out,
                                    long ldo, void* gate_out, long ldg, int rows_per_img, const int* img_group,
                                    int ngroups, int* col_zero, int* col_neg, int64_t* totals, float* workspace,
                                    long workspace_floats, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!(threshold >= 0.f)) return SDMOE_EARG;  // negative or NaN
  if (!totals && !(col_zero && col_neg)) return SDMOE_EARG;
  const int own = ngroups <= 0 || !workspace ? SDMOE_EARG : ngroups > 65535 ? SDMOE_ESHAPE : SDMOE_OK;
  if (int st = geglu_seam_check(Y, ldy, M, F, act, out, ldo, gate_out, ldg, rows_per_img, workspace, own)) return st;
  if (((uintptr_t)col_zero | (uintptr_t)col_neg) & 3 || (uintptr_t)totals & 7) return SDMOE_ESHAPE;
  const int xblocks = (F / 8 + 63) / 64;
  // 64-row slabs where 256-row ones would leave most of the chip without a block (one packed word per slab and column)
  const SlabPlan p = slab_plan(M, rows_per_img, xblocks, SPARSITY_SLAB_MIN, 512);
  if (p.nslab > 65535) return SDMOE_ESHAPE;
  if (slab_cells(p, SPARSITY_SLAB_MIN, F) > workspace_floats) return SDMOE_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* part = (uint32_t*)workspace;
  const GegluSeam sm = geglu_seam(Y, ldy, F, act, out, ldo, gate_out, ldg, p);
  const dim3 grid(xblocks, (unsigned)p.nslab);
  if (sm.tab) geglu_sparsity_kernel<true><<<grid, 256, 0, s>>>(sm, threshold, part, (u64_t*)totals, ngroups);
  else geglu_sparsity_kernel<false><<<grid, 256, 0, s>>>(sm, threshold, part, (u64_t*)totals, ngroups);
  SDMOE_CHECK_LAUNCH();
  sparsity_combine_kernel<<<dim3((F + 63) / 64, ngroups), 256, 0, s>>>(part, p.nimg, p.spi, F, img_group, col_zero,
                                                                       col_neg, (u64_t*)totals);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
