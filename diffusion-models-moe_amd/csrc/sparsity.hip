// Gate sparsity on the GEGLU seam (the reference's SparsityMeasure + sparsity/check_sparsity.py), gfx950:
//   sdmoe_geglu_sparsity  one streaming pass over Y = proj(x) = [value | gate] that serves
//     SparsityMeasure.hook_fn (neuron_receivers/sparsity_measure.py:13-18): the dense value * act(gate) product, and
//     instead of a host copy of every activated gate, the counts its consumers take from it: per neuron and group of
//     images the rows with |act(gate)| <= threshold (check_sparsity.py:41-46, `gate == 0.0` at threshold 0) and the
//     rows with act(gate) < 0 (SparsityMeasure.test, :39-41, `torch.all(gate >= 0)`).
// The loop is neuron.hip's geglu_neurons_kernel (same loads, same activation, same product: bit-identical out): 64
// chunk-columns x 4 row lanes per block, fixed row slabs that never straddle an image. Each lane counts its 8 columns
// in 8 registers (zeros in the low half, negatives in the high half: a lane sees at most 64 rows of a slab), the four
// waves are summed through LDS and the block writes one partial row of packed counts; a second small kernel sums each
// group's slabs per column and adds one integer per block and counter to the totals. Integer sums only: the result does
// not depend on the order.
#include "common.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int SPARSITY_SLAB_MIN = 64;  // smallest slab (the workspace bound is stated for it)

typedef unsigned long long u64_t;

// TAB: the registered fp16 GELU table staged in LDS (gelu_tab_h), else apply_act -- the two forms of geglu_route_kernel.
// grid (ceil(F / 512), nimg * spi); slab s = image s / spi, positions [(s % spi) * slab_rows, ...) of that image.
// totals (nullable, 2 * ngroups words) is zeroed by block (0, 0): the combine kernel that adds to it is ordered behind
// this whole grid by the stream.
template <bool TAB>
__global__ __launch_bounds__(256) void geglu_sparsity_kernel(
    const half_t* __restrict__ Y, long ldy, int F, int act, const half_t* __restrict__ gelu_tab, float threshold,
    half_t* __restrict__ out, long ldo, half_t* __restrict__ gate_out, long ldg, int rpi, int spi, int slab_rows,
    uint32_t* __restrict__ part, u64_t* __restrict__ totals, int ngroups) {
  __shared__ __attribute__((aligned(16))) half_t tab[TAB ? GELU_TAB_N : 8];
  __shared__ __attribute__((aligned(16))) uint32_t red[3][64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = blockIdx.x * 64 + lane;  // 8-column chunk
  const int slab = blockIdx.y;
  const int img = slab / spi;
  const int p0 = (slab - img * spi) * slab_rows, p1 = min(rpi, p0 + slab_rows);
  if (totals && blockIdx.x == 0 && blockIdx.y == 0)
    for (int i = threadIdx.x; i < 2 * ngroups; i += 256) totals[i] = 0;
  if constexpr (TAB) {
    for (int i = threadIdx.x; i < GELU_TAB_N / 8; i += 256)
      *reinterpret_cast<half8*>(tab + 8 * i) = *reinterpret_cast<const half8*>(gelu_tab + 8 * i);
    __syncthreads();
  }
  uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // zeros | negatives << 16
  if (chunk < F / 8) {
    const half_t* yv = Y + ((long)img * rpi) * ldy + 8 * chunk;
    half_t* orow = out + ((long)img * rpi) * ldo + 8 * chunk;
    half_t* grow = gate_out ? gate_out + ((long)img * rpi) * ldg + 8 * chunk : nullptr;
    // U rows per wave and trip: all 2 U loads are issued before the first is used (the tail's missing rows re-read
    // the trip's first row and are dropped)
    constexpr int U = 4;
    for (int pb = p0 + wave; pb < p1; pb += 4 * U) {
      half8 hv[U], gv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int pos = pb + 4 * u < p1 ? pb + 4 * u : pb;
        hv[u] = *reinterpret_cast<const half8*>(yv + (long)pos * ldy);
        gv[u] = *reinterpret_cast<const half8*>(yv + (long)pos * ldy + F);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int pos = pb + 4 * u;
        if (pos >= p1) break;  // wave-uniform
        half8 g, o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if constexpr (TAB) g[j] = gelu_tab_h(gv[u][j], tab);
          else g[j] = (half_t)apply_act((float)gv[u][j], act);
          const float gf = (float)g[j];
          cnt[j] += (__builtin_fabsf(gf) <= threshold ? 1u : 0u) + (gf < 0.f ? 0x10000u : 0u);
          o[j] = (half_t)((float)hv[u][j] * gf);
        }
        *reinterpret_cast<half8*>(orow + (long)pos * ldo) = o;
        if (grow) *reinterpret_cast<half8*>(grow + (long)pos * ldg) = g;
      }
    }
  }
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
    uint32_t* prow = part + (long)slab * F + 8 * chunk;
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
  if (f < F) {
    for (int img = 0; img < nimg; ++img) {
      if ((img_group ? img_group[img] : 0) != g) continue;
      for (int s = img * spi + wave; s < (img + 1) * spi; s += 4) {
        const uint32_t v = part[(long)s * F + f];
        zero += (int)(v & 0xffffu);
        neg += (int)(v >> 16);
      }
    }
  }
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
  if (!Y || !out || M < 0 || F <= 0) return SDMOE_EARG;
  if (!(threshold >= 0.f)) return SDMOE_EARG;  // negative or NaN
  if (!totals && !(col_zero && col_neg)) return SDMOE_EARG;
  if (F % 32 || ldy % 8 || ldo % 8 || (gate_out && ldg % 8)) return SDMOE_ESHAPE;
  if (ldy < 2L * F || ldo < F || (gate_out && ldg < F)) return SDMOE_ESHAPE;
  if (!(act == ACT_GELU || act == ACT_RELU || act == ACT_NONE || act == ACT_SILU)) return SDMOE_EUNSUP;
  const int rpi = rows_per_img > 0 ? rows_per_img : M;
  if (rows_per_img < 0 || M % rpi) return SDMOE_EARG;
  if (ngroups <= 0 || !workspace) return SDMOE_EARG;
  if (ngroups > 65535) return SDMOE_ESHAPE;
  if (((uintptr_t)Y | (uintptr_t)out | (uintptr_t)gate_out | (uintptr_t)workspace) & 15) return SDMOE_ESHAPE;
  if (((uintptr_t)col_zero | (uintptr_t)col_neg) & 3 || (uintptr_t)totals & 7) return SDMOE_ESHAPE;
  const int nimg = M / rpi;
  const int xblocks = (F / 8 + 63) / 64;
  // 256-row slabs, or 64-row ones where those would leave most of the chip without a block (one packed word per slab
  // and column; the bound is the 64-row one whichever is taken)
  int slab_rows = 256;
  if ((long)nimg * ((rpi + 255) / 256) * xblocks < 512) slab_rows = SPARSITY_SLAB_MIN;
  const int spi = (rpi + slab_rows - 1) / slab_rows;
  const long nslab = (long)nimg * spi;
  if (nslab > 65535) return SDMOE_ESHAPE;
  if ((long)nimg * ((rpi + SPARSITY_SLAB_MIN - 1) / SPARSITY_SLAB_MIN) * F > workspace_floats) return SDMOE_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* part = (uint32_t*)workspace;
  const half_t* tab = act == ACT_GELU ? sdmoe_gelu_tab_current() : nullptr;
  const dim3 grid(xblocks, (unsigned)nslab);
  if (tab)
    geglu_sparsity_kernel<true><<<grid, 256, 0, s>>>((const half_t*)Y, ldy, F, act, tab, threshold, (half_t*)out, ldo,
                                                     (half_t*)gate_out, ldg, rpi, spi, slab_rows, part, (u64_t*)totals,
                                                     ngroups);
  else
    geglu_sparsity_kernel<false><<<grid, 256, 0, s>>>((const half_t*)Y, ldy, F, act, nullptr, threshold, (half_t*)out,
                                                      ldo, (half_t*)gate_out, ldg, rpi, spi, slab_rows, part,
                                                      (u64_t*)totals, ngroups);
  SDMOE_CHECK_LAUNCH();
  sparsity_combine_kernel<<<dim3((F + 63) / 64, ngroups), 256, 0, s>>>(part, nimg, spi, F, img_group, col_zero,
                                                                       col_neg, (u64_t*)totals);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
