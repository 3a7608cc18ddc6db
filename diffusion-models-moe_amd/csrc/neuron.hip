// Neuron-level concept removal on the GEGLU seam (the reference's paired t-test path), gfx950:
//   sdmoe_geglu_neurons  one streaming pass over Y = proj(x) = [value | gate] that serves
//     NeuronPredictivity.hook_fn / NeuronPredictivityBB.hook_fn (neuron_receivers/predictivity.py:42-53,
//       neuron_predictivity_bb.py:43-63): per-neuron maximum of the activated gate over a prompt's tokens (or the
//       bounding-box positions of each image), next to the dense value * act(gate) product
//     RemoveNeurons.hook_fn (neuron_receivers/remove_skilled_neurons.py:26-42): gate[:, :, masked] = -0.17
// HBM-streaming, no MFMA: one 16-B load per lane of the value half and of the gate half, 64 chunk-columns x 4 row lanes
// per block (discovery.hip's colsq_partial_kernel), fixed row slabs that never straddle an image. Each block keeps a
// running fp16 maximum per column (from -inf: GELU columns can be negative on every row) and writes one partial row;
// a second small kernel takes each group's maximum over its images' slabs. No atomics: a maximum does not depend on
// the order, so the result is deterministic by construction.
#include "common.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int NEURON_SLAB_MIN = 64;  // smallest slab (the workspace bound is stated for it)

SDMOE_DEV half8 neg_inf8() {
  const half_t n = (half_t)(-__builtin_huge_valf());
  return half8{n, n, n, n, n, n, n, n};
}

// TAB: the registered fp16 GELU table staged in LDS (gelu_tab_h), else apply_act -- the two forms of geglu_route_kernel.
// grid (ceil(F / 512), nimg * spi); slab s = image s / spi, positions [(s % spi) * slab_rows, ...) of that image.
template <bool TAB>
__global__ __launch_bounds__(256) void geglu_neurons_kernel(
    const half_t* __restrict__ Y, long ldy, int F, int act, const half_t* __restrict__ gelu_tab,
    const uint32_t* __restrict__ override_bits, half_t override_value, half_t* __restrict__ out, long ldo,
    half_t* __restrict__ gate_out, long ldg, int rpi, int spi, int slab_rows, const uint32_t* __restrict__ pos_bits,
    half_t* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) half_t tab[TAB ? GELU_TAB_N : 8];
  __shared__ __attribute__((aligned(16))) half_t red[3][64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = blockIdx.x * 64 + lane;  // 8-column chunk
  const int slab = blockIdx.y;
  const int img = slab / spi;
  const int p0 = (slab - img * spi) * slab_rows, p1 = min(rpi, p0 + slab_rows);
  if constexpr (TAB) {
    for (int i = threadIdx.x; i < GELU_TAB_N / 8; i += 256)
      *reinterpret_cast<half8*>(tab + 8 * i) = *reinterpret_cast<const half8*>(gelu_tab + 8 * i);
    __syncthreads();
  }
  half8 mx = neg_inf8();
  if (chunk < F / 8) {
    const unsigned ob = override_bits ? (override_bits[chunk >> 2] >> (8 * (chunk & 3))) & 0xffu : 0u;
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
        }
        if (part && (!pos_bits || ((pos_bits[pos >> 5] >> (pos & 31)) & 1u))) mx = __builtin_elementwise_max(mx, g);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if ((ob >> j) & 1u) g[j] = override_value;
          o[j] = (half_t)((float)hv[u][j] * (float)g[j]);
        }
        *reinterpret_cast<half8*>(orow + (long)pos * ldo) = o;
        if (grow) *reinterpret_cast<half8*>(grow + (long)pos * ldg) = g;
      }
    }
  }
  if (!part) return;  // uniform over the grid
  if (wave > 0) *reinterpret_cast<half8*>(red[wave - 1][lane]) = mx;
  __syncthreads();
  if (wave == 0 && chunk < F / 8) {
#pragma unroll
    for (int w = 0; w < 3; ++w) mx = __builtin_elementwise_max(mx, *reinterpret_cast<const half8*>(red[w][lane]));
    *reinterpret_cast<half8*>(part + (long)slab * F + 8 * chunk) = mx;
  }
}

// colmax[g][f] = max over the slabs of the images of group g; grid (ceil(F / 64), ngroups), 64 columns x 4 slab lanes
__global__ __launch_bounds__(256) void neurons_colmax_kernel(const half_t* __restrict__ part, int nimg, int spi, int F,
                                                             const int* __restrict__ img_group,
                                                             half_t* __restrict__ colmax) {
  __shared__ half_t red[3][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + lane, g = blockIdx.y;
  half_t mx = (half_t)(-__builtin_huge_valf());
  if (f < F) {
    for (int img = 0; img < nimg; ++img) {
      if ((img_group ? img_group[img] : 0) != g) continue;
      for (int s = img * spi + wave; s < (img + 1) * spi; s += 4) {
        const half_t v = part[(long)s * F + f];
        mx = v > mx ? v : mx;
      }
    }
  }
  if (wave > 0) red[wave - 1][lane] = mx;
  __syncthreads();
  if (wave == 0 && f < F) {
#pragma unroll
    for (int w = 0; w < 3; ++w) mx = red[w][lane] > mx ? red[w][lane] : mx;
    colmax[(long)g * F + f] = mx;
  }
}

}  // namespace

extern "C" int sdmoe_geglu_neurons(const void* Y, long ldy, int M, int F, int act, const unsigned* override_bits,
                                   float override_value, void* out, long ldo, void* gate_out, long ldg,
                                   int rows_per_img, const int* img_group, int ngroups, const unsigned* pos_bits,
                                   void* colmax, float* workspace, long workspace_floats, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!Y || !out || M < 0 || F <= 0) return SDMOE_EARG;
  if (F % 32 || ldy % 8 || ldo % 8 || (gate_out && ldg % 8)) return SDMOE_ESHAPE;
  if (ldy < 2L * F || ldo < F || (gate_out && ldg < F)) return SDMOE_ESHAPE;
  if (!(act == ACT_GELU || act == ACT_RELU || act == ACT_NONE || act == ACT_SILU)) return SDMOE_EUNSUP;
  const int rpi = rows_per_img > 0 ? rows_per_img : M;
  if (rows_per_img < 0 || M % rpi) return SDMOE_EARG;
  if (colmax && (ngroups <= 0 || !workspace)) return SDMOE_EARG;
  if (((uintptr_t)Y | (uintptr_t)out | (uintptr_t)gate_out | (uintptr_t)workspace) & 15) return SDMOE_ESHAPE;
  const int nimg = M / rpi;
  const int xblocks = (F / 8 + 63) / 64;
  // 256-row slabs, or 64-row ones where those would leave most of the chip without a block (fp16 partials: two per
  // workspace float; the bound is the 64-row one whichever is taken)
  int slab_rows = 256;
  if ((long)nimg * ((rpi + 255) / 256) * xblocks < 512) slab_rows = NEURON_SLAB_MIN;
  const int spi = (rpi + slab_rows - 1) / slab_rows;
  const long nslab = (long)nimg * spi;
  if (nslab > 65535) return SDMOE_ESHAPE;
  if (colmax && (long)nimg * ((rpi + NEURON_SLAB_MIN - 1) / NEURON_SLAB_MIN) * F > 2 * workspace_floats)
    return SDMOE_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  half_t* part = colmax ? (half_t*)workspace : nullptr;
  const half_t* tab = act == ACT_GELU ? sdmoe_gelu_tab_current() : nullptr;
  const half_t ov = (half_t)override_value;
  const dim3 grid(xblocks, (unsigned)nslab);
  if (tab)
    geglu_neurons_kernel<true><<<grid, 256, 0, s>>>((const half_t*)Y, ldy, F, act, tab, override_bits, ov,
                                                    (half_t*)out, ldo, (half_t*)gate_out, ldg, rpi, spi, slab_rows,
                                                    pos_bits, part);
  else
    geglu_neurons_kernel<false><<<grid, 256, 0, s>>>((const half_t*)Y, ldy, F, act, nullptr, override_bits, ov,
                                                     (half_t*)out, ldo, (half_t*)gate_out, ldg, rpi, spi, slab_rows,
                                                     pos_bits, part);
  SDMOE_CHECK_LAUNCH();
  if (colmax) {
    neurons_colmax_kernel<<<dim3((F + 63) / 64, ngroups), 256, 0, s>>>(part, nimg, spi, F, img_group,
                                                                        (half_t*)colmax);
    SDMOE_CHECK_LAUNCH();
  }
  return SDMOE_OK;
}
