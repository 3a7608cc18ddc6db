// Neuron-level concept removal on the GEGLU seam (the reference's paired t-test path), gfx950:
//   sdmoe_geglu_neurons  one streaming pass over Y = proj(x) = [value | gate] that serves
//     NeuronPredictivity.hook_fn / NeuronPredictivityBB.hook_fn (neuron_receivers/predictivity.py:42-53,
//       neuron_predictivity_bb.py:43-63): per-neuron maximum of the activated gate over a prompt's tokens (or the
//       bounding-box positions of each image), next to the dense value * act(gate) product
//     RemoveNeurons.hook_fn (neuron_receivers/remove_skilled_neurons.py:26-42): gate[:, :, masked] = -0.17
// HBM-streaming, no MFMA: the seam loop, the slab plan and the group walk are geglu_stream.h's. Each block keeps a
// running fp16 maximum per column (from -inf: GELU columns can be negative on every row) and writes one partial row;
// a second small kernel takes each group's maximum over its images' slabs. No atomics: a maximum does not depend on
// the order, so the result is deterministic by construction.
#include "geglu_stream.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int NEURON_SLAB_MIN = 64;  // smallest slab (the workspace bound is stated for it)

// What a lane keeps of its 8 columns: the running maximum of the activated gate over the rows that count (all when
// pos_bits is null; none when no maximum is wanted), taken before the override of the columns of `ob` (one bit each).
struct NeuronStat {
  half8 mx;
  const uint32_t* pos_bits;
  bool want;
  unsigned ob;
  half_t override_value;
  SDMOE_DEV void row(int pos, half8 g) {
    if (want && (!pos_bits || ((pos_bits[pos >> 5] >> (pos & 31)) & 1u))) mx = __builtin_elementwise_max(mx, g);
  }
  SDMOE_DEV void gate(half8& g) const {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if ((ob >> j) & 1u) g[j] = override_value;
  }
};

// grid (ceil(F / 512), nimg * spi); part (nullable, uniform over the grid): [nslab, F] partial maxima
template <bool TAB>
__global__ __launch_bounds__(256) void geglu_neurons_kernel(const GegluSeam sm,
                                                            const uint32_t* __restrict__ override_bits,
                                                            half_t override_value,
                                                            const uint32_t* __restrict__ pos_bits,
                                                            half_t* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) half_t red[3][64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = blockIdx.x * 64 + lane;  // 8-column chunk
  const int F = sm.F;
  const half_t n = (half_t)(-__builtin_huge_valf());
  NeuronStat st{half8{n, n, n, n, n, n, n, n}, pos_bits, part != nullptr, 0u, override_value};
  if (override_bits && chunk < F / 8) st.ob = (override_bits[chunk >> 2] >> (8 * (chunk & 3))) & 0xffu;
  geglu_stream_slab<TAB>(sm, st);
  if (!part) return;
  half8 mx = st.mx;
  if (wave > 0) *reinterpret_cast<half8*>(red[wave - 1][lane]) = mx;
  __syncthreads();
  if (wave == 0 && chunk < F / 8) {
#pragma unroll
    for (int w = 0; w < 3; ++w) mx = __builtin_elementwise_max(mx, *reinterpret_cast<const half8*>(red[w][lane]));
    *reinterpret_cast<half8*>(part + (long)blockIdx.y * F + 8 * chunk) = mx;
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
  if (f < F)
    for_group_slabs(img_group, nimg, spi, g, wave, [&](int s) {
      const half_t v = part[(long)s * F + f];
      mx = v > mx ? v : mx;
    });
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
  if (int st = geglu_seam_check(Y, ldy, M, F, act, out, ldo, gate_out, ldg, rows_per_img, workspace,
                                colmax && (ngroups <= 0 || !workspace) ? SDMOE_EARG : SDMOE_OK))
    return st;
  const int xblocks = (F / 8 + 63) / 64;
  // 64-row slabs where 256-row ones would leave most of the chip without a block (fp16 partials: two per workspace
  // float)
  const SlabPlan p = slab_plan(M, rows_per_img, xblocks, NEURON_SLAB_MIN, 512);
  if (p.nslab > 65535) return SDMOE_ESHAPE;
  if (colmax && slab_cells(p, NEURON_SLAB_MIN, F) > 2 * workspace_floats) return SDMOE_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  half_t* part = colmax ? (half_t*)workspace : nullptr;
  const GegluSeam sm = geglu_seam(Y, ldy, F, act, out, ldo, gate_out, ldg, p);
  const half_t ov = (half_t)override_value;
  const dim3 grid(xblocks, (unsigned)p.nslab);
  if (sm.tab) geglu_neurons_kernel<true><<<grid, 256, 0, s>>>(sm, override_bits, ov, pos_bits, part);
  else geglu_neurons_kernel<false><<<grid, 256, 0, s>>>(sm, override_bits, ov, pos_bits, part);
  SDMOE_CHECK_LAUNCH();
  if (colmax) {
    neurons_colmax_kernel<<<dim3((F + 63) / 64, ngroups), 256, 0, s>>>(part, p.nimg, p.spi, F, img_group,
                                                                        (half_t*)colmax);
    SDMOE_CHECK_LAUNCH();
  }
  return SDMOE_OK;
}
