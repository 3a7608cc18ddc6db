// Expert-level discovery statistics on the outputs of the routing kernels, gfx950:
//   sdmoe_expert_stats  one streaming pass over the fp16 expert scores [M, E] and the per-token top-k bitmask sel
//     [M, ceil(E / 32)] (what sdmoe_geglu_route / sdmoe_moe_topk_mask / sdmoe_moe_topk_keep write) that serves
//     ExpertPredictivity.hook_fn (neuron_receivers/expert_activation.py:51-59): torch.max(score, dim=0), per group of
//       images
//     FrequencyMeasure.hook_fn (neuron_receivers/frequency_measure.py:53-57): how many tokens of each image selected
//       each expert (the reference's Python loop over labels[0])
// HBM-streaming, no MFMA, E <= 256 of any value: a block is 64 expert columns x 4 row lanes, so a wave reads 128
// contiguous bytes of one score row and broadcasts two sel words; the slab plan and the group walk are geglu_stream.h's
// (the row loop is this file's own: it reads scores and sel words, not the seam). Each
// block keeps a running fp16 maximum (from -inf: a GELU expert's score can be negative on every row) and an int32
// count per column and writes one partial row of each; a second small kernel combines the slabs of each group /
// image. No atomics: a maximum and an integer sum do not depend on the order, so the results are the same run to run.
#include "geglu_stream.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int STATS_SLAB_MIN = 16;  // smallest slab (the workspace bound is stated for it)

// grid (ceil(E / 64), nimg * spi); slab s = image s / spi, positions [(s % spi) * slab_rows, ...) of that image.
// pmax / pcnt: [nslab, E] partials, either may be null (uniform over the grid).
__global__ __launch_bounds__(256) void expert_stats_kernel(const half_t* __restrict__ S, long lds,
                                                           const uint32_t* __restrict__ sel, int E, int rpi, int spi,
                                                           int slab_rows, half_t* __restrict__ pmax,
                                                           int* __restrict__ pcnt) {
  __shared__ half_t redm[3][64];
  __shared__ int redc[3][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const int slab = blockIdx.y;
  const Slab sl = slab_decode(slab, rpi, spi, slab_rows);
  const int p0 = sl.p0, p1 = sl.p1;
  const int words = (E + 31) >> 5;
  half_t mx = (half_t)(-__builtin_huge_valf());
  int cnt = 0;
  if (e < E) {
    const long row0 = (long)sl.img * rpi;
    if (pmax) {
      const half_t* col = S + row0 * lds + e;
      for (int p = p0 + wave; p < p1; p += 4) {
        const half_t v = col[(long)p * lds];
        mx = v > mx ? v : mx;
      }
    }
    if (pcnt) {
      const uint32_t* w = sel + row0 * words + (e >> 5);
      for (int p = p0 + wave; p < p1; p += 4) cnt += (int)((w[(long)p * words] >> (e & 31)) & 1u);
    }
  }
  if (wave > 0) {
    redm[wave - 1][lane] = mx;
    redc[wave - 1][lane] = cnt;
  }
  __syncthreads();
  if (wave == 0 && e < E) {
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      mx = redm[w][lane] > mx ? redm[w][lane] : mx;
      cnt += redc[w][lane];
    }
    if (pmax) pmax[(long)slab * E + e] = mx;
    if (pcnt) pcnt[(long)slab * E + e] = cnt;
  }
}

// grid (ceil(E / 64), nmax + ncnt), 64 columns x 4 slab lanes: rows y < nmax give colmax[y] = the maximum over the
// slabs of the images of group y, rows y >= nmax give count[y - nmax] = the sum over the slabs of that image.
__global__ __launch_bounds__(256) void expert_stats_combine_kernel(const half_t* __restrict__ pmax,
                                                                   const int* __restrict__ pcnt, int nimg, int spi,
                                                                   int E, const int* __restrict__ img_group, int nmax,
                                                                   half_t* __restrict__ colmax,
                                                                   int* __restrict__ count) {
  __shared__ half_t redm[3][64];
  __shared__ int redc[3][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const int y = blockIdx.y;  // block-uniform
  half_t mx = (half_t)(-__builtin_huge_valf());
  int cnt = 0;
  if (e < E) {
    if (y < nmax)
      for_group_slabs(img_group, nimg, spi, y, wave, [&](int s) {
        const half_t v = pmax[(long)s * E + e];
        mx = v > mx ? v : mx;
      });
    else
      for_image_slabs(y - nmax, spi, wave, [&](int s) { cnt += pcnt[(long)s * E + e]; });
  }
  if (wave > 0) {
    redm[wave - 1][lane] = mx;
    redc[wave - 1][lane] = cnt;
  }
  __syncthreads();
  if (wave == 0 && e < E) {
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      mx = redm[w][lane] > mx ? redm[w][lane] : mx;
      cnt += redc[w][lane];
    }
    if (y < nmax) colmax[(long)y * E + e] = mx;
    else count[(long)(y - nmax) * E + e] = cnt;
  }
}

}  // namespace

extern "C" int sdmoe_expert_stats(const void* score, long ld_score, const unsigned* sel, int M, int E,
                                  int rows_per_img, const int* img_group, int ngroups, void* colmax, int* count,
                                  float* workspace, long workspace_floats, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (M < 0 || E <= 0) return SDMOE_EARG;
  if (E > 256) return SDMOE_ESHAPE;
  if (count && !sel) return SDMOE_EARG;
  if (colmax && (!score || ngroups <= 0)) return SDMOE_EARG;
  if (colmax && ld_score < E) return SDMOE_ESHAPE;
  const int rpi = rows_per_img > 0 ? rows_per_img : M;
  if (rows_per_img < 0 || M % rpi) return SDMOE_EARG;
  if (!colmax && !count) return SDMOE_OK;
  if (!workspace) return SDMOE_EARG;
  const int xblocks = (E + 63) / 64;
  // the largest slab that still gives every CU a block; counts first (int32), then the fp16 maxima, two per workspace
  // float
  const SlabPlan p = slab_plan(M, rows_per_img, xblocks, STATS_SLAB_MIN, 256);
  const long cells = slab_cells(p, STATS_SLAB_MIN, E);
  const long cnt_floats = count ? cells : 0;
  if (cnt_floats + (colmax ? (cells + 1) / 2 : 0) > workspace_floats) return SDMOE_ESHAPE;
  const long ny = (colmax ? (long)ngroups : 0) + (count ? (long)p.nimg : 0);
  if (p.nslab > 65535 || ny > 65535) return SDMOE_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  int* pcnt = count ? (int*)workspace : nullptr;
  half_t* pmax = colmax ? (half_t*)(workspace + cnt_floats) : nullptr;
  expert_stats_kernel<<<dim3(xblocks, (unsigned)p.nslab), 256, 0, s>>>((const half_t*)score, ld_score, sel, E, p.rpi,
                                                                       p.spi, p.slab_rows, pmax, pcnt);
  SDMOE_CHECK_LAUNCH();
  expert_stats_combine_kernel<<<dim3(xblocks, (unsigned)ny), 256, 0, s>>>(pmax, pcnt, p.nimg, p.spi, E, img_group,
                                                                          colmax ? ngroups : 0, (half_t*)colmax, count);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
