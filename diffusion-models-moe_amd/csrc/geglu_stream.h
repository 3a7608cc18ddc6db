// What the streaming statistics kernels on the GEGLU hook seam share (neuron.hip, sparsity.hip; expert_stats.hip takes
// the plan, the slab decode and the group walk): the row-slab plan and the entry checks on the host, the one loop over
// Y = proj(x) = [value | gate] and the walk over a group's slabs on the device.
// A block is 64 columns (or 8-column chunks) x 4 row lanes (waves) and owns one slab: rows [p0, p1) of one image, so a
// slab never straddles an image. It writes one partial row per slab; a second small kernel combines the slabs of each
// group of images.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------ slab plan (host)
struct SlabPlan {
  int rpi, nimg;       // rows per image (rows_per_img, or M: one image), images
  int slab_rows, spi;  // rows per slab, slabs per image
  long nslab;          // nimg * spi: the grid's y extent (the caller refuses > 65535)
};

// The largest of 256, 64, 16 ... rows, down to slab_min, that still gives want_blocks blocks of xblocks column blocks
// per slab. rows_per_img >= 0 and M % rpi == 0 are the caller's checks.
inline SlabPlan slab_plan(int M, int rows_per_img, int xblocks, int slab_min, int want_blocks) {
  SlabPlan p;
  p.rpi = rows_per_img > 0 ? rows_per_img : M;
  p.nimg = M / p.rpi;
  p.slab_rows = 256;
  while (p.slab_rows > slab_min &&
         (long)p.nimg * ((p.rpi + p.slab_rows - 1) / p.slab_rows) * xblocks < want_blocks)
    p.slab_rows /= 4;
  p.spi = (p.rpi + p.slab_rows - 1) / p.slab_rows;
  p.nslab = (long)p.nimg * p.spi;
  return p;
}

// Partial cells of cols columns at the smallest slab: what the workspace bounds are stated for, whichever slab is taken
inline long slab_cells(const SlabPlan& p, int slab_min, int cols) {
  return (long)p.nimg * ((p.rpi + slab_min - 1) / slab_min) * cols;
}

// ------------------------------------------------------------------------------------------------ entry checks (host)
// The argument checks of the entry points that stream the seam, after their `M == 0` return. own: the status of the
// entry point's own checks on the group / workspace arguments, which rank between rows_per_img and the alignment.
inline int geglu_seam_check(const void* Y, long ldy, int M, int F, int act, const void* out, long ldo,
                            const void* gate_out, long ldg, int rows_per_img, const void* workspace, int own) {
  if (!Y || !out || M < 0 || F <= 0) return SDMOE_EARG;
  if (F % 32 || ldy % 8 || ldo % 8 || (gate_out && ldg % 8)) return SDMOE_ESHAPE;
  if (ldy < 2L * F || ldo < F || (gate_out && ldg < F)) return SDMOE_ESHAPE;
  if (!(act == ACT_GELU || act == ACT_RELU || act == ACT_NONE || act == ACT_SILU)) return SDMOE_EUNSUP;
  if (rows_per_img < 0 || M % (rows_per_img > 0 ? rows_per_img : M)) return SDMOE_EARG;
  if (own != SDMOE_OK) return own;
  if (((uintptr_t)Y | (uintptr_t)out | (uintptr_t)gate_out | (uintptr_t)workspace) & 15) return SDMOE_ESHAPE;
  return SDMOE_OK;
}

// ------------------------------------------------------------------------------------------------ device
// The seam operands of one launch. tab: the registered fp16 GELU table (kernel<TAB = true>), or null.
struct GegluSeam {
  const half_t* Y;
  long ldy;
  int F, act;
  const half_t* tab;
  half_t* out;
  long ldo;
  half_t* gate_out;  // nullable
  long ldg;
  int rpi, spi, slab_rows;
};

inline GegluSeam geglu_seam(const void* Y, long ldy, int F, int act, void* out, long ldo, void* gate_out, long ldg,
                            const SlabPlan& p) {
  return GegluSeam{(const half_t*)Y, ldy, F, act, act == ACT_GELU ? sdmoe_gelu_tab_current() : nullptr, (half_t*)out,
                   ldo, (half_t*)gate_out, ldg, p.rpi, p.spi, p.slab_rows};
}

// slab s of a grid of nimg * spi slabs = image s / spi, positions [p0, p1) of that image
struct Slab {
  int img, p0, p1;
};
SDMOE_DEV Slab slab_decode(int slab, int rpi, int spi, int slab_rows) {
  const int img = slab / spi;
  const int p0 = (slab - img * spi) * slab_rows;
  return Slab{img, p0, min(rpi, p0 + slab_rows)};
}

// The loop of a 256-thread block over slab blockIdx.y, columns 8 * chunk .. + 7 (chunk = blockIdx.x * 64 + lane): out =
// value * g' and gate_out = g', g = act(gate) through the table staged in LDS (TAB; gelu_tab_h) or apply_act -- the two
// forms of geglu_route_kernel. Each row's activated gate goes to stat.row(pos, g), then stat.gate(g) may replace it
// (g') before the product. Ends without a barrier: the caller's cross-wave reduce brings its own.
template <bool TAB, class Stat>
SDMOE_DEV void geglu_stream_slab(const GegluSeam& sm, Stat& stat) {
  __shared__ __attribute__((aligned(16))) half_t tab[TAB ? GELU_TAB_N : 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = blockIdx.x * 64 + lane;
  const Slab sl = slab_decode(blockIdx.y, sm.rpi, sm.spi, sm.slab_rows);
  const int F = sm.F, p1 = sl.p1;
  if constexpr (TAB) {
    for (int i = threadIdx.x; i < GELU_TAB_N / 8; i += 256)
      *reinterpret_cast<half8*>(tab + 8 * i) = *reinterpret_cast<const half8*>(sm.tab + 8 * i);
    __syncthreads();
  }
  if (chunk >= F / 8) return;
  const long ldy = sm.ldy, ldo = sm.ldo, ldg = sm.ldg;
  const half_t* yv = sm.Y + ((long)sl.img * sm.rpi) * ldy + 8 * chunk;
  half_t* orow = sm.out + ((long)sl.img * sm.rpi) * ldo + 8 * chunk;
  half_t* grow = sm.gate_out ? sm.gate_out + ((long)sl.img * sm.rpi) * ldg + 8 * chunk : nullptr;
  // U rows per wave and trip: all 2 U loads are issued before the first is used (the tail's missing rows re-read
  // the trip's first row and are dropped)
  constexpr int U = 4;
  for (int pb = sl.p0 + wave; pb < p1; pb += 4 * U) {
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
        else g[j] = (half_t)apply_act((float)gv[u][j], sm.act);
      }
      stat.row(pos, g);
      stat.gate(g);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)hv[u][j] * (float)g[j]);
      *reinterpret_cast<half8*>(orow + (long)pos * ldo) = o;
      if (grow) *reinterpret_cast<half8*>(grow + (long)pos * ldg) = g;
    }
  }
}

// The combine kernels' walk, 4 slab lanes (waves): fn(s) for this wave's slabs of image img / of the images of group g
// (img_group null: every image is group 0)
template <class Fn>
SDMOE_DEV void for_image_slabs(int img, int spi, int wave, Fn fn) {
  for (int s = img * spi + wave; s < (img + 1) * spi; s += 4) fn(s);
}
template <class Fn>
SDMOE_DEV void for_group_slabs(const int* img_group, int nimg, int spi, int g, int wave, Fn fn) {
  for (int img = 0; img < nimg; ++img)
    if ((img_group ? img_group[img] : 0) == g) for_image_slabs(img, spi, wave, fn);
}
