// The noise-HPO objective on the device (the reference's modularity/remove_experts_noise_hpo.py:74-84), gfx950:
//   sdmoe_noise_capture   channels 0..3 of every row of the U-Net's padded output buffer -> one compact [rows, 4] step
//     slice of a [T, nimg * HW, 4] store (what the reference copies to the host at every step);
//   sdmoe_noise_distance  for every step t and group of images g of two such stores a, b:
//     out[t][g] = { S (a - b)^2, A = S |a|, B = S |b|, S (a / max(A, 1e-12) - b / max(B, 1e-12))^2 }
//     -- the squares of torch.norm(a - b) and of the distance of the F.normalize(p = 1)'d vectors.
// Everything after the fp16 loads is float64: the objective's minimum is a ~ b, where the fourth sum is the difference
// of two nearly equal quotients per element (an expanded S a^2 / A^2 - 2 S a b / (A B) + S b^2 / B^2 cancels there).
// Three launches, no atomics: (1) each block reduces one slab of <= 1024 rows of one image and step to the partial
// triple {S (a - b)^2, S |a|, S |b|}; (2) each block first sums its group's A and B from those partials, in image then
// slab order, and reduces the same slab to the partial of the fourth sum with IEEE divisions; (3) one thread per
// (t, g) adds the partials in the same fixed order. The slab split depends on HW alone, every in-block sum is a fixed
// tree: results are bit-identical from run to run. Only channels 0..3 of a row are ever loaded (one 8-byte load).
#include "common.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int NOISE_SLAB = 1024;  // rows per block: 256 threads x 4 rows
constexpr double NORMALIZE_EPS = 1e-12;  // F.normalize's clamp of the norm

SDMOE_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum of N per-thread doubles over the 256 threads of the block: wave trees, then waves 0..3 in order. Valid in
// thread 0. red: [N][4] doubles of LDS.
template <int N>
SDMOE_DEV void block_sum_f64(double (&v)[N], double (*red)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    v[i] = wave_sum_f64(v[i]);
    if (lane == 0) red[i][wave] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ((red[i][0] + red[i][1]) + red[i][2]) + red[i][3];
  }
}

// block -> (t, img, slab); rows [p0, p1) of image img
struct SlabPos {
  long t;
  int img, slab, p0, p1;
};
SDMOE_DEV SlabPos slab_pos(int nimg, int HW, int spi) {
  SlabPos s;
  const long b = blockIdx.x;
  s.slab = (int)(b % spi);
  s.img = (int)((b / spi) % nimg);
  s.t = b / ((long)spi * nimg);
  s.p0 = s.slab * NOISE_SLAB;
  s.p1 = min(HW, s.p0 + NOISE_SLAB);
  return s;
}

// part1[block][3] = {S (a - b)^2, S |a|, S |b|} of the block's slab. grid T * nimg * spi.
__global__ __launch_bounds__(256) void noise_partial_kernel(const half_t* __restrict__ a, long lda, long step_a,
                                                            const half_t* __restrict__ b, long ldb, long step_b,
                                                            int nimg, int HW, int spi, double* __restrict__ part1) {
  __shared__ double red[3][4];
  const SlabPos s = slab_pos(nimg, HW, spi);
  const half_t* ap = a + s.t * step_a + (long)s.img * HW * lda;
  const half_t* bp = b + s.t * step_b + (long)s.img * HW * ldb;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int p = s.p0 + threadIdx.x; p < s.p1; p += 256) {
    const half4 av = *reinterpret_cast<const half4*>(ap + (long)p * lda);
    const half4 bv = *reinterpret_cast<const half4*>(bp + (long)p * ldb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double x = (double)av[j], y = (double)bv[j], d = x - y;
      acc[0] += d * d;
      acc[1] += __builtin_fabs(x);
      acc[2] += __builtin_fabs(y);
    }
  }
  block_sum_f64<3>(acc, red);
  if (threadIdx.x == 0) {
    double* o = part1 + 3 * (long)blockIdx.x;
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
  }
}

// A and B of step t, group g: the partials of the group's images, image then slab order (the order of finalize).
SDMOE_DEV void group_l1(const double* __restrict__ part1, long t, int g, int nimg, int spi,
                        const int* __restrict__ img_group, double& A, double& B) {
  A = 0.0;
  B = 0.0;
  for (int i = 0; i < nimg; ++i) {
    if ((img_group ? img_group[i] : 0) != g) continue;
    const double* p = part1 + 3 * ((t * nimg + i) * spi);
    for (int s = 0; s < spi; ++s) {
      A += p[3 * s + 1];
      B += p[3 * s + 2];
    }
  }
}

// part2[block] = S (a / max(A, eps) - b / max(B, eps))^2 of the block's slab, A and B of the image's group.
__global__ __launch_bounds__(256) void noise_normalized_kernel(const half_t* __restrict__ a, long lda, long step_a,
                                                               const half_t* __restrict__ b, long ldb, long step_b,
                                                               int nimg, int HW, int spi,
                                                               const int* __restrict__ img_group,
                                                               const double* __restrict__ part1,
                                                               double* __restrict__ part2) {
  __shared__ double red[1][4];
  __shared__ double norms[2];
  const SlabPos s = slab_pos(nimg, HW, spi);
  if (threadIdx.x == 0) {
    double A, B;
    group_l1(part1, s.t, img_group ? img_group[s.img] : 0, nimg, spi, img_group, A, B);
    norms[0] = A > NORMALIZE_EPS ? A : NORMALIZE_EPS;
    norms[1] = B > NORMALIZE_EPS ? B : NORMALIZE_EPS;
  }
  __syncthreads();
  const double A = norms[0], B = norms[1];
  const half_t* ap = a + s.t * step_a + (long)s.img * HW * lda;
  const half_t* bp = b + s.t * step_b + (long)s.img * HW * ldb;
  double acc[1] = {0.0};
  for (int p = s.p0 + threadIdx.x; p < s.p1; p += 256) {
    const half4 av = *reinterpret_cast<const half4*>(ap + (long)p * lda);
    const half4 bv = *reinterpret_cast<const half4*>(bp + (long)p * ldb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)av[j] / A - (double)bv[j] / B;
      acc[0] += d * d;
    }
  }
  block_sum_f64<1>(acc, red);
  if (threadIdx.x == 0) part2[blockIdx.x] = acc[0];
}

// out[t][g][0..3]: one thread per (t, g). A group without images gives zeros.
__global__ __launch_bounds__(64) void noise_finalize_kernel(const double* __restrict__ part1,
                                                            const double* __restrict__ part2, int T, int nimg, int spi,
                                                            const int* __restrict__ img_group, int ngroups,
                                                            double* __restrict__ out) {
  const long idx = (long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (long)T * ngroups) return;
  const long t = idx / ngroups;
  const int g = (int)(idx - t * ngroups);
  double A, B, sq = 0.0, nsq = 0.0;
  group_l1(part1, t, g, nimg, spi, img_group, A, B);
  for (int i = 0; i < nimg; ++i) {
    if ((img_group ? img_group[i] : 0) != g) continue;
    const long base = (t * nimg + i) * spi;
    for (int s = 0; s < spi; ++s) {
      sq += part1[3 * (base + s)];
      nsq += part2[base + s];
    }
  }
  double* o = out + 4 * idx;
  o[0] = sq;
  o[1] = A;
  o[2] = B;
  o[3] = nsq;
}

__global__ __launch_bounds__(256) void noise_capture_kernel(const half_t* __restrict__ eps, long lde,
                                                            half_t* __restrict__ store, long lds, long rows) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  *reinterpret_cast<half4*>(store + r * lds) = *reinterpret_cast<const half4*>(eps + r * lde);
}

}  // namespace

extern "C" int sdmoe_noise_capture(const void* eps, long lde, void* store, long lds, long rows, void* stream) {
  if (rows == 0) return SDMOE_OK;
  if (!eps || !store || rows < 0) return SDMOE_EARG;
  if (lde < 4 || lds < 4 || lde % 4 || lds % 4) return SDMOE_ESHAPE;
  if (((uintptr_t)eps | (uintptr_t)store) & 7) return SDMOE_ESHAPE;
  const long blocks = (rows + 255) / 256;
  if (blocks > 0x7fffffffL) return SDMOE_ESHAPE;
  noise_capture_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const half_t*)eps, lde, (half_t*)store, lds,
                                                                          rows);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_noise_distance(const void* a, long lda, long step_a, const void* b, long ldb, long step_b, int T,
                                    int nimg, int HW, const int* img_group, int ngroups, double* out,
                                    double* workspace, long workspace_doubles, void* stream) {
  if (!a || !b || !out || !workspace) return SDMOE_EARG;
  if (T <= 0 || nimg <= 0 || HW < 1 || ngroups <= 0) return SDMOE_EARG;
  if (!img_group && ngroups != 1) return SDMOE_EARG;  // no table: one group
  if (step_a < 0 || step_b < 0) return SDMOE_EARG;
  if (lda < 4 || ldb < 4 || lda % 4 || ldb % 4 || step_a % 4 || step_b % 4) return SDMOE_ESHAPE;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out | (uintptr_t)workspace) & 7) return SDMOE_ESHAPE;
  if ((uintptr_t)img_group & 3) return SDMOE_ESHAPE;
  const int spi = (HW + NOISE_SLAB - 1) / NOISE_SLAB;
  const long blocks = (long)T * nimg * spi;
  if (blocks > 0x7fffffffL || (long)T * ngroups > 0x7fffffffL * 64) return SDMOE_ESHAPE;
  if (4 * blocks > workspace_doubles) return SDMOE_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  double* part1 = workspace;
  double* part2 = workspace + 3 * blocks;
  noise_partial_kernel<<<(unsigned)blocks, 256, 0, s>>>((const half_t*)a, lda, step_a, (const half_t*)b, ldb, step_b,
                                                        nimg, HW, spi, part1);
  SDMOE_CHECK_LAUNCH();
  noise_normalized_kernel<<<(unsigned)blocks, 256, 0, s>>>((const half_t*)a, lda, step_a, (const half_t*)b, ldb,
                                                           step_b, nimg, HW, spi, img_group, part1, part2);
  SDMOE_CHECK_LAUNCH();
  const long cells = (long)T * ngroups;
  noise_finalize_kernel<<<(unsigned)((cells + 63) / 64), 64, 0, s>>>(part1, part2, T, nimg, spi, img_group, ngroups,
                                                                    out);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
