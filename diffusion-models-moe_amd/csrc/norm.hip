// Normalisation kernels for the SD U-Net step (gfx950).
//
// GroupNorm is split into a statistics pass (this file: one coalesced read of the activation -> per-(image,
// channel) fp32 scale/shift) and a vectorised apply(+SiLU) pass (gemm.hip, sdmoe_groupnorm_apply) that feeds
// the LDS-DMA conv/GEMM. (Applying it inside the conv's operand load would redo it for all 9 taps x N-tiles.)
//   diffusers ResnetBlock2D norm1/norm2 (GroupNorm(32, C, eps=1e-5)), Transformer2DModel.norm
//   (GroupNorm(32, C, eps=1e-6)), conv_norm_out.
// LayerNorm (BasicTransformerBlock norm1/2/3, eps=1e-5) is one wave per token row, two-pass in registers.
#include "common.h"
#include "tune.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int GN_SMALL_HW = 1024;  // latents up to 32x32 take the single-launch path (measured crossover)
// KNOB_GN_FUSED picks sdmoe_groupnorm's path at HW <= GN_FUSED_HW: gn_fused_reg_kernel (1), gn_fused_kernel (2) or the
// two launches (0);
// single-launch statistics + apply up to 16x16 latents: 13.0 vs 15.9 us at 8x8 (C = 1280, 16 images), 14.5 vs 16.0
// at 16x16; at 32x32 it is slower (21.9 vs 21.1 us, C = 640; 47.6 vs 42.2 at C = 1920): every block re-reads its
// chunk's 1024 rows with 16 KB in flight, which no longer hides behind the saved launch (tools/micro_ab.py gn)
constexpr int GN_FUSED_HW = 256;

// chunk width of the small-latent kernels: whole groups and whole 16-B chunks (lcm(cpg, 8)), doubled towards 80
// channels while the chunk count stays integral; 0 when no such chunk exists
int gn_chunk_width(int C, int groups) {
  const int cpg = C / groups;
  int wc = cpg;
  while (wc % 8) wc += cpg;
  while (wc < 80 && C % (2 * wc) == 0 && 2 * wc <= 256) wc *= 2;
  return (wc <= 256 && wc / cpg <= 32 && C % wc == 0) ? wc : 0;
}

// Reference of the shifted sums of one (image, group); g0 = the group's first channel in the image's row 0. The sums
// are well conditioned while |ref - mean| is a few std: the variance b / n - m1^2 cancels ((ref - mean) / std)^2 of its
// leading digits. ref is the mean of 8 channels spread over the group in row 0 (the first among them), rounded to fp16
// so that x - ref stays exact. A single element as the reference put the whole cancellation on that element: an
// outlier there (|ref - mean| / std = sqrt(n), n the group's element count) cost n * 4e-8 of the variance, 4e-3 at
// 1088 rows x 80 channels; with 8 samples the same outlier costs 64 times less. Every statistics kernel and the
// finalize call this, so their sums stay bit-identical.
SDMOE_DEV float gn_ref(const half_t* g0, int cpg) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += (float)g0[(j * cpg) >> 3];
  return (float)(half_t)(s * 0.125f);
}

// Partial sums of (x - ref) and (x - ref)^2 over a slice of rows of one image, for every group at once.
// ref = gn_ref of the group (shifted sums keep the variance well conditioned).
// Reads whole rows with 16-B loads: "virtual thread" vt (NV per thread) owns 8-channel chunk vt % nch and row
// phase vt / nch, accumulates per-channel sums in registers; LDS reduces phases, then channels per group.
SDMOE_DEV void gn_accum8(const half8& v, const float (&rf)[8], float (&s1)[8], float (&s2)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float a = (float)v[i] - rf[i];
    s1[i] += a;
    s2[i] = __builtin_fmaf(a, a, s2[i]);
  }
}

template <int NV>
__global__ __launch_bounds__(256) void gn_partial_kernel(const half_t* __restrict__ X, long ldx, int HW, int C,
                                                         int G, int S, float2* __restrict__ part) {
  __shared__ float red[256 * NV][17];
  __shared__ float csum[2][2560];
  __shared__ float refs[64];
  const int s = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const int cpg = C / G, nch = C / 8;
  const int RP = max(1, (256 * NV) / nch);
  const int r0 = (int)((long)HW * s / S), r1 = (int)((long)HW * (s + 1) / S);
  const half_t* base = X + (long)img * HW * ldx;
  if (tid < G) refs[tid] = gn_ref(base + tid * cpg, cpg);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int vt = tid + 256 * j;
    if (vt < nch * RP) {
      const int c = vt % nch, ph = vt / nch;
      float rf[8], s1[8], s2[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { rf[i] = refs[(c * 8 + i) / cpg]; s1[i] = 0.f; s2[i] = 0.f; }
      // 4 rows' loads in flight per step: the 8x8 / 16x16 latents give a thread only ~8 rows, and one
      // load-use chain per row left those launches latency-bound (~10 us for 2.6 MB)
      const half_t* xp = base + (long)(r0 + ph) * ldx + c * 8;
      const long step = (long)RP * ldx;
      int r = r0 + ph;
      for (; r + 3 * RP < r1; r += 4 * RP, xp += 4 * step) {
        const half8 v0 = *reinterpret_cast<const half8*>(xp);
        const half8 v1 = *reinterpret_cast<const half8*>(xp + step);
        const half8 v2 = *reinterpret_cast<const half8*>(xp + 2 * step);
        const half8 v3 = *reinterpret_cast<const half8*>(xp + 3 * step);
        gn_accum8(v0, rf, s1, s2);
        gn_accum8(v1, rf, s1, s2);
        gn_accum8(v2, rf, s1, s2);
        gn_accum8(v3, rf, s1, s2);
      }
      for (; r < r1; r += RP, xp += step) gn_accum8(*reinterpret_cast<const half8*>(xp), rf, s1, s2);
#pragma unroll
      for (int i = 0; i < 8; ++i) { red[vt][i] = s1[i]; red[vt][8 + i] = s2[i]; }
    }
  }
  __syncthreads();
  for (int c = tid; c < nch; c += 256) {
    float a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
    for (int ph = 0; ph < RP; ++ph)
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] += red[ph * nch + c][i];
#pragma unroll
    for (int i = 0; i < 8; ++i) { csum[0][c * 8 + i] = a[i]; csum[1][c * 8 + i] = a[8 + i]; }
  }
  __syncthreads();
  if (tid < G) {
    float a = 0.f, b = 0.f;
    for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { a += csum[0][c]; b += csum[1][c]; }
    part[((long)img * G + tid) * S + s] = make_float2(a, b);
  }
}

// Small latents (HW <= 1024: the 32x32 / 16x16 / 8x8 levels): one block per (image, chunk of WC channels holding
// whole groups) reads its chunk of every row and writes the final scale/shift itself — one launch instead of
// partial + finalize, whose two launch latencies dominated these 0.1-1.3 MB GroupNorms (~12 us each).
// Same shifted sums as gn_partial_kernel; thread t owns 8-channel chunk t % nq and row phase t / nq.
__global__ __launch_bounds__(256) void gn_small_kernel(const half_t* __restrict__ X, long ldx, int HW, int C, int G,
                                                       int WC, const half_t* __restrict__ gamma,
                                                       const half_t* __restrict__ beta, float eps,
                                                       float* __restrict__ scale, float* __restrict__ shift) {
  __shared__ float red[256][17];
  __shared__ float csum[2][256];
  __shared__ float refs[32];
  __shared__ float stat[32][2];
  const int chunk = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const int cpg = C / G, c0 = chunk * WC, nq = WC / 8, R = 256 / nq, gc = WC / cpg;
  const half_t* base = X + (long)img * HW * ldx + c0;
  if (tid < gc) refs[tid] = gn_ref(base + tid * cpg, cpg);
  __syncthreads();
  const int q = tid % nq, ph = tid / nq;
  float rf[8], s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { rf[i] = refs[min((q * 8 + i) / cpg, gc - 1)]; s1[i] = 0.f; s2[i] = 0.f; }
  if (ph < R) {
    const half_t* xp = base + (long)ph * ldx + q * 8;
    const long step = (long)R * ldx;
    int r = ph;
    for (; r + 3 * R < HW; r += 4 * R, xp += 4 * step) {
      const half8 v0 = *reinterpret_cast<const half8*>(xp);
      const half8 v1 = *reinterpret_cast<const half8*>(xp + step);
      const half8 v2 = *reinterpret_cast<const half8*>(xp + 2 * step);
      const half8 v3 = *reinterpret_cast<const half8*>(xp + 3 * step);
      gn_accum8(v0, rf, s1, s2);
      gn_accum8(v1, rf, s1, s2);
      gn_accum8(v2, rf, s1, s2);
      gn_accum8(v3, rf, s1, s2);
    }
    for (; r < HW; r += R, xp += step) gn_accum8(*reinterpret_cast<const half8*>(xp), rf, s1, s2);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) { red[tid][i] = s1[i]; red[tid][8 + i] = s2[i]; }
  __syncthreads();
  for (int c = tid; c < nq; c += 256) {
    float a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
    for (int p = 0; p < R; ++p)
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] += red[p * nq + c][i];
#pragma unroll
    for (int i = 0; i < 8; ++i) { csum[0][c * 8 + i] = a[i]; csum[1][c * 8 + i] = a[8 + i]; }
  }
  __syncthreads();
  if (tid < gc) {
    double a = 0.0, b = 0.0;
    for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { a += csum[0][c]; b += csum[1][c]; }
    const double n = (double)HW * cpg;
    const double m1 = a / n;
    double var = b / n - m1 * m1;
    if (var < 0) var = 0;
    stat[tid][0] = (float)((double)refs[tid] + m1);
    stat[tid][1] = (float)(1.0 / sqrt(var + (double)eps));
  }
  __syncthreads();
  for (int c = tid; c < WC; c += 256) {
    const int g = c / cpg, ch = c0 + c;
    const float sc = stat[g][1] * (float)gamma[ch];
    scale[(long)img * C + ch] = sc;
    shift[(long)img * C + ch] = (float)beta[ch] - stat[g][0] * sc;
  }
}

// GroupNorm statistics AND apply(+SiLU) in ONE launch for small latents (HW <= GN_FUSED_HW). Block (chunk, slice, image):
// the statistics of its (image, WC-channel chunk) exactly as gn_small_kernel computes them (same shifted sums, same
// reduction order, same fp64 finalize -> bit-identical scale/shift), every block over ALL HW rows of its chunk (the
// S slices of a chunk re-read it from L2: S x the chunk's bytes, a few MB), then the apply on its own slice of rows.
// Replaces gn_small_kernel + gn_apply_kernel -- two dependent launches of ~10 us each on these 0.1-1.3 MB
// tensors, i.e. launch and load latency, not bytes -- with one; S slices per chunk keep >= ~512 blocks in flight.
__global__ __launch_bounds__(256) void gn_fused_kernel(const half_t* __restrict__ X, long ldx, int HW, int C, int G,
                                                       int WC, int S, const half_t* __restrict__ gamma,
                                                       const half_t* __restrict__ beta, float eps, int silu,
                                                       half_t* __restrict__ Y, long ldy, float* __restrict__ scale,
                                                       float* __restrict__ shift) {
  __shared__ float red[256][17];
  __shared__ float csum[2][256];
  __shared__ float refs[32];
  __shared__ float stat[32][2];
  __shared__ float cscale[256], cshift[256];
  const int nchunk = C / WC;
  const int chunk = blockIdx.x % nchunk, slice = blockIdx.x / nchunk, img = blockIdx.y, tid = threadIdx.x;
  const int cpg = C / G, c0 = chunk * WC, nq = WC / 8, R = 256 / nq, gc = WC / cpg;
  const half_t* base = X + (long)img * HW * ldx + c0;
  if (tid < gc) refs[tid] = gn_ref(base + tid * cpg, cpg);
  __syncthreads();
  const int q = tid % nq, ph = tid / nq;
  float rf[8], s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { rf[i] = refs[min((q * 8 + i) / cpg, gc - 1)]; s1[i] = 0.f; s2[i] = 0.f; }
  if (ph < R) {
    const half_t* xp = base + (long)ph * ldx + q * 8;
    const long step = (long)R * ldx;
    int r = ph;
    for (; r + 3 * R < HW; r += 4 * R, xp += 4 * step) {
      const half8 v0 = *reinterpret_cast<const half8*>(xp);
      const half8 v1 = *reinterpret_cast<const half8*>(xp + step);
      const half8 v2 = *reinterpret_cast<const half8*>(xp + 2 * step);
      const half8 v3 = *reinterpret_cast<const half8*>(xp + 3 * step);
      gn_accum8(v0, rf, s1, s2);
      gn_accum8(v1, rf, s1, s2);
      gn_accum8(v2, rf, s1, s2);
      gn_accum8(v3, rf, s1, s2);
    }
    for (; r < HW; r += R, xp += step) gn_accum8(*reinterpret_cast<const half8*>(xp), rf, s1, s2);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) { red[tid][i] = s1[i]; red[tid][8 + i] = s2[i]; }
  __syncthreads();
  for (int c = tid; c < nq; c += 256) {
    float a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
    for (int p = 0; p < R; ++p)
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] += red[p * nq + c][i];
#pragma unroll
    for (int i = 0; i < 8; ++i) { csum[0][c * 8 + i] = a[i]; csum[1][c * 8 + i] = a[8 + i]; }
  }
  __syncthreads();
  if (tid < gc) {
    double a = 0.0, b = 0.0;
    for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { a += csum[0][c]; b += csum[1][c]; }
    const double n = (double)HW * cpg;
    const double m1 = a / n;
    double var = b / n - m1 * m1;
    if (var < 0) var = 0;
    stat[tid][0] = (float)((double)refs[tid] + m1);
    stat[tid][1] = (float)(1.0 / sqrt(var + (double)eps));
  }
  __syncthreads();
  for (int c = tid; c < WC; c += 256) {
    const int g = c / cpg, ch = c0 + c;
    const float sc = stat[g][1] * (float)gamma[ch];
    const float sh = (float)beta[ch] - stat[g][0] * sc;
    cscale[c] = sc;
    cshift[c] = sh;
    if (slice == 0 && scale) {
      scale[(long)img * C + ch] = sc;
      shift[(long)img * C + ch] = sh;
    }
  }
  __syncthreads();
  // apply on rows [r0, r1) of this slice: the gn_apply_kernel arithmetic on the same fp32 scale / shift
  const int r0 = (int)((long)HW * slice / S), r1 = (int)((long)HW * (slice + 1) / S);
  float sc8[8], sh8[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { sc8[j] = cscale[q * 8 + j]; sh8[j] = cshift[q * 8 + j]; }
  if (ph >= R) return;
  const long rowbase = (long)img * HW;
  for (int r = r0 + ph; r < r1; r += R) {
    const half8 x = *reinterpret_cast<const half8*>(X + (rowbase + r) * ldx + c0 + q * 8);
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = (float)x[j] * sc8[j] + sh8[j];
      if (silu) f = silu_f(f);
      o[j] = (half_t)f;
    }
    *reinterpret_cast<half8*>(Y + (rowbase + r) * ldy + c0 + q * 8) = o;
  }
}

// gn_fused_kernel with its latency chain cut (sdmoe_tune knob 7 = 1, default; 2 = the kernel above): every row of
// the thread's chunk (RMAX at most) is loaded into registers up front -- before the barrier that publishes the
// group references -- together with its gamma / beta, so the kernel waits on global memory once; the row-phase
// reduction runs on nq x 16 threads instead of nq; the apply reads the rows from those registers (no second global
// read) and each block stores the rows of its slice [r0, r1). Same sums in the same order as gn_small_kernel +
// gn_apply_kernel: bit-identical output, scale and shift.
template <int RMAX>
__global__ __launch_bounds__(256) void gn_fused_reg_kernel(const half_t* __restrict__ X, long ldx, int HW, int C,
                                                           int G, int WC, int S, const half_t* __restrict__ gamma,
                                                           const half_t* __restrict__ beta, float eps, int silu,
                                                           half_t* __restrict__ Y, long ldy, float* __restrict__ scale,
                                                           float* __restrict__ shift) {
  __shared__ float red[256][17];
  __shared__ float csum[2][256];
  __shared__ float refs[32];
  __shared__ float stat[32][2];
  const int nchunk = C / WC;
  const int chunk = blockIdx.x % nchunk, slice = blockIdx.x / nchunk, img = blockIdx.y, tid = threadIdx.x;
  const int cpg = C / G, c0 = chunk * WC, nq = WC / 8, R = 256 / nq, gc = WC / cpg;
  const half_t* base = X + (long)img * HW * ldx + c0;
  const int q = tid % nq, ph = tid / nq;
  const bool live = ph < R;
  half8 v[RMAX];
#pragma unroll
  for (int k = 0; k < RMAX; ++k) {
    const int r = ph + k * R;
    v[k] = (live && r < HW) ? *reinterpret_cast<const half8*>(base + (long)r * ldx + q * 8)
                            : (half8){0, 0, 0, 0, 0, 0, 0, 0};
  }
  const half8 gm8 = *reinterpret_cast<const half8*>(gamma + c0 + q * 8);
  const half8 bt8 = *reinterpret_cast<const half8*>(beta + c0 + q * 8);
  if (tid < gc) refs[tid] = gn_ref(base + tid * cpg, cpg);
  __syncthreads();
  float rf[8], s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { rf[i] = refs[min((q * 8 + i) / cpg, gc - 1)]; s1[i] = 0.f; s2[i] = 0.f; }
#pragma unroll
  for (int k = 0; k < RMAX; ++k)
    if (live && ph + k * R < HW) gn_accum8(v[k], rf, s1, s2);
#pragma unroll
  for (int i = 0; i < 8; ++i) { red[tid][i] = s1[i]; red[tid][8 + i] = s2[i]; }
  __syncthreads();
  // (chunk c, value i): the R row phases in order, as gn_small_kernel's per-c loop; nq * 16 can exceed the 256
  // threads (WC up to 256 -> nq up to 32, e.g. C = 576 / 1152 / 1600 with 32 groups), hence the stride
  for (int id = tid; id < nq * 16; id += 256) {
    const int c = id >> 4, i = id & 15;
    float a = 0.f;
    for (int p = 0; p < R; ++p) a += red[p * nq + c][i];
    csum[i >> 3][c * 8 + (i & 7)] = a;
  }
  __syncthreads();
  if (tid < gc) {
    double a = 0.0, b = 0.0;
    for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { a += csum[0][c]; b += csum[1][c]; }
    const double n = (double)HW * cpg;
    const double m1 = a / n;
    double var = b / n - m1 * m1;
    if (var < 0) var = 0;
    stat[tid][0] = (float)((double)refs[tid] + m1);
    stat[tid][1] = (float)(1.0 / sqrt(var + (double)eps));
  }
  __syncthreads();
  if (slice == 0 && scale) {
    for (int c = tid; c < WC; c += 256) {
      const int g = c / cpg, ch = c0 + c;
      const float sc = stat[g][1] * (float)gamma[ch];
      scale[(long)img * C + ch] = sc;
      shift[(long)img * C + ch] = (float)beta[ch] - stat[g][0] * sc;
    }
  }
  if (!live) return;
  float sc8[8], sh8[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int g = min((q * 8 + j) / cpg, gc - 1);
    sc8[j] = stat[g][1] * (float)gm8[j];
    sh8[j] = (float)bt8[j] - stat[g][0] * sc8[j];
  }
  const int r0 = (int)((long)HW * slice / S), r1 = (int)((long)HW * (slice + 1) / S);
  const long rowbase = (long)img * HW;
#pragma unroll
  for (int k = 0; k < RMAX; ++k) {
    const int r = ph + k * R;
    if (r < r0 || r >= r1) continue;
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = (float)v[k][j] * sc8[j] + sh8[j];
      if (silu) f = silu_f(f);
      o[j] = (half_t)f;
    }
    *reinterpret_cast<half8*>(Y + (rowbase + r) * ldy + c0 + q * 8) = o;
  }
}

// One wave per (image, group): combine slices in fp64, emit scale = rstd*gamma, shift = beta - mean*scale.
__global__ __launch_bounds__(64) void gn_finalize_kernel(const half_t* __restrict__ X, long ldx, int HW, int C,
                                                         int G, int S, const float2* __restrict__ part,
                                                         const half_t* __restrict__ gamma,
                                                         const half_t* __restrict__ beta, float eps,
                                                         float* __restrict__ scale, float* __restrict__ shift) {
  const int g = blockIdx.x, img = blockIdx.y, lane = threadIdx.x;
  const int cpg = C / G;
  double a = 0.0, b = 0.0;
  for (int s = lane; s < S; s += 64) {
    float2 v = part[((long)img * G + g) * S + s];
    a += v.x; b += v.y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
  const double n = (double)HW * cpg;
  const double ref = (double)gn_ref(X + (long)img * HW * ldx + g * cpg, cpg);
  const double m1 = a / n;
  double var = b / n - m1 * m1;
  if (var < 0) var = 0;
  const float mean = (float)(ref + m1);
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  for (int c = lane; c < cpg; c += 64) {
    const int ch = g * cpg + c;
    const float sc = rstd * (float)gamma[ch];
    scale[(long)img * C + ch] = sc;
    shift[(long)img * C + ch] = (float)beta[ch] - mean * sc;
  }
}


// LayerNorm over the last dim (C % 64 == 0, C <= 2048): 8 lanes per row, 8 rows per wave, blockDim/8 rows per
// block (4 waves; 1 wave when M is small, so the 16x16 / 8x8 latents' few thousand rows still cover every CU);
// lane (row r = lane/8, sub = lane%8) holds 16-B chunks sub, sub+8, ... (128-B coalesced per 8 lanes), two-pass
// mean / variance in registers with 8-lane xor reductions.
template <int CPL>  // chunks per lane = C / 64
__global__ __launch_bounds__(256) void layernorm_kernel(const half_t* __restrict__ X, long ldx, half_t* __restrict__ Y,
                                                        long ldy, int M, int C, const half_t* __restrict__ gamma,
                                                        const half_t* __restrict__ beta, float eps) {
  const int lane = threadIdx.x & 63, sub = lane & 7;
  const int row = blockIdx.x * (int)(blockDim.x >> 3) + (int)(threadIdx.x >> 3);
  const bool live = row < M;
  const half_t* xr = X + (long)(live ? row : 0) * ldx;
  half8 v[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) v[i] = *reinterpret_cast<const half8*>(xr + (sub + 8 * i) * 8);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) s += (float)v[i][j];
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float d = (float)v[i][j] - mean; q = __builtin_fmaf(d, d, q); }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) q += __shfl_xor(q, o, 64);
  const float rstd = rsqrtf(q / C + eps);
  if (!live) return;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = (sub + 8 * i) * 8;
    const half8 gm = *reinterpret_cast<const half8*>(gamma + c);
    const half8 bt = *reinterpret_cast<const half8*>(beta + c);
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)(((float)v[i][j] - mean) * rstd * (float)gm[j] + (float)bt[j]);
    *reinterpret_cast<half8*>(Y + (long)row * ldy + c) = o;
  }
}

}  // namespace

namespace {
// statistics: gn_small_kernel for HW <= 1024, else partial sums + finalize
int groupnorm_impl(const void* X, long ldx, int nimg, int HW, int C, int groups, const void* gamma, const void* beta,
                   float eps, float* scale, float* shift, float* workspace, long workspace_floats, void* stream) {
  if (!X || !gamma || !beta || !scale || !shift || !workspace || nimg <= 0 || HW <= 0 || groups <= 0)
    return SDMOE_EARG;
  if (C % groups || C % 8 || ldx % 8 || C > 2560 || groups > 64) return SDMOE_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (HW <= GN_SMALL_HW) {
    const int wc = gn_chunk_width(C, groups);
    if (wc) {
      gn_small_kernel<<<dim3(C / wc, nimg), 256, 0, st>>>((const half_t*)X, ldx, HW, C, groups, wc,
                                                          (const half_t*)gamma, (const half_t*)beta, eps, scale,
                                                          shift);
      SDMOE_CHECK_LAUNCH();
      return SDMOE_OK;
    }
  }
  // ~1024 workgroups in total, every slice at least 8 rows
  int S = (1024 + nimg - 1) / nimg;
  if (S > HW / 8) S = HW / 8;
  if (S > 64) S = 64;
  if (S < 1) S = 1;
  if ((long)nimg * groups * S * 2 > workspace_floats) return SDMOE_EARG;
  hipStream_t s = (hipStream_t)stream;
  float2* part = reinterpret_cast<float2*>(workspace);
  if (C / 8 > 256)
    gn_partial_kernel<2><<<dim3(S, nimg), 256, 0, s>>>((const half_t*)X, ldx, HW, C, groups, S, part);
  else
    gn_partial_kernel<1><<<dim3(S, nimg), 256, 0, s>>>((const half_t*)X, ldx, HW, C, groups, S, part);
  SDMOE_CHECK_LAUNCH();
  gn_finalize_kernel<<<dim3(groups, nimg), 64, 0, s>>>((const half_t*)X, ldx, HW, C, groups, S, part,
                                                       (const half_t*)gamma, (const half_t*)beta, eps, scale, shift);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
}  // namespace

extern "C" int sdmoe_groupnorm_stats(const void* X, long ldx, int nimg, int HW, int C, int groups,
                                     const void* gamma, const void* beta, float eps, float* scale, float* shift,
                                     float* workspace, long workspace_floats, void* stream) {
  return groupnorm_impl(X, ldx, nimg, HW, C, groups, gamma, beta, eps, scale, shift, workspace, workspace_floats,
                        stream);
}

extern "C" int sdmoe_groupnorm(const void* X, long ldx, int nimg, int HW, int C, int groups, const void* gamma,
                               const void* beta, float eps, int silu, void* Y, long ldy, float* scale, float* shift,
                               float* workspace, long workspace_floats, void* stream) {
  if (!Y || ldy % 8) return Y ? SDMOE_ESHAPE : SDMOE_EARG;
  // small latents: statistics + apply in one launch, the rows of each chunk split over S slices so the grid keeps
  // >= ~512 blocks (one block per chunk -- 128-256 blocks -- streamed the output 0.4-1 % slower end to end)
  if (knob(KNOB_GN_FUSED) && HW <= GN_FUSED_HW && X && gamma && beta && nimg > 0 && groups > 0 && C % groups == 0 &&
      C % 8 == 0 && ldx % 8 == 0 && groups <= 64) {
    const int wc = gn_chunk_width(C, groups);
    if (wc) {
      const int nchunk = C / wc;
      int S = (512 + nchunk * nimg - 1) / (nchunk * nimg);
      const int R = 256 / (wc / 8);
      if (S > HW / R) S = HW / R;  // every slice at least one row per row phase
      if (S < 1) S = 1;
      const dim3 grid(nchunk * S, nimg);
      hipStream_t st = (hipStream_t)stream;
      const half_t *x = (const half_t*)X, *g = (const half_t*)gamma, *b = (const half_t*)beta;
      const int rpt = (HW + R - 1) / R;  // rows per thread of the register-resident kernel
      if (knob(KNOB_GN_FUSED) == 1 && rpt <= 16) {
        if (rpt <= 4) gn_fused_reg_kernel<4><<<grid, 256, 0, st>>>(x, ldx, HW, C, groups, wc, S, g, b, eps, silu, (half_t*)Y, ldy, scale, shift);
        else if (rpt <= 8) gn_fused_reg_kernel<8><<<grid, 256, 0, st>>>(x, ldx, HW, C, groups, wc, S, g, b, eps, silu, (half_t*)Y, ldy, scale, shift);
        else gn_fused_reg_kernel<16><<<grid, 256, 0, st>>>(x, ldx, HW, C, groups, wc, S, g, b, eps, silu, (half_t*)Y, ldy, scale, shift);
      } else {
        gn_fused_kernel<<<grid, 256, 0, st>>>(x, ldx, HW, C, groups, wc, S, g, b, eps, silu, (half_t*)Y, ldy, scale,
                                              shift);
      }
      SDMOE_CHECK_LAUNCH();
      return SDMOE_OK;
    }
  }
  // statistics then the wide-grid apply pass
  int st = groupnorm_impl(X, ldx, nimg, HW, C, groups, gamma, beta, eps, scale, shift, workspace, workspace_floats,
                          stream);
  if (st != SDMOE_OK) return st;
  return sdmoe_groupnorm_apply(X, ldx, nimg, HW, C, scale, shift, silu, Y, ldy, stream);
}

extern "C" int sdmoe_layernorm(const void* X, long ldx, void* Y, long ldy, int M, int C, const void* gamma,
                               const void* beta, float eps, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!X || !Y || !gamma || !beta || M < 0 || C <= 0) return SDMOE_EARG;
  if (C % 64 || ldx % 8 || ldy % 8 || C > 2048) return SDMOE_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  // 32-row blocks while that still gives >= ~4 blocks per CU, else one-wave 8-row blocks
  const int nt = M >= 32 * 1024 ? 256 : 64;
  const int blocks = (M + nt / 8 - 1) / (nt / 8);
  const half_t* x = (const half_t*)X;
  half_t* y = (half_t*)Y;
  const half_t* g = (const half_t*)gamma;
  const half_t* b = (const half_t*)beta;
  switch (C / 64) {
#define SDMOE_LN(n) \
    case n: layernorm_kernel<n><<<blocks, nt, 0, s>>>(x, ldx, y, ldy, M, C, g, b, eps); break;
    SDMOE_LN(1) SDMOE_LN(2) SDMOE_LN(3) SDMOE_LN(4) SDMOE_LN(5) SDMOE_LN(6) SDMOE_LN(8) SDMOE_LN(10)
    SDMOE_LN(12) SDMOE_LN(16) SDMOE_LN(20) SDMOE_LN(24) SDMOE_LN(32)
#undef SDMOE_LN
    default: return SDMOE_EUNSUP;
  }
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
