// The CLIP scorer's image front end and score reduction on the device (the reference's benchmarks/artist_removal.py:
// 173-215 and art_removal.py:80-127 do this on the host: PNG round trip, CLIPProcessor's Pillow resize, fp32 cosines
// one image at a time), gfx950:
//   sdmoe_clip_quantise    [B, 3, H, W] fp16 / fp32 in [0, 1] -> [B, H, W, 3] uint8, rint(float(x) * 255) half-even,
//     clamped: diffusers' numpy_to_pil.
//   sdmoe_clip_resample_h  Pillow's 8-bit bicubic horizontal pass (libImaging/Resample.c) for the crop window's
//     columns and the rows the vertical pass reads: clip8((2^21 + S pixel * k) >> 22) in int32, uint8 out.
//   sdmoe_clip_resample_v  the vertical pass for the crop window's rows, and in its store the rescale, CLIP
//     normalisation and patchify: fp16((u8 * (1/255) - mean[c]) / std[c]) straight into the patch-embedding GEMM's A
//     operand (row b G^2 + py G + px, column c p^2 + iy p + ix, padding columns zero); the uint8 crop is optional.
//   sdmoe_clip_scores      per row the float64 cosines cos(T,A), cos(T,R), cos(A,R) of fp16 feature rows, then
//     S cos(A,R), S cos(A,R)^2 and the count of cos(T,A) > cos(T,R) in one fixed-order block: no atomics, results
//     bit-identical from run to run (noise.hip is the precedent).
// The coefficient tables come from the host (float64, Pillow's precompute_coeffs / normalize_coeffs_8bpc): the
// kernels are integer-exact, so the whole front end is bit-identical to Pillow + the processor's uint8 pixels.
// One thread per output pixel (three channels); every access is guarded by the pixel's own bounds.
#include "common.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int PRECISION_BITS = 22;  // Pillow's 8bpc fixed point (32 - 8 - 2)

SDMOE_DEV unsigned quant8(float x) {
  const float v = __builtin_rintf(x * 255.0f);  // v_rndne: round half to even, as numpy's round
  return (unsigned)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));  // NaN -> 0
}

SDMOE_DEV unsigned clip8(int acc) {
  const int v = acc >> PRECISION_BITS;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Four pixels of one row per thread: three coalesced plane reads, 12 bytes out (three dword stores when W % 4 == 0
// and the output is dword aligned, else byte stores).
template <typename T>
__global__ __launch_bounds__(256) void quantise_kernel(const T* __restrict__ x, uint8_t* __restrict__ out, int B,
                                                       int H, int W, int W4, int dwords) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)B * H * W4;
  if (idx >= total) return;
  const int x4 = (int)(idx % W4);
  const long by = idx / W4;  // b * H + y
  const long b = by / H;
  const int y = (int)(by - b * H);
  const int x0 = x4 * 4;
  const long plane = (long)H * W;
  const T* src = x + (b * 3) * plane + (long)y * W + x0;
  uint8_t* dst = out + (by * W + x0) * 3;
  const int nx = min(4, W - x0);
  unsigned q[12];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) q[i * 3 + c] = i < nx ? quant8((float)src[c * plane + i]) : 0u;
  if (dwords && nx == 4) {
    unsigned* d32 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      d32[j] = q[4 * j] | (q[4 * j + 1] << 8) | (q[4 * j + 2] << 16) | (q[4 * j + 3] << 24);
  } else {
    for (int i = 0; i < nx * 3; ++i) dst[i] = (uint8_t)q[i];
  }
}

// tmp[b, r, xo, c] = clip8(2^21 + S_t in[b, row0 + r, bounds[xo].lo + t, c] * kk[xo][t]), r < nrows, xo < S.
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ in, long in_bstride, int W,
                                                         int row0, int nrows, const int* __restrict__ bounds,
                                                         const int* __restrict__ kk, int ksize, int S, int B,
                                                         uint8_t* __restrict__ tmp) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * nrows * S) return;
  const int xo = (int)(idx % S);
  const long br = idx / S;  // b * nrows + r
  const long b = br / nrows;
  const int r = (int)(br - b * nrows);
  const int lo = bounds[2 * xo], n = bounds[2 * xo + 1];
  const int* k = kk + (long)xo * ksize;
  const uint8_t* src = in + b * in_bstride + ((long)(row0 + r) * W + lo) * 3;
  int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < n; ++t) {
    const int w = k[t];
    a0 += (int)src[3 * t] * w;
    a1 += (int)src[3 * t + 1] * w;
    a2 += (int)src[3 * t + 2] * w;
  }
  uint8_t* dst = tmp + idx * 3;
  dst[0] = (uint8_t)clip8(a0);
  dst[1] = (uint8_t)clip8(a1);
  dst[2] = (uint8_t)clip8(a2);
}

// fp16(((u8 * (1/255)) - mean) / std), every step rounded to fp32 as the processor's NumPy does: no contraction of the
// multiply and the subtraction into one fma, IEEE division.
SDMOE_DEV half_t clip_normalise(unsigned q, float mean, float std) {
#pragma clang fp contract(off)
  const float v = (float)q * (1.0f / 255.0f);
  const float d = v - mean;
  return (half_t)(d / std);
}

struct NormC {
  float mean[3], std[3];
};

// u8[b, yo, xo, c] = clip8(2^21 + S_t tmp[b, bounds[yo].lo - row0 + t, xo, c] * kk[yo][t]); A as in the header.
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ tmp, int row0, int nrows,
                                                         const int* __restrict__ bounds, const int* __restrict__ kk,
                                                         int ksize, int S, int B, int patch, NormC nc,
                                                         uint8_t* __restrict__ u8out, half_t* __restrict__ A,
                                                         long lda, int kpad) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * S * S) return;
  const int xo = (int)(idx % S);
  const long byo = idx / S;
  const long b = byo / S;
  const int yo = (int)(byo - b * S);
  const int lo = bounds[2 * yo] - row0, n = bounds[2 * yo + 1];
  const int* k = kk + (long)yo * ksize;
  const uint8_t* src = tmp + ((b * nrows + lo) * S + xo) * 3;
  const long rstride = (long)S * 3;
  int acc[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
  for (int t = 0; t < n; ++t) {
    const int w = k[t];
    const uint8_t* p = src + t * rstride;
    acc[0] += (int)p[0] * w;
    acc[1] += (int)p[1] * w;
    acc[2] += (int)p[2] * w;
  }
  unsigned q[3] = {clip8(acc[0]), clip8(acc[1]), clip8(acc[2])};
  if (u8out) {
    uint8_t* d = u8out + idx * 3;
    d[0] = (uint8_t)q[0];
    d[1] = (uint8_t)q[1];
    d[2] = (uint8_t)q[2];
  }
  if (A) {
    const int G = S / patch, pp = patch * patch;
    const int py = yo / patch, iy = yo - py * patch, px = xo / patch, ix = xo - px * patch;
    half_t* row = A + ((b * G + py) * G + px) * lda;
#pragma unroll
    for (int c = 0; c < 3; ++c) row[c * pp + iy * patch + ix] = clip_normalise(q[c], nc.mean[c], nc.std[c]);
    if (iy == 0 && ix == 0)
      for (int j = 3 * pp; j < kpad; ++j) row[j] = (half_t)0.0f;
  }
}

SDMOE_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr double COS_EPS = 1e-8;  // torch.nn.functional.cosine_similarity's clamp of each norm

SDMOE_DEV double cosine(double xy, double xx, double yy) {
  const double nx = __builtin_sqrt(xx), ny = __builtin_sqrt(yy);
  return xy / ((nx > COS_EPS ? nx : COS_EPS) * (ny > COS_EPS ? ny : COS_EPS));
}

// One wave per row: out[i] = cos(T,A), out[n + i] = cos(T,R), out[2n + i] = cos(A,R) (the first two 0 without T).
__global__ __launch_bounds__(64) void clip_cos_kernel(const half_t* __restrict__ T, long ldt,
                                                      const half_t* __restrict__ A, long lda,
                                                      const half_t* __restrict__ R, long ldr, int n, int D,
                                                      double* __restrict__ out) {
  const long i = blockIdx.x;
  const half_t* a = A + i * lda;
  const half_t* r = R + i * ldr;
  const half_t* t = T ? T + i * ldt : nullptr;
  double ta = 0.0, tr = 0.0, ar = 0.0, tt = 0.0, aa = 0.0, rr = 0.0;
  for (int j = threadIdx.x; j < D; j += 64) {
    const double x = (double)a[j], y = (double)r[j], z = t ? (double)t[j] : 0.0;
    ta += z * x;
    tr += z * y;
    ar += x * y;
    tt += z * z;
    aa += x * x;
    rr += y * y;
  }
  ta = wave_sum_f64(ta);
  tr = wave_sum_f64(tr);
  ar = wave_sum_f64(ar);
  tt = wave_sum_f64(tt);
  aa = wave_sum_f64(aa);
  rr = wave_sum_f64(rr);
  if (threadIdx.x == 0) {
    out[i] = t ? cosine(ta, tt, aa) : 0.0;
    out[n + i] = t ? cosine(tr, tt, rr) : 0.0;
    out[2L * n + i] = cosine(ar, aa, rr);
  }
}

// out[3n .. 3n + 2] = S cos(A,R), S cos(A,R)^2, #(cos(T,A) > cos(T,R)): thread j takes rows j, j + 256, ... in
// order, then wave trees and waves 0..3 in order.
__global__ __launch_bounds__(256) void clip_score_sum_kernel(int n, int has_text, double* __restrict__ out) {
  __shared__ double red[3][4];
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += 256) {
    const double c = out[2L * n + i];
    v[0] += c;
    v[1] += c * c;
    v[2] += (has_text && out[i] > out[n + i]) ? 1.0 : 0.0;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    v[j] = wave_sum_f64(v[j]);
    if (lane == 0) red[j][wave] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int j = threadIdx.x;
    out[3L * n + j] = ((red[j][0] + red[j][1]) + red[j][2]) + red[j][3];
  }
}

bool grid_ok(long threads) { return (threads + 255) / 256 <= 0x7fffffffL; }

}  // namespace

extern "C" int sdmoe_clip_quantise(const void* x, int is_fp32, int B, int H, int W, void* out, void* stream) {
  if (!x || !out || B <= 0 || H <= 0 || W <= 0) return SDMOE_EARG;
  if ((uintptr_t)x & (is_fp32 ? 3 : 1)) return SDMOE_ESHAPE;
  const int W4 = (W + 3) / 4;
  const long threads = (long)B * H * W4;
  if (!grid_ok(threads)) return SDMOE_ESHAPE;
  const int dwords = (W % 4 == 0) && !((uintptr_t)out & 3);
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (is_fp32)
    quantise_kernel<float><<<blocks, 256, 0, s>>>((const float*)x, (uint8_t*)out, B, H, W, W4, dwords);
  else
    quantise_kernel<half_t><<<blocks, 256, 0, s>>>((const half_t*)x, (uint8_t*)out, B, H, W, W4, dwords);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_clip_resample_h(const void* in, long in_bstride, int B, int H, int W, int row0, int nrows,
                                     const int* bounds, const int* kk, int ksize, int S, void* tmp, void* stream) {
  if (!in || !bounds || !kk || !tmp) return SDMOE_EARG;
  if (B <= 0 || H <= 0 || W <= 0 || S <= 0 || ksize <= 0 || nrows <= 0) return SDMOE_EARG;
  if (row0 < 0 || (long)row0 + nrows > H || in_bstride < (long)H * W * 3) return SDMOE_EARG;
  if (((uintptr_t)bounds | (uintptr_t)kk) & 3) return SDMOE_ESHAPE;
  const long threads = (long)B * nrows * S;
  if (!grid_ok(threads)) return SDMOE_ESHAPE;
  resample_h_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (const uint8_t*)in, in_bstride, W, row0, nrows, bounds, kk, ksize, S, B, (uint8_t*)tmp);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_clip_resample_v(const void* tmp, int B, int row0, int nrows, const int* bounds, const int* kk,
                                     int ksize, int S, int patch, const float* mean, const float* std, void* u8out,
                                     void* A, long lda, int kpad, void* stream) {
  if (!tmp || !bounds || !kk || (!u8out && !A)) return SDMOE_EARG;
  if (B <= 0 || S <= 0 || ksize <= 0 || nrows <= 0 || row0 < 0) return SDMOE_EARG;
  if (((uintptr_t)bounds | (uintptr_t)kk) & 3) return SDMOE_ESHAPE;
  NormC nc = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
  if (A) {
    if (!mean || !std) return SDMOE_EARG;
    if (patch <= 0 || S % patch || kpad < 3L * patch * patch || lda < kpad || ((uintptr_t)A & 1)) return SDMOE_ESHAPE;
    for (int c = 0; c < 3; ++c) {
      nc.mean[c] = mean[c];
      nc.std[c] = std[c];
    }
  } else {
    patch = S;
  }
  const long threads = (long)B * S * S;
  if (!grid_ok(threads)) return SDMOE_ESHAPE;
  resample_v_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (const uint8_t*)tmp, row0, nrows, bounds, kk, ksize, S, B, patch, nc, (uint8_t*)u8out, (half_t*)A, lda, kpad);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_clip_scores(const void* T, long ldt, const void* A, long lda, const void* R, long ldr, int n,
                                 int D, double* out, void* stream) {
  if (!A || !R || !out || n <= 0 || D <= 0) return SDMOE_EARG;
  if (lda < D || ldr < D || (T && ldt < D)) return SDMOE_EARG;
  if (((uintptr_t)A | (uintptr_t)R | (uintptr_t)T) & 1) return SDMOE_ESHAPE;
  if ((uintptr_t)out & 7) return SDMOE_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  clip_cos_kernel<<<(unsigned)n, 64, 0, s>>>((const half_t*)T, ldt, (const half_t*)A, lda, (const half_t*)R, ldr, n,
                                             D, out);
  SDMOE_CHECK_LAUNCH();
  clip_score_sum_kernel<<<1, 256, 0, s>>>(n, T ? 1 : 0, out);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
