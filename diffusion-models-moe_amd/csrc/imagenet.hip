// The parts of an ImageNet classification CNN (torchvision ResNet-50) that the U-Net kernels lack, and the object-
// erasure score reduction (the reference's benchmarks/object_erase.py:247-302 runs resnet50 on the host one PNG per
// call and matches the top-5 names in Python), gfx950:
//   sdmoe_stem_rows      uint8 [B, S, S, 3] -> the fp16 A operand of the 7x7 / stride 2 / padding 3 stem as a GEMM
//     (im2col rows, normalised in the store as sdmoe_clip_resample_v does; padding taps and columns are zero).
//   sdmoe_maxpool3x3s2   NHWC fp16 max pooling, window 3, stride 2, padding 1 (padding never wins, NaN propagates).
//   sdmoe_avgpool_rows   per (image, channel) mean of HW rows: fp32 sum in row order, one rounding.
//   sdmoe_add_relu       out = max(a + b, 0): fp32 sum, one rounding (the bottleneck's residual join).
//   sdmoe_topk_hits      per image the k best classes (descending; ties to the lower id; NaN first), whether one of
//     them is set in the label's row of a bit table, and the number of such images.
// All five stream: one thread per 8 fp16 (16 bytes) where pointers and strides allow, a narrow element-wise path
// otherwise. No atomics; every sum has a fixed order, so results are bit-identical from run to run. Every access is
// guarded by the thread's own bounds.
#include "common.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int STEM_K = 147;  // 3 channels x 7 x 7 taps

template <bool VEC>
SDMOE_DEV half8 load8(const half_t* p) {
  if (VEC) return *reinterpret_cast<const half8*>(p);
  half8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = p[j];
  return v;
}

template <bool VEC>
SDMOE_DEV void store8(half_t* p, half8 v) {
  if (VEC) {
    *reinterpret_cast<half8*>(p) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = v[j];
  }
}

bool aligned16(const void* p, long ld) { return !((uintptr_t)p & 15) && ld % 8 == 0; }
bool grid_ok(long threads) { return (threads + 255) / 256 <= 0x7fffffffL; }

struct NormC {
  float mean[3], std[3];
};

// fp16(((u8 * (1/255)) - mean) / std), every step rounded to fp32 as torchvision's to_tensor + normalize do: no
// contraction of the multiply and the subtraction into one fma, IEEE division (clip_image.hip's clip_normalise).
SDMOE_DEV half_t stem_normalise(unsigned q, float mean, float std) {
#pragma clang fp contract(off)
  const float v = (float)q * (1.0f / 255.0f);
  const float d = v - mean;
  return (half_t)(d / std);
}

// A[b So^2 + oy So + ox, c 49 + ky 7 + kx] = normalise(in[b, 2 oy - 3 + ky, 2 ox - 3 + kx, c]), 0 outside the image
// and in columns [147, kpad). One thread per 8 columns of one row: the byte reads hit the cache (an output row
// re-reads 147 bytes its neighbours share), the 16-byte stores are the traffic.
template <bool VEC>
__global__ __launch_bounds__(256) void stem_rows_kernel(const uint8_t* __restrict__ in, int B, int S, int So,
                                                        NormC nc, half_t* __restrict__ A, long lda, int kpad,
                                                        int chunks) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * So * So * chunks) return;
  const int ch = (int)(idx % chunks);
  const long row = idx / chunks;  // (b So + oy) So + ox
  const int ox = (int)(row % So);
  const long boy = row / So;
  const int oy = (int)(boy % So);
  const long b = boy / So;
  const uint8_t* img = in + b * (long)S * S * 3;
  half8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = ch * 8 + j;
    half_t h = (half_t)0.0f;
    if (col < STEM_K) {
      const int c = col / 49, t = col - c * 49, ky = t / 7, kx = t - ky * 7;
      const int y = 2 * oy - 3 + ky, x = 2 * ox - 3 + kx;
      if (y >= 0 && y < S && x >= 0 && x < S)
        h = stem_normalise(img[((long)y * S + x) * 3 + c], nc.mean[c], nc.std[c]);
    }
    v[j] = h;
  }
  half_t* dst = A + row * lda + ch * 8;
  if (VEC) {
    store8<true>(dst, v);
  } else {
    for (int j = 0; j < 8 && ch * 8 + j < kpad; ++j) dst[j] = v[j];
  }
}

// torch's max_pool2d update: a value replaces the running maximum when it is greater or NaN, from -inf, window rows
// then columns -- so the first of equal values (+0 / -0) stays and a NaN is never lost.
SDMOE_DEV half_t pool_max(half_t m, half_t v) { return (v > m || v != v) ? v : m; }

template <bool VEC>
__global__ __launch_bounds__(256) void maxpool_kernel(const half_t* __restrict__ X, long ldx, int B, int H, int W,
                                                      int C8, int OH, int OW, half_t* __restrict__ Y, long ldy) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * OH * OW * C8) return;
  const int c8 = (int)(idx % C8);
  const long pix = idx / C8;  // (b OH + oy) OW + ox
  const int ox = (int)(pix % OW);
  const long boy = pix / OW;
  const int oy = (int)(boy % OH);
  const long b = boy / OH;
  const half_t ninf = __builtin_bit_cast(half_t, (unsigned short)0xfc00);
  half8 m;
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] = ninf;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int y = 2 * oy - 1 + ky;
    if (y < 0 || y >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int x = 2 * ox - 1 + kx;
      if (x < 0 || x >= W) continue;
      const half8 v = load8<VEC>(X + ((b * H + y) * W + x) * ldx + c8 * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = pool_max(m[j], v[j]);
    }
  }
  store8<VEC>(Y + pix * ldy + c8 * 8, m);
}

// out[b, c] = fp16((x[b HW, c] + x[b HW + 1, c] + ... in fp32, in row order) / HW). One thread per 8 channels of one
// image: consecutive threads read consecutive 16 bytes of a row.
template <bool VEC>
__global__ __launch_bounds__(256) void avgpool_kernel(const half_t* __restrict__ X, long ldx, int B, int HW, int C8,
                                                      half_t* __restrict__ Y, long ldy) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * C8) return;
  const int c8 = (int)(idx % C8);
  const long b = idx / C8;
  const half_t* src = X + b * HW * ldx + c8 * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < HW; ++r) {
    const half8 v = load8<VEC>(src + r * ldx);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
  }
  const float n = (float)HW;
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (half_t)(acc[j] / n);
  store8<VEC>(Y + b * ldy + c8 * 8, o);
}

// torch.relu(a + b) on fp16: the sum in fp32, rounded once; negative -> +0, -0 and NaN pass through.
SDMOE_DEV half_t add_relu1(half_t a, half_t b) {
  const half_t s = (half_t)((float)a + (float)b);
  return s < (half_t)0.0f ? (half_t)0.0f : s;
}

// One thread per 8 elements; a and b may alias out (each thread reads its elements before it writes them).
template <bool VEC>
__global__ __launch_bounds__(256) void add_relu_kernel(const half_t* a, const half_t* b, half_t* out, long n) {
  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  if (VEC && i0 + 8 <= n) {
    const half8 x = load8<true>(a + i0), y = load8<true>(b + i0);
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = add_relu1(x[j], y[j]);
    store8<true>(out + i0, o);
  } else {
    const long i1 = i0 + 8 < n ? i0 + 8 : n;
    for (long i = i0; i < i1; ++i) out[i] = add_relu1(a[i], b[i]);
  }
}

// Rank of a class: (logit, lower id first) as one unsigned key, larger = better. The 16 logit bits become an
// order-preserving unsigned (sign flip), -0 counts as +0 and every NaN ranks above +inf, as torch.topk places it.
SDMOE_DEV unsigned long long topk_key(half_t v, int id) {
  unsigned u = __builtin_bit_cast(unsigned short, v);
  if (u == 0x8000u) u = 0u;
  unsigned k = (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
  if ((u & 0x7fffu) > 0x7c00u) k = 0xffffu;
  return ((unsigned long long)k << 32) | (unsigned)(0x7fffffff - id);
}

SDMOE_DEV unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// One wave per image, k rounds: in each, every lane scans its classes (lane, lane + 64, ...) for the best key below
// the previous round's winner and the wave takes the maximum. Keys are distinct (the id is part of them), so the k
// winners are the k best in order. 0 is below every key, and k <= C leaves a candidate for every round.
__global__ __launch_bounds__(64) void topk_hits_kernel(const half_t* __restrict__ L, long ldl, int n, int C, int k,
                                                       const unsigned* __restrict__ table, int G, int words,
                                                       const int* __restrict__ label, int* __restrict__ topk,
                                                       int* __restrict__ hit) {
  const long i = blockIdx.x;
  const half_t* row = L + i * ldl;
  const int g = label[i];
  const bool g_ok = g >= 0 && g < G;
  unsigned long long prev = ~0ull;
  int any = 0;
  for (int r = 0; r < k; ++r) {
    unsigned long long best = 0ull;
    for (int c = threadIdx.x; c < C; c += 64) {
      const unsigned long long key = topk_key(row[c], c);
      if (key < prev && key > best) best = key;
    }
    best = wave_max_u64(best);
    prev = best;
    const int c = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
    if (threadIdx.x == 0) topk[i * k + r] = c;
    if (g_ok && c >= 0 && c < C) any |= (int)((table[(long)g * words + (c >> 5)] >> (c & 31)) & 1u);
  }
  if (threadIdx.x == 0) hit[i] = g_ok ? any : -1;
}

// total = sum of hit in image order (thread j takes images j, j + 256, ...; wave trees; waves 0..3 in order), or -1
// when a label was out of range.
__global__ __launch_bounds__(256) void hit_total_kernel(const int* __restrict__ hit, int n, int* __restrict__ total) {
  __shared__ int red[2][4];
  int s = 0, bad = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int h = hit[i];
    s += h > 0 ? h : 0;
    bad |= h < 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = s;
    red[1][wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    total[0] = (red[1][0] | red[1][1] | red[1][2] | red[1][3]) ? -1 : t;
  }
}

}  // namespace

extern "C" int sdmoe_stem_rows(const void* u8, int B, int S, const float* mean, const float* std, void* A, long lda,
                               int kpad, void* stream) {
  if (B == 0) return SDMOE_OK;
  if (!u8 || !A || !mean || !std || B < 0 || S <= 0) return SDMOE_EARG;
  if (kpad < STEM_K || lda < kpad || ((uintptr_t)A & 1)) return SDMOE_ESHAPE;
  NormC nc;
  for (int c = 0; c < 3; ++c) {
    nc.mean[c] = mean[c];
    nc.std[c] = std[c];
  }
  const int So = (S - 1) / 2 + 1, chunks = (kpad + 7) / 8;
  const long threads = (long)B * So * So * chunks;
  if (!grid_ok(threads)) return SDMOE_ESHAPE;
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (aligned16(A, lda) && kpad % 8 == 0)
    stem_rows_kernel<true><<<blocks, 256, 0, s>>>((const uint8_t*)u8, B, S, So, nc, (half_t*)A, lda, kpad, chunks);
  else
    stem_rows_kernel<false><<<blocks, 256, 0, s>>>((const uint8_t*)u8, B, S, So, nc, (half_t*)A, lda, kpad, chunks);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_maxpool3x3s2(const void* X, long ldx, int B, int H, int W, int C, void* Y, long ldy,
                                  void* stream) {
  if (B == 0) return SDMOE_OK;
  if (!X || !Y || B < 0 || H <= 0 || W <= 0 || C <= 0) return SDMOE_EARG;
  if (C % 8 || ldx < C || ldy < C || (((uintptr_t)X | (uintptr_t)Y) & 1)) return SDMOE_ESHAPE;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const long threads = (long)B * OH * OW * (C / 8);
  if (!grid_ok(threads)) return SDMOE_ESHAPE;
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (aligned16(X, ldx) && aligned16(Y, ldy))
    maxpool_kernel<true><<<blocks, 256, 0, s>>>((const half_t*)X, ldx, B, H, W, C / 8, OH, OW, (half_t*)Y, ldy);
  else
    maxpool_kernel<false><<<blocks, 256, 0, s>>>((const half_t*)X, ldx, B, H, W, C / 8, OH, OW, (half_t*)Y, ldy);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_avgpool_rows(const void* X, long ldx, int B, int HW, int C, void* Y, long ldy, void* stream) {
  if (B == 0) return SDMOE_OK;
  if (!X || !Y || B < 0 || HW <= 0 || C <= 0) return SDMOE_EARG;
  if (C % 8 || ldx < C || ldy < C || (((uintptr_t)X | (uintptr_t)Y) & 1)) return SDMOE_ESHAPE;
  const long threads = (long)B * (C / 8);
  if (!grid_ok(threads)) return SDMOE_ESHAPE;
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (aligned16(X, ldx) && aligned16(Y, ldy))
    avgpool_kernel<true><<<blocks, 256, 0, s>>>((const half_t*)X, ldx, B, HW, C / 8, (half_t*)Y, ldy);
  else
    avgpool_kernel<false><<<blocks, 256, 0, s>>>((const half_t*)X, ldx, B, HW, C / 8, (half_t*)Y, ldy);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_add_relu(const void* a, const void* b, void* out, long n, void* stream) {
  if (n == 0) return SDMOE_OK;
  if (!a || !b || !out || n < 0) return SDMOE_EARG;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 1) return SDMOE_ESHAPE;
  const long threads = (n + 7) / 8;
  if (!grid_ok(threads)) return SDMOE_ESHAPE;
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (!(((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15))
    add_relu_kernel<true><<<blocks, 256, 0, s>>>((const half_t*)a, (const half_t*)b, (half_t*)out, n);
  else
    add_relu_kernel<false><<<blocks, 256, 0, s>>>((const half_t*)a, (const half_t*)b, (half_t*)out, n);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_topk_hits(const void* logits, long ldl, int n, int C, int k, const unsigned* table, int G,
                               const int* label, int* topk, int* hit, int* total, void* stream) {
  if (n == 0) return SDMOE_OK;
  if (!logits || !table || !label || !topk || !hit || !total || n < 0 || C <= 0 || G <= 0) return SDMOE_EARG;
  if (k < 1 || k > 8 || k > C || ldl < C) return SDMOE_EARG;
  if ((uintptr_t)logits & 1) return SDMOE_ESHAPE;
  if (((uintptr_t)table | (uintptr_t)label | (uintptr_t)topk | (uintptr_t)hit | (uintptr_t)total) & 3)
    return SDMOE_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  topk_hits_kernel<<<(unsigned)n, 64, 0, s>>>((const half_t*)logits, ldl, n, C, k, table, G, (C + 31) / 32, label,
                                              topk, hit);
  SDMOE_CHECK_LAUNCH();
  hit_total_kernel<<<1, 256, 0, s>>>(hit, n, total);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
