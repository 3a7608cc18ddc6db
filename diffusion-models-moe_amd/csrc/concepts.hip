// The concept checkers' decision step on the device (the reference's benchmarks/concept_checkers.py runs, per prompt
// and per checker, its own fp32 CLIP text pass, a mean over the 77 token rows, an L2 normalisation, dot products
// against a bank of concept features and a few Python comparisons, and hands a concept name back to the host), gfx950:
//   sdmoe_text_pool      fp16 hidden-state rows [nseq * L, D] -> float64 features: per sequence p = mean of its L rows,
//     f = p / |p| (IEEE division, no epsilon: a zero block gives NaN, as the reference); per run of `group` sequences
//     the mean of their f in sequence order, re-normalised if asked. group = 1: a prompt's feature; group = n_objects:
//     a bank row (embed_all_objects / embed_anchor_prompts: not re-normalised; no_concept_features: re-normalised).
//     The reference normalises object_features twice (concept_checkers.py:55, :59); on a unit vector the second pass
//     is a no-op to within an ulp in float64, so it is done once here.
//   sdmoe_concept_route  one launch per batch: pool each prompt's rows (group = 1), sims[b][r] = f_b . bank[r], then
//     the checker groups' rule (first arg-max row, strict comparisons, NaN never fires) and the prompt's 32-bit select
//     word, the operand of sdmoe_wmask_union_sets.
// float64 throughout, one fixed summation order, no atomics: results are bit-identical from run to run.
//   Pooling: one block of 256 threads per sequence. Thread (s, c) owns the 8 columns of chunk c (one 16-byte load per
//   row when the pointer and the row stride are 16-byte aligned and the chunk lies inside D, else eight 2-byte loads)
//   and sums rows s, s + S, ... in order, S = 256 / (chunks rounded up to a power of two); the S slices are added in
//   slice order through LDS. The squared norm is the 8 columns in order, a wave butterfly, then waves 0..3 in order.
//   Dot products: one wave per bank row, lane j takes columns j, j + 64, ... with one fma chain, then the butterfly:
//   the same lane / column order for every row, so identical bank rows give identical sims; the group rule evaluates
//   its rows with the same function, so what it compares is what sims_out holds, bit for bit.
// Every global access is guarded by the sequence's own bounds; group records and row bits come from device memory
// and are range-checked in the kernel (a record that points outside the bank never fires, a bit outside 0..31 is
// ignored).
#include "common.h"
#include "../../include/sdmoe.h"

namespace {

constexpr int POOL_THREADS = 256;
constexpr int POOL_MAX_D = 2048;  // 256 chunks of 8 columns

SDMOE_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over the block of v: wave butterflies, then waves 0..3 in order. red: 4 doubles of LDS, free again on return.
SDMOE_DEV double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}

// f[0..7] = columns 8c .. 8c + 7 of the unit mean of x's L rows, valid in the threads of slice 0 (tid < 1 << cshift)
// whose chunk starts inside D (zero elsewhere). part: 256 * 8 doubles of LDS, red: 4.
SDMOE_DEV void pool_unit(const half_t* __restrict__ x, long ldx, int L, int D, int vec, int cshift, double* part,
                         double* red, double (&f)[8]) {
  const int tid = threadIdx.x;
  const int c = tid & ((1 << cshift) - 1), s = tid >> cshift, S = POOL_THREADS >> cshift;
  const int col0 = c * 8;
  const bool full = vec && col0 + 8 <= D;
  double acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0;
  if (col0 < D) {
    for (int l = s; l < L; l += S) {
      const half_t* row = x + (long)l * ldx + col0;
      if (full) {
        const half8 h = *reinterpret_cast<const half8*>(row);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (double)h[j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (col0 + j < D) acc[j] += (double)row[j];
      }
    }
  }
  if (S > 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) part[tid * 8 + j] = acc[j];
    __syncthreads();
    if (s == 0) {
      for (int q = 1; q < S; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += part[((q << cshift) + c) * 8 + j];
    }
    __syncthreads();
  }
  double sq = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc[j] = s == 0 ? acc[j] / (double)L : 0.0;
    sq = __builtin_fma(acc[j], acc[j], sq);
  }
  const double norm = __builtin_sqrt(block_sum_f64(sq, red));
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = acc[j] / norm;
}

__global__ __launch_bounds__(POOL_THREADS) void text_pool_kernel(const half_t* __restrict__ X, long ldx, int L, int D,
                                                                 int group, int renorm, int vec, int cshift,
                                                                 double* __restrict__ out, long ldo) {
  __shared__ double part[POOL_THREADS * 8];
  __shared__ double red[4];
  const long g = blockIdx.x;
  const int tid = threadIdx.x;
  const bool owner = tid < (1 << cshift);
  double m[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] = 0.0;
  for (int q = 0; q < group; ++q) {
    double f[8];
    pool_unit(X + (g * group + q) * L * ldx, ldx, L, D, vec, cshift, part, red, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] += f[j];
  }
  double sq = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = (owner && tid * 8 + j < D) ? m[j] / (double)group : 0.0;
    sq = __builtin_fma(m[j], m[j], sq);
  }
  if (renorm) {
    const double norm = __builtin_sqrt(block_sum_f64(sq, red));
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = m[j] / norm;
  }
  if (owner) {
    double* o = out + g * ldo + tid * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (tid * 8 + j < D) o[j] = m[j];
  }
}

// f . b over D columns, the same value in every lane.
SDMOE_DEV double wave_dot(const double* f, const double* __restrict__ b, int D) {
  double v = 0.0;
  for (int j = threadIdx.x & 63; j < D; j += 64) v = __builtin_fma(f[j], b[j], v);
  return wave_sum_f64(v);
}

__global__ __launch_bounds__(POOL_THREADS) void concept_route_kernel(
    const half_t* __restrict__ X, long ldx, int L, int D, int vec, int cshift, const double* __restrict__ bank,
    long ldb, int R, const int* __restrict__ row_bit, const sdmoe_concept_group* __restrict__ groups, int G,
    const unsigned* __restrict__ preset, unsigned* __restrict__ select_out, double* __restrict__ sims_out) {
  __shared__ double part[POOL_THREADS * 8];
  __shared__ double fs[POOL_MAX_D];
  __shared__ double red[4];
  __shared__ unsigned wsel[4];
  const long b = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6;
  double f[8];
  pool_unit(X + b * L * ldx, ldx, L, D, vec, cshift, part, red, f);
  if (tid < (1 << cshift)) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (tid * 8 + j < D) fs[tid * 8 + j] = f[j];
  }
  __syncthreads();
  if (sims_out) {
    for (int r = wave; r < R; r += 4) {
      const double d = wave_dot(fs, bank + (long)r * ldb, D);
      if ((tid & 63) == 0) sims_out[b * R + r] = d;
    }
  }
  unsigned word = 0;
  for (int g = wave; g < G; g += 4) {
    const sdmoe_concept_group q = groups[g];
    if (q.row0 < 0 || q.row1 > R || q.row0 >= q.row1 || q.neg_row < 0 || q.neg_row >= R || q.anchor_row >= R) continue;
    double m = wave_dot(fs, bank + (long)q.row0 * ldb, D);
    int best = q.row0;
    for (int r = q.row0 + 1; r < q.row1; ++r) {
      const double d = wave_dot(fs, bank + (long)r * ldb, D);
      if (d > m) {  // strict: the first row reaching the maximum stays
        m = d;
        best = r;
      }
    }
    const double neg = wave_dot(fs, bank + (long)q.neg_row * ldb, D);
    bool fire = m > neg && m > q.threshold;
    if (!fire && q.anchor_row >= 0) fire = wave_dot(fs, bank + (long)q.anchor_row * ldb, D) > neg;
    const int bit = row_bit[best];
    if (fire && bit >= 0 && bit < 32) word |= 1u << bit;
  }
  if ((tid & 63) == 0) wsel[wave] = word;
  __syncthreads();
  if (tid == 0) select_out[b] = (preset ? preset[b] : 0u) | wsel[0] | wsel[1] | wsel[2] | wsel[3];
}

// log2 of the chunk count rounded up to a power of two (D <= 2048: at most 8)
int chunk_shift(int D) {
  const int chunks = (D + 7) / 8;
  int sh = 0;
  while ((1 << sh) < chunks) ++sh;
  return sh;
}

int rows_vec(const void* X, long ldx) { return !((uintptr_t)X & 15) && ldx % 8 == 0; }

}  // namespace

extern "C" int sdmoe_text_pool(const void* X, long ldx, int nseq, int L, int D, int group, int renorm, double* out,
                               long ldo, void* stream) {
  if (nseq == 0) return SDMOE_OK;
  if (!X || !out || nseq < 0 || L <= 0 || D <= 0 || group <= 0) return SDMOE_EARG;
  if (nseq % group || ldx < D || ldo < D) return SDMOE_EARG;
  if (D > POOL_MAX_D) return SDMOE_EUNSUP;
  if (((uintptr_t)X & 1) || ((uintptr_t)out & 7)) return SDMOE_ESHAPE;
  text_pool_kernel<<<(unsigned)(nseq / group), POOL_THREADS, 0, (hipStream_t)stream>>>(
      (const half_t*)X, ldx, L, D, group, renorm ? 1 : 0, rows_vec(X, ldx), chunk_shift(D), out, ldo);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_concept_route(const void* X, long ldx, int nprompt, int L, int D, const double* bank, long ldb,
                                   int R, const int* row_bit, const sdmoe_concept_group* groups, int G,
                                   const unsigned* preset, unsigned* select_out, double* sims_out, void* stream) {
  if (nprompt == 0) return SDMOE_OK;
  if (!X || !bank || !row_bit || !select_out || nprompt < 0 || L <= 0 || D <= 0 || R <= 0 || G < 0) return SDMOE_EARG;
  if ((G > 0 && !groups) || ldx < D || ldb < D) return SDMOE_EARG;
  if (D > POOL_MAX_D) return SDMOE_EUNSUP;
  if (((uintptr_t)X & 1) || (((uintptr_t)bank | (uintptr_t)sims_out | (uintptr_t)groups) & 7)) return SDMOE_ESHAPE;
  if (((uintptr_t)row_bit | (uintptr_t)preset | (uintptr_t)select_out) & 3) return SDMOE_ESHAPE;
  concept_route_kernel<<<(unsigned)nprompt, POOL_THREADS, 0, (hipStream_t)stream>>>(
      (const half_t*)X, ldx, L, D, rows_vec(X, ldx), chunk_shift(D), bank, ldb, R, row_bit, groups, G, preset,
      select_out, sims_out);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
