// Device side of gemm.hip (included only there): the launch parameters, the modes, the one compile-time LDS layout
// (GemmLayout, evaluated by the kernel and by the host's planning alike), gemm_kernel and splitk_reduce_kernel. The
// kernel body is one function: every part cut out of it as a function changed some instantiation's registers.
#pragma once
#include <type_traits>
#include <utility>
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void_t;

struct GemmParams {
  const half_t* A; long lda;
  const half_t* W; long ldw;
  const half_t* bias;
  const half_t* coladd; long coladd_bstride;
  const half_t* R; long ldr;
  half_t* C; long ldc;
  float* part;  // split-K partial slabs [ksplit][M][N] fp32 (ld N), or null
  int M, N, K;
  int act;
  int rows_per_batch;
  int H, Wd, Cin, OH, OW, stride, upsample;
  int ksplit, kchunk;
  int kchunk2;  // halo conv: folded-shortcut K-steps (32 channels of A2 each) per split (kchunk = main slices per split)
  int mfast;  // tile order M-fastest (split-K grids, sdmoe_tune knob 14)
  int a_bytes, w_bytes;  // SRD num_records
  // routed-GEGLU epilogue (sdmoe_linear_geglu): W rows interleaved [value 2 | gate 2] per neuron pair, C is
  // the [M, N/2] product value * act(gate); score [M, ld_score] gets per-expert sums of act(gate) over
  // contiguous esize-neuron experts (neurons pre-permuted so every expert is contiguous)
  half_t* score; long ld_score;
  int esize;
  int res16;  // residual on the fp16 staging path (sdmoe_tune knob 8)
  int diag;  // diagnostics bits (sdmoe_tune knob 6, results garbage)
  int epi_direct;  // fp16 epilogue: stores straight from the fragments instead of LDS staging (knob 23 policy)
  // expert keep mask of the A operand (MODE_KEEP / MODE_KEEPW): keep[(k / 64) * M * 8 + m * 8 + (k % 64) / 8] bit
  // (k % 8) = neuron k of token m survives the top-k; the A fragments are ANDed with it after their LDS read
  const uint8_t* keep;
  int keep_bytes;
  // Wanda weight mask of the W operand (MODE_WMASK / MODE_KEEPW), the same K-step-major layout over W's rows:
  // wmask[(k / 64) * N * 8 + n * 8 + (k % 64) / 8] bit (k % 8) SET = W[n, k] removed (zeroed on the B fragments)
  const uint8_t* wmask;
  int wmask_bytes;
  // one Wanda mask per image (sdmoe_linear_masked_sets): image i = m / rows_per_batch takes the mask at wmask +
  // image_set[i] * wset_bytes (wmask_bytes = the extent of ONE set); null = the one mask at wmask
  const int* image_set;
  long wset_bytes;
  // LayerNorm folded into the GEMM (MODE_GEMM_LN / MODE_GEGLU_LN): C = rstd_m * (A W'^T - mean_m * wsum) + ln_bias
  // with W' = W diag(gamma) (fp16), wsum[n] = sum_k W'[n, k], ln_bias[n] = bias[n] + sum_k W[n, k] beta[k] (fp32,
  // sdmoe_ln_fold); mean_m / rstd_m over the K = C channels of row m, accumulated from the A tiles in LDS
  const float* ln_wsum;
  const float* ln_bias;
  float ln_eps;
  // MODE_CONV with a folded 1x1 shortcut (sdmoe_conv3x3_sc): K-steps past the 9 * Cin conv steps read A2 [M, K2]
  // (the block input at the output pixel, row stride lda2) against the shortcut weights appended to W's rows
  const half_t* A2; long lda2;
  int a2_bytes;
  // GroupNorm folded into the GEMM (sdmoe_linear_per_image): image i = m / rows_per_batch multiplies its own weights
  // W + i * w_bstride (0 = one weight set) and adds colf[i * colf_bstride + n] (fp32 per-image column add)
  long w_bstride;
  const float* colf; long colf_bstride;
  // routed GEGLU with act == GELU: the registered fp16 GELU table (gelu_tab_h), staged into LDS for the epilogue
  const half_t* gelu_tab;
  // halo conv: GroupNorm(+SiLU) of the main input applied to each staged halo slice (sdmoe_conv3x3_gn): per image
  // and channel fp32 scale / shift ([nimg][Cin]); null = the input is used as is
  const float* gn_scale; const float* gn_shift; int gn_silu;
};

constexpr unsigned OOB = 0x80000000u;  // > every num_records used here (tensors < 2 GiB)

SDMOE_DEV void bld16(__amdgpu_buffer_rsrc_t rs, char* lds_dst, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)lds_dst, 16, voff, soff, 0, 0);
}
// one wave's LDS writes made visible to its own later reads (per-wave staging areas: no workgroup barrier)
SDMOE_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int N>
SDMOE_DEV void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
SDMOE_DEV void vm_wait(int n) {  // s_waitcnt vmcnt(n) for the wave-uniform n (immediates only; smaller = safe)
  if (n >= 12) vm_wait<12>();
  else if (n == 11) vm_wait<11>();
  else if (n == 10) vm_wait<10>();
  else if (n == 9) vm_wait<9>();
  else if (n == 8) vm_wait<8>();
  else if (n == 7) vm_wait<7>();
  else if (n == 6) vm_wait<6>();
  else if (n == 5) vm_wait<5>();
  else if (n == 4) vm_wait<4>();
  else if (n == 3) vm_wait<3>();
  else if (n == 2) vm_wait<2>();
  else if (n == 1) vm_wait<1>();
  else vm_wait<0>();
}
// shared epilogue for one 8-column chunk: v += bias, coladd; act; + residual; store fp16
SDMOE_DEV void epilogue8(const GemmParams& p, int m, int n, float (&v)[8]) {
  if (p.bias) {
    half8 bb = *reinterpret_cast<const half8*>(p.bias + n);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += (float)bb[j];
  }
  if (p.coladd) {
    const int b = m / p.rows_per_batch;
    half8 cc = *reinterpret_cast<const half8*>(p.coladd + (long)b * p.coladd_bstride + n);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += (float)cc[j];
  }
  if (p.colf) {
    const float* cf = p.colf + (long)(m / p.rows_per_batch) * p.colf_bstride + n;
    const float4v c0 = *reinterpret_cast<const float4v*>(cf), c1 = *reinterpret_cast<const float4v*>(cf + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] += c0[j]; v[4 + j] += c1[j]; }
  }
  if (p.act != ACT_NONE) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = apply_act(v[j], p.act);
  }
  if (p.R) {
    half8 rr = *reinterpret_cast<const half8*>(p.R + (long)m * p.ldr + n);
    if (p.res16 && p.act == ACT_NONE) {
      // the fp16 staging path's order (knob 8): output rounded to fp16, residual added, rounded again -- so split-K
      // launches (this reduce) and unsplit ones give the same residual semantics for every shape
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (float)(half_t)v[j] + (float)rr[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += (float)rr[j];
    }
  }
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (half_t)v[j];
  if (p.diag & 8) {  // diagnostics: everything but the global store
    asm volatile("" ::"v"(o));
    return;
  }
  *reinterpret_cast<half8*>(p.C + (long)m * p.ldc + n) = o;
}

// GEGLU: GEMM loads, routed-GEGLU epilogue; KEEP: GEMM whose A operand is masked per (row, neuron) by keep bits;
// WMASK: W operand masked per (row, k) by Wanda bits; KEEPW: both (the routed FFN down projection under a Wanda mask)
// GEMM_LN / GEGLU_LN: GEMM / GEGLU with the LayerNorm of the A rows folded in (row statistics from the A tiles)
enum { MODE_GEMM = 0, MODE_CONV = 1, MODE_CONV_UP = 2, MODE_GEGLU = 3, MODE_KEEP = 4, MODE_WMASK = 5, MODE_KEEPW = 6,
       MODE_GEMM_LN = 7, MODE_GEGLU_LN = 8, MODE_CONVH64 = 9, MODE_CONVH32 = 10, MODE_CONVH16 = 11,
       MODE_CONVHUP64 = 12, MODE_CONVHUP32 = 13, MODE_CONVHUP16 = 14, MODE_GEGLU_GT = 15, MODE_CONV_UP2X = 16 };
// MODE_CONV_UP2X: the nearest-2x upsample conv collapsed to four 2x2 phase convs on the LOW-resolution image
// (sdmoe_conv_up2x): M = low-res pixels, N = 4 Cout (phase 2 py + px major), K = 4 Cin (64-channel slice, tap 2 a + c,
// channel). A tile's columns lie in one phase (Cout % BN == 0); tap (a, c) of output pixel (r, q) reads input pixel
// (r + py + a - 1, q + px + c - 1), zero outside; the epilogue stores row (b, r, q) to output row up2x_out_row()
// MODE_GEGLU_GT: the routed GEGLU with act = GELU from the registered table (its own instantiation: a third epilogue
// variant inside MODE_GEGLU pushed the 256x320 kernel past 256 VGPRs into scratch, 115 -> 494 us)
// halo-tiled stride-1 3x3 conv (MODE_CONVH<W>, image width W): a tile is BM / W whole output rows of one image; per
// 32-channel slice the (BM / W + 2) x (W + 2) input halo is staged in LDS ONCE and read by all 9 taps at shifted
// rows, instead of 9 shifted A tiles (A pieces per K-step 27/9 instead of BM / 16)
// MODE_CONVHUP<OW>: the same for the fused nearest-2x upsample conv (output width OW): the halo is the
// (BM / OW / 2 + 2) x (OW / 2 + 2) LOW-resolution input patch; output pixel (oh, ow) at tap (kh, kw) reads input
// ((oh + kh - 1) >> 1, (ow + kw - 1) >> 1) -- two lanes of a fragment share each input row (an LDS broadcast)
// MODE_CONV_UP2X row map, shared by the fp16 epilogue and splitk_reduce_up2x_kernel: GEMM row m = low-res pixel (b, r, q)
// of nimg H x W images, phase ph = 2 py + px -> row of the 2H x 2W output image
SDMOE_DEV long up2x_out_row(int m, int H, int W, int ph) {
  const int hw = H * W;
  const int b = m / hw, rq = m - b * hw;
  const int r = rq / W, q = rq - r * W;
  return ((long)(b * 2 * H + 2 * r + (ph >> 1)) * (2 * W) + 2 * q + (ph & 1));
}
constexpr bool mode_halo(int mode) { return mode >= MODE_CONVH64 && mode <= MODE_CONVHUP16; }
constexpr bool mode_halo_up(int mode) { return mode >= MODE_CONVHUP64 && mode <= MODE_CONVHUP16; }
constexpr int halo_w(int mode) {  // OUTPUT width
  return (mode == MODE_CONVH64 || mode == MODE_CONVHUP64) ? 64 : ((mode == MODE_CONVH32 || mode == MODE_CONVHUP32) ? 32 : 16);
}
constexpr bool mode_akeep(int mode) { return mode == MODE_KEEP || mode == MODE_KEEPW; }
constexpr bool mode_wmask(int mode) { return mode == MODE_WMASK || mode == MODE_KEEPW; }
constexpr bool mode_geglu(int mode) { return mode == MODE_GEGLU || mode == MODE_GEGLU_LN || mode == MODE_GEGLU_GT; }
constexpr bool mode_ln(int mode) { return mode == MODE_GEMM_LN || mode == MODE_GEGLU_LN; }

// LDS bytes one ring stage holds besides the A/B tiles: the mask bytes of the tile's rows for one 64-deep K-step
// (A keep: BM rows x 8 bytes; W mask: BN rows x 8 bytes; each in whole 1-KiB LDS-DMA pieces)
constexpr int keep_a_bytes(int bm, int mode) { return mode_akeep(mode) ? ((bm * 8 + 1023) / 1024) * 1024 : 0; }
constexpr int keep_w_bytes(int bn, int mode) { return mode_wmask(mode) ? ((bn * 8 + 1023) / 1024) * 1024 : 0; }
constexpr int keep_stage_bytes(int bm, int bn, int mode) { return keep_a_bytes(bm, mode) + keep_w_bytes(bn, mode); }
// MODE_KEEP: a keep byte (8 neurons) -> 4 x 32-bit masks of the 8 fp16 halves, one ds_read_b128 per A fragment
// (round 5: two dependent ds_read_b64 from a 16-entry nibble table: keep-masked down projections 1.5-3 % slower);
// the W-masked modes keep the nibble table (the byte table there cost the 128x160 KEEPW tile its second workgroup
// per CU: 173 -> 268 VGPRs)
constexpr int keep_lut_bytes(int mode) { return mode == MODE_KEEP ? 256 * 16 : 16 * 8; }

constexpr int GN_MAXC = 1280;               // halo conv GroupNorm: fp32 scale + shift per channel
constexpr int TAB_BYTES = GELU_TAB_N * 2;   // routed GEGLU under GELU: the fp16 activation table

// ---- the layout: every compile-time size and LDS offset of gemm_kernel<bm, bn, wmw, wnw, mode, nstage, bk>, written
// once for the kernel and for the host's planning: GemmLayout{bm, bn, wmw, wnw, mode, nstage, bk}, the rest follows
struct GemmLayout {
  int bm, bn, wmw, wnw, mode, nstage, bk;
  bool keep = mode_akeep(mode) || mode_wmask(mode), halo = mode_halo(mode), hup = mode_halo_up(mode), ln = mode_ln(mode);
  int RB = bk * 2, CPRW = bk / 8, RPP = 1024 / RB;  // LDS row bytes, 16-B chunks per row, rows per 1-KiB LDS-DMA piece
  int NW = wmw * wnw, NT = 64 * NW;                 // waves, threads
  int WM = bm / wmw, WN = bn / wnw, FM = WM / 16, FN = WN / 16;  // per-wave output tile and its 16x16 fragments
  int A_INS = bm / RPP, B_INS = bn / RPP;           // 1-KiB LDS-DMA wave-instructions per stage
  int A_PW = (A_INS + NW - 1) / NW, B_PW = (B_INS + NW - 1) / NW;
  int KA_INS = keep_a_bytes(bm, mode) / 1024;       // A keep pieces per stage
  int K_INS = keep_stage_bytes(bm, bn, mode) / 1024;  // A keep + W mask pieces per stage (<= NW)
  // every wave issues exactly PER_WAVE pieces per stage (surplus -> dummy slot; keep: one per wave, waves >= K_INS
  // repeat piece 0)
  int PER_WAVE = A_PW + B_PW + (keep ? 1 : 0);
  int STAGE_AB = (bm + bn) * bk * 2;
  bool PADDED = (A_PW * NW != A_INS) || (B_PW * NW != B_INS);
  int KEEP_OFF = STAGE_AB + (PADDED ? 1024 : 0), WKEEP_OFF = KEEP_OFF + keep_a_bytes(bm, mode);
  int STAGE = KEEP_OFF + keep_stage_bytes(bm, bn, mode);
  // halo conv (MODE_CONVH*): two halo buffers of H_INS pieces (input rows BM / HW_ + 2 at a pitch of HW_ + 8 pixels: a
  // multiple of 8 rows, so a fragment's swizzle depends only on its lane and tap column) + an NSTAGE ring of B tiles
  int HW_ = halo_w(mode), HWIN = hup ? HW_ / 2 : HW_, HP = HWIN + 8, HR = bm / HW_;
  int HROWS_IN = hup ? HR / 2 + 2 : HR + 2;  // input rows of the halo
  int H_INS = halo ? (HROWS_IN * HP + RPP - 1) / RPP : 0;
  // a halo buffer also holds two A2 ring slots (BM rows x 32 channels) of the folded-shortcut K-steps
  int A2BYTES = bm * RB;
  int HBYTES = H_INS * 1024 > 2 * A2BYTES ? H_INS * 1024 : 2 * A2BYTES, BSTAGE = bn * RB;
  int RING = halo ? 2 * HBYTES + nstage * BSTAGE : nstage * STAGE;  // main-loop LDS
  int RINGX = RING + (halo && !hup ? GN_MAXC * 8 : 0);             // + the halo conv's GroupNorm scale / shift
  // epilogue staging: fp16 final values (row stride RS16 halves: 16-B aligned rows, conflict-free b64 stores of the
  // swapped fragments) in NPASS16 passes; the fp32 path (activation, residual) in NPASS passes; GEGLU: its own passes
  int RS16 = WN + 8;
  int NPASS16 = (NW * WM * RS16 * 2 <= RING) ? 1 : (NW * (WM / 2) * RS16 * 2 <= RING) ? 2
                : ((NW * (WM / 4) * RS16 * 2 <= RING) ? 4 : 8);
  int WN_PAD = WN + 4;
  int NPASS = (NW * (WM / 2) * WN_PAD * 4 <= RING) ? 2 : ((NW * (WM / 4) * WN_PAD * 4 <= RING) ? 4 : 8);
  int EPI = NW * (WM / NPASS) * WN_PAD * 4, EPI16 = NW * (WM / NPASS16) * RS16 * 2;
  int SMEM0 = (RINGX > EPI) ? (RINGX > EPI16 ? RINGX : EPI16) : (EPI > EPI16 ? EPI : EPI16);
  int LUT_OFF = SMEM0;                 // the keep tables (byte or nibble -> lane masks) behind everything
  int SMEM1 = SMEM0 + (keep ? keep_lut_bytes(mode) : 0);
  // LN: per tile row (rstd, -mean*rstd), then the tile's BN columns of wsum and ln_bias (fp32), behind everything;
  // LN_IPL 16-B chunks of the row statistics per lane and K-step
  int LN_ROW_OFF = SMEM1, LN_COL_OFF = SMEM1 + bm * 8, LN_IPL = ln ? (bm * 8) / NT : 1;
  int SMEM = SMEM1 + (ln ? bm * 8 + bn * 8 : 0);
  // GEGLU epilogue staging; the GELU table in the top of a ring stage during the last K-step where a stage holds it,
  // else behind the staging
  int G_STAGING = NW * 2 * (16 * (FM % 2 == 0 ? 2 : 1)) * (WN / 2) * 2 + NW * WN * 4;
  bool TAB_PREFETCH = mode == MODE_GEGLU_GT && STAGE >= TAB_BYTES && G_STAGING <= STAGE;
  int TAB_LATE_OFF = ((G_STAGING + 1023) / 1024) * 1024;
  bool TAB_OK = mode == MODE_GEGLU_GT && (TAB_PREFETCH || TAB_LATE_OFF + TAB_BYTES <= SMEM1);
};

// one instantiation's template arguments, mode predicates and layout
template <int BM_, int BN_, int WMW_, int WNW_, int MODE_, int NSTAGE_, int BKT_>
struct GemmCfg {
  // BK: K per stage, 64 (128-B rows) or 32 (64-B rows, deeper ring)
  static constexpr int BM = BM_, BN = BN_, WMW = WMW_, WNW = WNW_, MODE = MODE_, NSTAGE = NSTAGE_, BK = BKT_;
  static constexpr bool UP2X = MODE == MODE_CONV_UP2X;
  static constexpr bool CONV = MODE == MODE_CONV || MODE == MODE_CONV_UP || UP2X, GEGLU = mode_geglu(MODE), LN = mode_ln(MODE);
  static constexpr bool AKEEP = mode_akeep(MODE), WKEEP = mode_wmask(MODE), KEEP = AKEEP || WKEEP;
  static constexpr bool HALO = mode_halo(MODE), HUP = mode_halo_up(MODE);
  static constexpr GemmLayout lay() { return GemmLayout{BM, BN, WMW, WNW, MODE, NSTAGE, BK}; }
  static constexpr int swzk(int row) { return (row >> 1) & (BK / 8 - 1); }  // conflict-free b128 fragment reads
};

// Routed-GEGLU expert scores over one staged pass of a wave's tile: the activated gates (fp16) of RG rows x NH
// neurons, experts = contiguous S-neuron slices (neurons pre-permuted expert-major). score = fp32 sum in neuron order,
// rounded to fp16 (as sdmoe_geglu_route). Row-fastest lane mapping (lane -> row id % RG).
// acc + (float)h for the low / high fp16 half of x in ONE v_fma_mix_f32 (fma(h, 1.0, acc): the f16 -> f32 conversion
// is exact and the fma rounds once, so the result is bit-identical to cvt + add; the compiler folds fma(h, 1, acc)
// back into the two-instruction cvt + add)
SDMOE_DEV float add_f16_lo(float acc, unsigned x) {
  asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(x));
  return acc;
}
SDMOE_DEV float add_f16_hi(float acc, unsigned x) {
  asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(x));
  return acc;
}

template <int S, int NH, int RG>
SDMOE_DEV void expert_sums(const GemmParams& p, const half_t* sg, int mrow0, int n0, int lane) {
  constexpr int NE = NH / S;
  for (int id = lane; id < RG * NE; id += 64) {
    const int r = id % RG, e = id / RG;
    const int m = mrow0 + r;
    const half_t* rp = sg + r * NH + e * S;
    float acc = 0.f;
    if constexpr (S % 4 == 0) {  // 8-B aligned quads, summed in neuron order by mixed-precision fmas
#pragma unroll
      for (int q = 0; q < S / 4; ++q) {
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        const u2 x = *reinterpret_cast<const u2*>(rp + 4 * q);
        acc = add_f16_hi(add_f16_lo(acc, x[0]), x[0]);
        acc = add_f16_hi(add_f16_lo(acc, x[1]), x[1]);
      }
    } else {
#pragma unroll
      for (int t = 0; t < S; ++t) acc += (float)rp[t];
    }
    if (p.diag & 8) asm volatile("" ::"v"(acc));
    else if (m < p.M) p.score[(long)m * p.ld_score + n0 / 2 / S + e] = (half_t)acc;
  }
}

template <int BM, int BN, int WMW, int WNW, int MODE, int NSTAGE, int BKT>
__global__ __launch_bounds__(64 * WMW * WNW, (NSTAGE == 2 && (WMW * WNW == 4 || BM * BN <= 20480) ? 2 : 1)) void gemm_kernel(
    GemmParams p) {
  using G = GemmCfg<BM, BN, WMW, WNW, MODE, NSTAGE, BKT>;
  constexpr GemmLayout L = G::lay();
  constexpr int BK = BKT;
  static_assert(!G::KEEP || BKT == 64, "keep bytes are laid out per 64-deep K-step");
  static_assert(L.WM % 16 == 0 && L.WN % 16 == 0, "wave tile must be whole 16x16 fragments");
  static_assert(L.K_INS <= L.NW, "one keep piece per wave at most");
  static_assert(L.FM % L.NPASS == 0 && L.FM % L.NPASS16 == 0, "epilogue passes must split the wave's fragment rows");
  static_assert(!G::LN || ((BM * 8) % L.NT == 0 && BK == 64), "LN statistics: whole 16-B chunks per lane");
  static_assert(MODE != MODE_GEGLU_GT || L.TAB_OK, "GELU table must fit this tile's LDS");
  __shared__ __attribute__((aligned(1024))) char smem[L.SMEM];
  // LN row statistics: lane tid reads 16-B chunk (tid % 8) of tile rows tid / 8 + (NT / 8) t, t < LN_IPL, every
  // K-step (8 lanes cover one 128-B row: conflict-free), summing x and x^2 with v_dot2_f32_f16
  float ln_s1[L.LN_IPL], ln_s2[L.LN_IPL];
#pragma unroll
  for (int t = 0; t < L.LN_IPL; ++t) ln_s1[t] = ln_s2[t] = 0.f;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WNW, wc = wave % WNW;
  const int ntn = (p.N + BN - 1) / BN, ntm = (p.M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, ntn * ntm * p.ksplit);
  // tile order: (split, N-tile, M-tile) with the split fastest, or -- split-K grids under mfast -- the M-tile
  // fastest, so the workgroups xcd_remap puts on one XCD share (N-tile, split) weight slices in that XCD's L2
  int split, tn, tm;
  if (p.mfast) {
    tm = bid % ntm;
    const int r = bid / ntm;
    tn = r % ntn;
    split = r / ntn;
  } else {
    split = bid % p.ksplit;
    const int tile = bid / p.ksplit;
    tn = tile % ntn;
    tm = tile / ntn;
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int nk_total = p.K / BK;
  const int ks0 = split * p.kchunk;
  const int ks1 = min(nk_total, ks0 + p.kchunk);
  const int nk = ks1 - ks0;
  // MODE_CONV_UP2X: the phase this tile's columns lie in (Cout % BN == 0, host check) and its row / column shift
  const int up_ph = G::UP2X ? n0 / (p.N >> 2) : 0, up_py = up_ph >> 1, up_px = up_ph & 1;

  // ---- LDS-DMA sources: buffer loads through two SRDs (A, W); an out-of-range offset (OOB) is dropped by the
  // hardware range check and lands as zeros, which gives conv halo rows and M/N tails for free.
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, (short)0, p.a_bytes, 0x00020000);
  // per-image weights (sdmoe_linear_per_image): a tile never straddles two images (host check rows_per_batch % BM)
  const half_t* Wimg = p.w_bstride ? p.W + (long)(m0 / p.rows_per_batch) * p.w_bstride : p.W;
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)Wimg, (short)0, p.w_bytes, 0x00020000);
  const int lrow = lane / L.CPRW, lch = lane % L.CPRW;
  // A rows: wave w stages rows [8*(w*A_PW + j), +8); B rows likewise with B_PW
  unsigned avoff[L.A_PW];  // GEMM: byte offset of (row, pre-swizzled chunk); conv: of the centre-tap pixel
  unsigned amask[L.A_PW];  // conv: bit t = tap t in bounds (0 = M-tail row)
  int aoh[L.A_PW], aow[L.A_PW], ab_[L.A_PW];  // conv-upsample rows
  unsigned avoff2[L.A_PW];  // conv + shortcut: byte offset of (output pixel row, pre-swizzled chunk) in A2
  unsigned bvoff[L.B_PW];
#pragma unroll
  for (int j = 0; j < L.A_PW; ++j) {
    const int r = L.RPP * (j * L.NW + wave) + lrow;
    const unsigned chb = (unsigned)((lch ^ G::swzk(r)) * 16);
    const int m = m0 + r;
    avoff[j] = OOB; amask[j] = 0; aoh[j] = 0; aow[j] = 0; ab_[j] = 0; avoff2[j] = OOB;
    if (MODE == MODE_CONV && p.A2 && j * L.NW + wave < L.A_INS && m < p.M) avoff2[j] = (unsigned)((long)m * p.lda2 * 2) + chb;
    if (j * L.NW + wave < L.A_INS && m < p.M) {
      if (!G::CONV) {
        avoff[j] = (unsigned)((long)m * p.lda * 2) + chb;
      } else {
        const int hw = p.OH * p.OW;
        const int b = m / hw, rr = m - b * hw;
        const int oh = rr / p.OW, ow = rr - oh * p.OW;
        if (MODE == MODE_CONV) {
          const int ih = oh * p.stride, iw = ow * p.stride;  // centre tap (kh = kw = 1)
          avoff[j] = (unsigned)(((long)(b * p.H + ih) * p.Wd + iw) * p.lda * 2) + chb;
          unsigned msk = 0;
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const int y = ih + t / 3 - 1, x = iw + t % 3 - 1;
            msk |= (y >= 0 && y < p.H && x >= 0 && x < p.Wd) ? (1u << t) : 0u;
          }
          amask[j] = msk;
        } else if (G::UP2X) {  // tap-(1 - py, 1 - px) pixel = the low-res pixel itself; bit t = 2 a + c in bounds
          avoff[j] = (unsigned)(((long)(b * p.H + oh) * p.Wd + ow) * p.lda * 2) + chb;
          unsigned msk = 0;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int y = oh + up_py + (t >> 1) - 1, x = ow + up_px + (t & 1) - 1;
            msk |= (y >= 0 && y < p.H && x >= 0 && x < p.Wd) ? (1u << t) : 0u;
          }
          amask[j] = msk;
        } else {
          amask[j] = 1; avoff[j] = chb; aoh[j] = oh; aow[j] = ow; ab_[j] = b;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < L.B_PW; ++j) {
    const int r = L.RPP * (j * L.NW + wave) + lrow;
    const int n = n0 + r;
    bvoff[j] = (j * L.NW + wave < L.B_INS && n < p.N) ? (unsigned)((long)n * p.ldw * 2) + (unsigned)((lch ^ G::swzk(r)) * 16)
                                                  : OOB;
  }
  // mask pieces: wave w < KA_INS stages the A keep bytes of tile rows [128 w, 128 w + 128) (16 B = two rows per
  // lane), waves KA_INS .. K_INS-1 the W mask bytes of tile columns [128 (w - KA_INS), +128); the other waves
  // repeat piece 0 -- the same bytes to the same LDS place -- so every wave issues PER_WAVE instructions per stage
  // and the counted vmcnt waits stay uniform
  const int kpiece = G::KEEP && wave < L.K_INS ? wave : 0;
  const bool kpa = G::AKEEP && kpiece < L.KA_INS;  // wave-uniform: this wave's piece is A keep bytes (else W mask bytes)
  // per-image mask sets (sdmoe_linear_masked_sets): the tile's image picks the base of its set's mask -- one scalar
  // load per workgroup; a tile never straddles two images (host check rows_per_batch % BM)
  const uint8_t* wmask = p.wmask;
  if constexpr (G::WKEEP) {
    if (p.image_set) wmask += (long)p.image_set[m0 / p.rows_per_batch] * p.wset_bytes;
  }
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(
      kpa ? (void*)p.keep : (void*)wmask, (short)0, G::KEEP ? (kpa ? p.keep_bytes : p.wmask_bytes) : 0, 0x00020000);
  const unsigned kstride = kpa ? (unsigned)p.M * 8u : (unsigned)p.N * 8u;  // bytes per K-step of the mask layout
  unsigned kvoff = OOB;
  int kdst = L.KEEP_OFF;
  if constexpr (G::KEEP) {
    kvoff = kpa ? (unsigned)((m0 + 128 * kpiece) * 8 + lane * 16)
                : (unsigned)((n0 + 128 * (kpiece - L.KA_INS)) * 8 + lane * 16);
    kdst = kpa ? L.KEEP_OFF + kpiece * 1024 : L.WKEEP_OFF + (kpiece - L.KA_INS) * 1024;
    // byte -> four 32-bit masks: entry e masks fp16 halves 0..7 by bits 0..7 of e (one ds_read_b128 per fragment;
    // round 5's 16-entry nibble table took two dependent ds_read_b64)
    if constexpr (MODE == MODE_KEEP) {
      for (int e = tid; e < 256; e += L.NT) {
        uint4v m;
#pragma unroll
        for (int d = 0; d < 4; ++d)
          m[d] = (((e >> (2 * d)) & 1) ? 0xFFFFu : 0u) | (((e >> (2 * d + 1)) & 1) ? 0xFFFF0000u : 0u);
        *reinterpret_cast<uint4v*>(smem + L.LUT_OFF + e * 16) = m;
      }
    } else if (tid < 16) {  // nibble -> two 32-bit masks
      const unsigned lo = ((tid & 1) ? 0xFFFFu : 0u) | ((tid & 2) ? 0xFFFF0000u : 0u);
      const unsigned hi = ((tid & 4) ? 0xFFFFu : 0u) | ((tid & 8) ? 0xFFFF0000u : 0u);
      *reinterpret_cast<uint2v*>(smem + L.LUT_OFF + tid * 8) = (uint2v){lo, hi};
    }
    __syncthreads();  // no LDS-DMA in flight yet
  }
  // LDS destination of wave-instruction j (surplus instructions of a padded tile land in a dummy 1-KiB slot)
  auto a_dst = [&](int j) { return (j * L.NW + wave < L.A_INS) ? (j * L.NW + wave) * 1024 : L.STAGE_AB; };
  auto b_dst = [&](int j) { return (j * L.NW + wave < L.B_INS) ? BM * BK * 2 + (j * L.NW + wave) * 1024 : L.STAGE_AB; };

  // conv K walk: (64-channel step, tap) advanced incrementally in scalar registers. Channel-step-major: the 9
  // consecutive K-steps of one 64-channel slice re-read the same activation rows (shifted by a tap), so a
  // workgroup's A working set is ~(BM + halo) x 128 B and stays in the XCD's L2 across the taps.
  // Folded shortcut (MODE_CONV, p.A2): channel steps st_c >= csl (= Cin / 64) are single K-steps of A2.
  const int csl = G::CONV ? p.Cin / BK : 0;
  const __amdgpu_buffer_rsrc_t rsA2 =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.A2, (short)0, p.A2 ? p.a2_bytes : 0, 0x00020000);
  constexpr int NTAP = G::UP2X ? 4 : 9;  // K-steps per 64-channel slice
  int st_c = G::CONV ? ks0 / NTAP : 0, st_tap = G::CONV ? ks0 - st_c * NTAP : 0;
  if (MODE == MODE_CONV && ks0 >= 9 * csl) { st_c = csl + (ks0 - 9 * csl); st_tap = 0; }

  auto issue_stage = [&](int ks, int buf) {
    char* sa = smem + buf * L.STAGE;
    const unsigned kb = (unsigned)(ks * BK * 2);
    if (p.diag & 16) {  // diagnostics: no A pieces (B only)
    } else if (!G::CONV) {
#pragma unroll
      for (int j = 0; j < L.A_PW; ++j) bld16(rsA, sa + a_dst(j), avoff[j], kb);
    } else if (MODE == MODE_CONV && st_c >= csl) {  // folded shortcut K-step (wave-uniform)
      const unsigned c2b = (unsigned)((st_c - csl) * BK * 2);
      ++st_c;
#pragma unroll
      for (int j = 0; j < L.A_PW; ++j) bld16(rsA2, sa + a_dst(j), avoff2[j] == OOB ? OOB : avoff2[j] + c2b, 0);
    } else if constexpr (G::UP2X) {  // tap (a, c) of the tile's phase: input pixel shifted by (py + a - 1, px + c - 1)
      const int tap = st_tap;
      const int c0b = st_c * BK * 2;
      if (++st_tap == 4) { st_tap = 0; ++st_c; }
      const unsigned tapoff =
          (unsigned)(((up_py + (tap >> 1) - 1) * p.Wd + (up_px + (tap & 1) - 1)) * (int)p.lda * 2 + c0b);
#pragma unroll
      for (int j = 0; j < L.A_PW; ++j) {
        const unsigned vo = ((amask[j] >> tap) & 1u) ? avoff[j] + tapoff : OOB;
        bld16(rsA, sa + a_dst(j), vo, 0);
      }
    } else {
      const int tap = st_tap;
      const int kh = tap >= 6 ? 2 : (tap >= 3 ? 1 : 0);
      const int kw = tap - 3 * kh;
      const int c0b = st_c * BK * 2;
      if (++st_tap == 9) { st_tap = 0; ++st_c; }
      if (MODE == MODE_CONV) {
        const unsigned tapoff = (unsigned)(((kh - 1) * p.Wd + (kw - 1)) * (int)p.lda * 2 + c0b);
#pragma unroll
        for (int j = 0; j < L.A_PW; ++j) {
          const unsigned vo = ((amask[j] >> tap) & 1u) ? avoff[j] + tapoff : OOB;
          bld16(rsA, sa + a_dst(j), vo, 0);
        }
      } else {
#pragma unroll
        for (int j = 0; j < L.A_PW; ++j) {
          const int uh = aoh[j] + kh - 1, uw = aow[j] + kw - 1;
          const bool ok = amask[j] && uh >= 0 && uh < 2 * p.H && uw >= 0 && uw < 2 * p.Wd;
          const unsigned vo =
              ok ? (unsigned)(((long)(ab_[j] * p.H + (uh >> 1)) * p.Wd + (uw >> 1)) * p.lda * 2) + avoff[j] + c0b
                 : OOB;
          bld16(rsA, sa + a_dst(j), vo, 0);
        }
      }
    }
    if (!(p.diag & 32)) {  // diagnostics: bit 5 = no B pieces (A only)
#pragma unroll
      for (int j = 0; j < L.B_PW; ++j) bld16(rsW, sa + b_dst(j), bvoff[j], kb);
    }
    if constexpr (G::KEEP) bld16(rsK, sa + kdst, kvoff, (unsigned)ks * kstride);
  };

  // routed GEGLU under GELU: the 32-KiB activation table goes to LDS by LDS-DMA (GELU_TAB_N / 512 pieces over the
  // waves) -- during the last K-step into the top of the ring stage nothing reads then (stage nk % NSTAGE: consumed
  // at step nk - NSTAGE, or never), when a stage holds it; otherwise after the main loop, behind the staging area
  auto issue_gelu_tab = [&](char* dst) {
    const __amdgpu_buffer_rsrc_t rsT = __builtin_amdgcn_make_buffer_rsrc((void*)p.gelu_tab, (short)0, TAB_BYTES, 0x00020000);
#pragma unroll
    for (int j = 0; j < (TAB_BYTES / 1024 + L.NW - 1) / L.NW; ++j) {
      const int piece = j * L.NW + wave;
      if (piece < TAB_BYTES / 1024) bld16(rsT, dst + piece * 1024, (unsigned)(piece * 1024 + lane * 16), 0);
    }
  };

  // C^T fragments (the MFMA's operands swapped): acc[i][j][r] = C[row wr*WM + 16 i + fr][col wc*WN + 16 j + 4 fg + r], 4
  // consecutive output columns of one row per lane, so the epilogue works on half4 / float4 row pieces (and the routed
  // GEGLU pairs value / gate columns with one lane swap).
  float4v acc[L.FM][L.FN];
#pragma unroll
  for (int i = 0; i < L.FM; ++i)
#pragma unroll
    for (int j = 0; j < L.FN; ++j) acc[i][j] = (float4v){0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fg = lane >> 4;
  if constexpr (G::HALO) {
    // ---- halo-tiled 3x3 conv main loop. Local K-steps: 9 per main 32-channel slice (tap t; the 9 taps unrolled: kh,
    // kw compile-time), then the folded shortcut's K-steps (32 channels of A2 at the output pixel each). Per step: a
    // counted wait for the NEXT step's B tile (older pieces -- this step's A2 tile, the halos -- with it), one barrier,
    // the MFMAs on the fragments read ahead at the end of the previous step (the DMA issue of the step after its first
    // MFMA group: A2(ks + 2), B(ks + 3), at t = 0 the next slice's halo into the other buffer), then the next step's B
    // fragments and first A pair. Round 5 read every step's fragments right behind its barrier: PMC of the 64x64
    // 320 -> 320 conv with the K-loop loads and the epilogue off (profiles/r06b_pmc_conv.txt) put the MFMA pipe at 61 %
    // busy with 32 % of the wave cycles in s_waitcnt / s_barrier -- ~800 idle cycles per 1280-cycle K-step.
    // A2 ring slots: slot s = k2 % 3 lives in halo buffer (nsl + (s == 2)) % 2 at offset (s == 1) * A2BYTES: slots 0 / 1
    // are in the buffer the last main slice does not read (their loads are issued during its taps 7 / 8), slot 2 in the
    // other one (issued after the first shortcut step's barrier).
    static_assert(BK == 32 && NSTAGE == 4 && BM % L.HW_ == 0 && L.WM % L.HW_ == 0 && L.HW_ % 16 == 0 && L.FM % 2 == 0 &&
                      (!G::HUP || ((L.WM / L.HW_) % 2 == 0 && L.HR % 2 == 0)),
                  "halo conv tile");
    constexpr int HB_INS = BN / L.RPP, H_PW = (L.H_INS + L.NW - 1) / L.NW, BH_PW = (HB_INS + L.NW - 1) / L.NW;
    constexpr int A2_INS = BM / L.RPP, A2_PW = (A2_INS + L.NW - 1) / L.NW;
    const int h_cnt = L.H_INS / L.NW + (wave < L.H_INS % L.NW ? 1 : 0);
    const int b_cnt = HB_INS / L.NW + (wave < HB_INS % L.NW ? 1 : 0);
    const int a2_cnt = p.A2 ? A2_INS / L.NW + (wave < A2_INS % L.NW ? 1 : 0) : 0;
    const int pix = (G::HUP ? 2 * p.H : p.H) * L.HW_;  // output pixels per image
    const int bimg = m0 / pix, oh0 = (m0 - bimg * pix) / L.HW_;
    // B / A2 pieces j > 0 sit whole 128-row rounds below piece 0 (same swizzle): their offsets go to the scalar
    // offset (j x bstep / a2step), one VGPR per operand instead of one per piece -- the 256x320 tile has none spare
    unsigned hvo[H_PW], bvo0, a2vo0;
    const unsigned bstep = (unsigned)(L.NW * L.RPP * p.ldw * 2), a2step = (unsigned)(L.NW * L.RPP * p.lda2 * 2);
#pragma unroll
    for (int j = 0; j < H_PW; ++j) {
      const int row = (j * L.NW + wave) * L.RPP + lane / L.CPRW;
      const int r = row / L.HP, c = row - r * L.HP;
      const int ih = (G::HUP ? oh0 / 2 : oh0) - 1 + r, iw = c - 1;
      const bool ok = j * L.NW + wave < L.H_INS && ih >= 0 && ih < p.H && iw >= 0 && iw < L.HWIN;
      hvo[j] = ok ? (unsigned)(((long)(bimg * p.H + ih) * L.HWIN + iw) * p.lda * 2) + (unsigned)(((lane % L.CPRW) ^ G::swzk(row)) << 4)
                  : OOB;
    }
    static_assert(L.NW * L.RPP % 8 == 0, "a piece round keeps the row swizzle");
    {  // (N is a multiple of 320 and M of BM on the halo path: every issued piece is in range)
      const int row = wave * L.RPP + lane / L.CPRW;
      bvo0 = (unsigned)((long)(n0 + row) * p.ldw * 2) + (unsigned)(((lane % L.CPRW) ^ G::swzk(row)) << 4);
      a2vo0 = p.A2 ? (unsigned)((long)(m0 + row) * p.lda2 * 2) + (unsigned)(((lane % L.CPRW) ^ G::swzk(row)) << 4) : OOB;
    }
    char* const hbase = smem;
    char* const bbase = smem + 2 * L.HBYTES;
    // this split's main slices [c_first, c_first + nsl) and shortcut steps [k2_first, k2_first + n2)
    const int nsl_all = p.Cin / 32, n2_all = p.A2 ? (p.K - 9 * p.Cin) / 32 : 0;
    const int c_first = min(nsl_all, split * p.kchunk), nsl = min(nsl_all, c_first + p.kchunk) - c_first;
    const int k2_first = min(n2_all, split * p.kchunk2), n2 = min(n2_all, k2_first + p.kchunk2) - k2_first;
    const int nkl = 9 * nsl + n2;
    auto issue_halo = [&](int c32, int hb) {  // input channels 32 c32 .. +31 of the halo, into buffer hb
#pragma unroll
      for (int j = 0; j < H_PW; ++j)  // (whole rounds of pieces need no per-wave test)
        if ((j + 1) * L.NW <= L.H_INS || j * L.NW + wave < L.H_INS)
          bld16(rsA, hbase + hb * L.HBYTES + (j * L.NW + wave) * 1024, hvo[j], (unsigned)(c32 * 64));
    };
    // B tiles: a 4-slot ring (slot ks % 4), issued three local K-steps ahead; A2 tiles (folded shortcut): three slots
    // in the halo buffers (slot ks % 3), issued two steps ahead, ahead of the B tile issued at the same point
    auto issue_b_kb = [&](int ks, unsigned kb) {
#pragma unroll
      for (int j = 0; j < BH_PW; ++j)
        if ((j + 1) * L.NW <= HB_INS || j * L.NW + wave < HB_INS)
          bld16(rsW, bbase + (ks & 3) * L.BSTAGE + (j * L.NW + wave) * 1024, bvo0, kb + j * bstep);
    };
    // W columns of main slice c32 (global 32-channel slice) at tap: ((c32 / 2) * 9 + tap) * 64 + (c32 % 2) * 32; of
    // shortcut step k2 (local): 9 Cin + 32 (k2_first + k2)
    auto kb_main = [&](int c32, int tap) { return (unsigned)(((c32 >> 1) * 9 + tap) * 128 + (c32 & 1) * 64); };
    auto kb_sc = [&](int k2) { return (unsigned)(18 * p.Cin + 64 * (k2_first + k2)); };
    auto a2_slot = [&](int ks) -> char* {
      const int slot = ks % 3;
      return hbase + ((nsl + (slot == 2 ? 1 : 0)) & 1) * L.HBYTES + (slot == 1 ? L.A2BYTES : 0);
    };
    auto issue_a2 = [&](int ks) {
      char* const a2s = a2_slot(ks);
      const int k2 = k2_first + ks - 9 * nsl;
#pragma unroll
      for (int j = 0; j < A2_PW; ++j)
        if ((j + 1) * L.NW <= A2_INS || j * L.NW + wave < A2_INS)
          bld16(rsA2, a2s + (j * L.NW + wave) * 1024, a2vo0, (unsigned)(64 * k2) + j * a2step);
    };
    // per-lane LDS byte offsets: A row fr of a halo fragment at tap column kw (swizzle of row fr + kw: the fragment's
    // first halo row is a multiple of 8), row fr of an aligned B / A2 fragment
    unsigned aoff[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {  // upsample: lane fr reads input column offset (fr + kw + 1) >> 1
      const int rr = G::HUP ? (fr + kw + 1) >> 1 : fr + kw;
      aoff[kw] = (unsigned)((G::HUP ? rr : fr) * L.RB + ((fg ^ G::swzk(rr)) << 4));
    }
    const unsigned boff = (unsigned)(fr * L.RB + ((fg ^ G::swzk(fr)) << 4));
    const int orow_w = (wr * L.WM) / L.HW_;  // the wave's first output row within the tile
    // GroupNorm(+SiLU) of the main input (sdmoe_conv3x3_gn): this image's per-channel scale / shift go to LDS first;
    // every staged halo slice is then normalised in place -- slice c + 1 at tap 5 of slice c (its pieces are older
    // than that step's group, so landed; nobody reads its buffer before slice c + 1), the first one before its taps.
    // Thread tid always holds 16-B chunk position tid % 4 of halo rows tid / 4 + 128 k, i.e. data chunk
    // (tid % 4) ^ swzk(row) = (tid % 4) ^ ((tid >> 3) & 3): eight fixed channels. Out-of-image pixels stay zero (the
    // conv pads the NORMALISED tensor). Same arithmetic as gn_apply_kernel: the conv input is bit-identical.
    const bool gn = !G::HUP && p.gn_scale != nullptr;
    float* const gsc = reinterpret_cast<float*>(smem + L.RING);
    float* const gsh = gsc + GN_MAXC;
    if constexpr (!G::HUP) {
      if (gn) {
        for (int i = tid; i < p.Cin; i += L.NT) {
          gsc[i] = p.gn_scale[(long)bimg * p.Cin + i];
          gsh[i] = p.gn_shift[(long)bimg * p.Cin + i];
        }
        __syncthreads();
      }
    }
    auto transform = [&](int c32, int hb) {
      if constexpr (!G::HUP) {
        static_assert(L.NT == 512 && L.RB == 64, "transform mapping: 128 halo rows of 4 chunks per pass");
        const int q = tid & 3, ch0 = c32 * 32 + ((q ^ ((tid >> 3) & 3)) << 3);
        const float4v s0 = *reinterpret_cast<const float4v*>(gsc + ch0), s1 = *reinterpret_cast<const float4v*>(gsc + ch0 + 4);
        const float4v h0 = *reinterpret_cast<const float4v*>(gsh + ch0), h1 = *reinterpret_cast<const float4v*>(gsh + ch0 + 4);
        const float sc[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
        const float sh[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        char* const buf = hbase + hb * L.HBYTES + q * 16;
#pragma unroll
        for (int k = 0; k < (L.HROWS_IN * L.HP + 127) / 128; ++k) {
          const int row = (tid >> 2) + 128 * k;
          const int r = row / L.HP, c = row - r * L.HP;
          const int ih = oh0 - 1 + r, iw = c - 1;
          if (row < L.HROWS_IN * L.HP && ih >= 0 && ih < p.H && iw >= 0 && iw < L.HW_) {
            half8 v = *reinterpret_cast<const half8*>(buf + row * L.RB);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              float f = (float)v[j] * sc[j] + sh[j];
              if (p.gn_silu) f = silu_f(f);
              v[j] = (half_t)f;
            }
            *reinterpret_cast<half8*>(buf + row * L.RB) = v;
          }
        }
      }
    };
    // Issue points: j = -3, -2, -1 in the prologue, j = s after step s's barrier; point j issues A2(j + 2) (a shortcut
    // step), then B(j + 3), then -- at tap 0 of a slice with a successor -- that successor's halo. Step s's B fragments
    // and first A pair are read AHEAD, at the end of step s - 1 (so step s's MFMAs start right behind its barrier instead
    // of behind a burst of LDS reads): the barrier at the start of step s therefore waits for B(s + 1) (and with it
    // every older piece: A2(s), the halos), issued at point s - 2. Main-slice steps keep the tap compile-time.
    auto is_sc = [&](int ks) { return ks >= 9 * nsl && ks < nkl; };
    auto issue_b_any = [&](int ks) {  // (prologue / shortcut steps: runtime tap)
      if (ks < 9 * nsl) issue_b_kb(ks, kb_main(c_first + ks / 9, ks % 9));
      else issue_b_kb(ks, kb_sc(ks - 9 * nsl));
    };
    half8 bcur[L.FN], a0, a1;
    auto read_b = [&](int ks) {  // B fragments of step ks (slot ks % 4)
      const char* sb = bbase + (ks & 3) * L.BSTAGE + wc * L.WN * L.RB;
#pragma unroll
      for (int j = 0; j < L.FN; ++j) bcur[j] = *reinterpret_cast<const half8*>(sb + boff + 16 * j * L.RB);
    };
    auto a_frag = [&](const char* hbuf, auto tc, int i) -> half8 {  // A fragment i at compile-time tap, halo buffer hbuf
      constexpr int t = decltype(tc)::value, kh = t / 3, kw = t % 3;
      const int i16 = 16 * i;
      if constexpr (G::HUP)  // input row ((orow + kh - 1) >> 1) - (oh0 / 2 - 1), column (ocol0 / 2) + lane part
        return *reinterpret_cast<const half8*>(hbuf + aoff[kw] + (((((i16 / L.HW_) + kh - 1) >> 1) + 1) * L.HP + (i16 % L.HW_) / 2) * L.RB);
      else
        return *reinterpret_cast<const half8*>(hbuf + aoff[kw] + ((i16 / L.HW_ + kh) * L.HP + (i16 % L.HW_) + kw) * L.RB);
    };
    const int hrow = (G::HUP ? orow_w / 2 : orow_w) * L.HP * L.RB;  // the wave's first halo row
    // the step's MFMAs on bcur / a0 a1 (already in registers); the rest of the A pairs read one group ahead; mid()
    // (the step's DMA issue) after the first group, so both waves of a SIMD have matrix work queued while it issues
    auto mfma_groups = [&](auto&& a_at, auto&& mid) {
#pragma unroll
      for (int g = 0; g < L.FM / 2; ++g) {
        half8 n0 = a0, n1 = a1;
        if (g + 1 < L.FM / 2) {
          n0 = a_at(2 * g + 2);
          n1 = a_at(2 * g + 3);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < L.FN; ++j) acc[2 * g][j] = mfma16x16x32(bcur[j], a0, acc[2 * g][j]);
#pragma unroll
        for (int j = 0; j < L.FN; ++j) acc[2 * g + 1][j] = mfma16x16x32(bcur[j], a1, acc[2 * g + 1][j]);
        __builtin_amdgcn_sched_barrier(0);
        if (g == 0) {
          asm volatile("" ::: "memory");
          mid();
          __builtin_amdgcn_sched_barrier(0);
        }
        a0 = n0;
        a1 = n1;
      }
    };
    // Every main slice but the last has a successor (MORE), so its taps' waits are compile-time counts; the last slice
    // and the shortcut steps count at run time. (The diagnostics knob stays a run-time test: a copy of the loop with it
    // compile-time off pushed the 256x320 tiles to 256 VGPRs + 188 B of scratch.) The compile-time waits
    // use the smallest per-wave piece counts (b_lo, h_lo): a wave holding one more piece waits for that piece too --
    // issued a full K-step earlier -- instead of walking a compare-and-branch chain for its exact count every step.
    constexpr int b_lo = HB_INS / L.NW, h_lo = L.H_INS / L.NW;
    auto main_loop = [&]() {
      const int diag = p.diag;
      if (nkl > 0) {
        if (nsl > 0) issue_halo(c_first, 0);
        if (!(diag & 1)) {  // points -3, -2, -1: B(0); A2(0), B(1); A2(1), B(2)
          issue_b_any(0);
          if (is_sc(0)) issue_a2(0);
          if (nkl > 1) issue_b_any(1);
          if (is_sc(1)) issue_a2(1);
          if (nkl > 2) issue_b_any(2);
        }
        // younger than B(0): A2(0), B(1), A2(1), B(2)
        const int w0 = (is_sc(0) ? a2_cnt : 0) + (nkl > 1 ? b_cnt : 0) + (is_sc(1) ? a2_cnt : 0) + (nkl > 2 ? b_cnt : 0);
        if (gn && nsl > 0) {  // the first slice's halo (the oldest load) landed, visible to all, normalised
          vm_wait(w0 + b_cnt);
          __syncthreads();
          transform(c_first, 0);
        }
        vm_wait(w0);
        __syncthreads();
        read_b(0);
        if (nsl > 0) {
          a0 = a_frag(hbase + hrow, std::integral_constant<int, 0>(), 0);
          a1 = a_frag(hbase + hrow, std::integral_constant<int, 0>(), 1);
        }
      }
      auto slice = [&](int cs, auto more_tag) {
        constexpr bool MORE = decltype(more_tag)::value;
        const char* const hcur = hbase + (cs & 1) * L.HBYTES + hrow;
        const char* const hnxt = hbase + ((cs & 1) ^ 1) * L.HBYTES + hrow;
        const int c32 = c_first + cs;
        auto tap_step = [&](auto tc) {
          constexpr int t = decltype(tc)::value;
          const int ks = cs * 9 + t;
          // younger than B(ks + 1): the halo issued at point ks - 2 (t == 2) and ks - 1 (t == 1), A2(ks + 1) (the
          // first shortcut step, t == 8 of the last slice), B(ks + 2)
          if constexpr (MORE) {
            vm_wait(b_lo + ((t == 1 || t == 2) ? h_lo : 0));
          } else if constexpr (t <= 6) {  // last slice: B(ks + 2) is a main-slice tile up to tap 6, nothing else younger
            vm_wait(b_lo);
          } else {
            int nwait = ks + 2 < nkl ? b_cnt : 0;
            if (t == 8 && n2 > 0) nwait += a2_cnt;
            vm_wait(ks + 1 < nkl ? nwait : 0);
          }
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
          if constexpr (MORE && t == 5) {
            if (gn) transform(c32 + 1, (cs & 1) ^ 1);
          }
          auto mid = [&]() {
            if (diag & 1) return;
            if constexpr (!MORE) {
              if (t >= 7 && n2 > t - 7) issue_a2(ks + 2);  // A2 of shortcut step t - 7
            }
            if constexpr (t + 3 < 9) {
              issue_b_kb(ks + 3, kb_main(c32, t + 3));
            } else if constexpr (MORE) {
              issue_b_kb(ks + 3, kb_main(c32 + 1, t - 6));
            } else {
              if (n2 > t - 6) issue_b_kb(ks + 3, kb_sc(t - 6));
            }
            if constexpr (MORE && t == 0) issue_halo(c32 + 1, (cs & 1) ^ 1);
          };
          if (!(diag & 2)) mfma_groups([&](int i) -> half8 { return a_frag(hcur, tc, i); }, mid);
          else mid();
          // read-ahead of step ks + 1: tap t + 1, or tap 0 of the next slice, or (B only) the first shortcut step
          if constexpr (t < 8) {
            read_b(ks + 1);
            a0 = a_frag(hcur, std::integral_constant<int, t + 1>(), 0);
            a1 = a_frag(hcur, std::integral_constant<int, t + 1>(), 1);
          } else if constexpr (MORE) {
            read_b(ks + 1);
            a0 = a_frag(hnxt, std::integral_constant<int, 0>(), 0);
            a1 = a_frag(hnxt, std::integral_constant<int, 0>(), 1);
          } else {
            if (ks + 1 < nkl) read_b(ks + 1);
          }
        };
        tap_step(std::integral_constant<int, 0>());
        tap_step(std::integral_constant<int, 1>());
        tap_step(std::integral_constant<int, 2>());
        tap_step(std::integral_constant<int, 3>());
        tap_step(std::integral_constant<int, 4>());
        tap_step(std::integral_constant<int, 5>());
        tap_step(std::integral_constant<int, 6>());
        tap_step(std::integral_constant<int, 7>());
        tap_step(std::integral_constant<int, 8>());
      };
      for (int cs = 0; cs + 1 < nsl; ++cs) slice(cs, std::true_type());
      if (nsl > 0) slice(nsl - 1, std::false_type());
      for (int k2l = 0; k2l < n2; ++k2l) {  // folded shortcut K-steps: B read ahead, the A2 pair right behind the barrier
        const int ks = 9 * nsl + k2l;
        // younger than B(ks + 1): A2(ks + 1), B(ks + 2) -- compile-time counts but for the last two steps
        if (ks + 2 < nkl) vm_wait(A2_INS / L.NW + b_lo);
        else vm_wait(ks + 1 < nkl ? (is_sc(ks + 1) ? a2_cnt : 0) + (ks + 2 < nkl ? b_cnt : 0) : 0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        auto mid = [&]() {
          if (diag & 1) return;
          if (is_sc(ks + 2)) issue_a2(ks + 2);
          if (ks + 3 < nkl) issue_b_kb(ks + 3, kb_sc(k2l + 3));
        };
        const char* a2s = a2_slot(ks) + wr * L.WM * L.RB;
        auto a2_at = [&](int i) -> half8 { return *reinterpret_cast<const half8*>(a2s + boff + 16 * i * L.RB); };
        if (!(diag & 2)) {
          a0 = a2_at(0);
          a1 = a2_at(1);
          mfma_groups(a2_at, mid);
        } else {
          mid();
        }
        if (ks + 1 < nkl) read_b(ks + 1);
      }
    };
    main_loop();
  } else {
    // prologue: stages 0 .. NSTAGE-2
#pragma unroll
    for (int s = 0; s < NSTAGE - 1; ++s)
      if (s < nk) issue_stage(ks0 + s, s);

    for (int it = 0; it < nk; ++it) {
      // wait for this K-step's tile (leave the later ones in flight), then make every wave's DMA visible
      {
        const int ahead = min(NSTAGE - 2, nk - 1 - it);  // stages issued after this one (wave-uniform)
        if (NSTAGE >= 4 && ahead >= 2) {
          if (NSTAGE >= 5 && ahead >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * L.PER_WAVE) : "memory");
          else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * L.PER_WAVE) : "memory");
        } else if (NSTAGE >= 3 && ahead >= 1) {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L.PER_WAVE) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      }
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // the next stage's LDS-DMA (into the slot read in step it - 1, which every wave finished before the barrier).
      // 3-stage rings: issued after this step's first fragment reads, so its ~60 issue cycles per piece overlap their
      // LDS latency instead of delaying the first MFMA behind the barrier. 2-stage rings keep it right behind the
      // barrier: their stage has one K-step to land, and the later issue measured 2-5 % slower there (routed GEGLU,
      // 128x160 convs, K = 5120 projections; r05f)
      auto issue_next = [&]() {
        if (it + NSTAGE - 1 < nk && !(p.diag & 1)) issue_stage(ks0 + it + NSTAGE - 1, (it + NSTAGE - 1) % NSTAGE);
        else if (L.TAB_PREFETCH && it == nk - 1) issue_gelu_tab(smem + (nk % NSTAGE) * L.STAGE + L.STAGE - TAB_BYTES);
      };
      constexpr bool PIPE = !(G::KEEP && L.FN > 5);
      constexpr bool LATE_DMA = PIPE && NSTAGE >= 3;
      if (!LATE_DMA || (p.diag & 2)) issue_next();

      const char* sa = smem + (it % NSTAGE) * L.STAGE;
      const char* sbm = sa + BM * BK * 2;
      if (p.diag & 2) continue;
      // fragment reads (A masked by MoE keep bits, B by Wanda bits where the mode says so)
      // MODE_KEEP on the software-pipelined tiles: every A fragment's lane mask of the K-step looked up up front, right
      // behind the barrier (one ds_read_b64 of a fragment row's 8 keep bytes, then one ds_read_b128 per fragment), so the
      // fragment reads of the loop carry no dependent keep-byte -> table chain (it was exposed behind the 10-MFMA groups
      // of the 64x160 / 128x160 tiles: keep-masked 16x16-level down projection 49.9 vs 32.5 us plain, loads and epilogue
      // off)
      constexpr bool KPRE = MODE == MODE_KEEP && !(G::KEEP && L.FN > 5) && BK == 64 && L.FM <= 4;  // (FM = 8: +64 VGPRs, spills)
      uint4v kmask[KPRE ? 2 : 1][KPRE ? L.FM : 1];
      if constexpr (KPRE) {
#pragma unroll
        for (int i = 0; i < L.FM; ++i) {
          const uint2v kq = *reinterpret_cast<const uint2v*>(sa + L.KEEP_OFF + (wr * L.WM + i * 16 + fr) * 8);
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
            kmask[kk][i] = *reinterpret_cast<const uint4v*>(smem + L.LUT_OFF + ((kq[kk] >> (8 * fg)) & 255u) * 16);
        }
      }
      auto read_a = [&](int kk, int i) -> half8 {
        const int row = wr * L.WM + i * 16 + fr;
        half8 a = *reinterpret_cast<const half8*>(sa + row * L.RB + (((kk * 4 + fg) ^ G::swzk(row)) << 4));
        if constexpr (KPRE) {
          uint4v u = __builtin_bit_cast(uint4v, a);
          const uint4v mk = kmask[kk][i];
          u[0] &= mk[0]; u[1] &= mk[1]; u[2] &= mk[2]; u[3] &= mk[3];
          a = __builtin_bit_cast(half8, u);
        } else if constexpr (G::AKEEP) {  // zero the neurons of this row's dropped experts (8 neurons = chunk kk*4+fg)
          const unsigned kbyte = *reinterpret_cast<const unsigned char*>(sa + L.KEEP_OFF + row * 8 + kk * 4 + fg);
          uint4v u = __builtin_bit_cast(uint4v, a);
          if constexpr (MODE == MODE_KEEP) {  // byte table: one ds_read_b128 behind the keep byte
            const uint4v mk = *reinterpret_cast<const uint4v*>(smem + L.LUT_OFF + kbyte * 16);
            u[0] &= mk[0]; u[1] &= mk[1]; u[2] &= mk[2]; u[3] &= mk[3];
          } else {  // KEEPW: the nibble table (its wider reads cost the 128x160 tile its second workgroup per CU)
            const uint2v lo = *reinterpret_cast<const uint2v*>(smem + L.LUT_OFF + (kbyte & 15u) * 8);
            const uint2v hi = *reinterpret_cast<const uint2v*>(smem + L.LUT_OFF + (kbyte >> 4) * 8);
            u[0] &= lo[0]; u[1] &= lo[1]; u[2] &= hi[0]; u[3] &= hi[1];
          }
          a = __builtin_bit_cast(half8, u);
        }
        return a;
      };
      auto read_b = [&](int kk, int j) -> half8 {
        const int row = wc * L.WN + j * 16 + fr;
        half8 b = *reinterpret_cast<const half8*>(sbm + row * L.RB + (((kk * 4 + fg) ^ G::swzk(row)) << 4));
        if constexpr (G::WKEEP) {  // zero this W row's Wanda-masked weights (8 k = chunk kk*4+fg); mask bit SET = removed
          const unsigned mbyte = ~*reinterpret_cast<const unsigned char*>(sa + L.WKEEP_OFF + row * 8 + kk * 4 + fg);
          const uint2v lo = *reinterpret_cast<const uint2v*>(smem + L.LUT_OFF + (mbyte & 15u) * 8);
          const uint2v hi = *reinterpret_cast<const uint2v*>(smem + L.LUT_OFF + ((mbyte >> 4) & 15u) * 8);
          uint4v u = __builtin_bit_cast(uint4v, b);
          u[0] &= lo[0]; u[1] &= lo[1]; u[2] &= hi[0]; u[3] &= hi[1];
          b = __builtin_bit_cast(half8, u);
        }
        return b;
      };
      if constexpr (PIPE) {  // (wide masked tiles: no registers to spare)
        // software-pipelined: A fragments in pairs, the next pair's LDS reads issued before the current pair's
        // 2*FN MFMAs (one group of latency cover); the next kk's B fragments read during the last group when they
        // fit a second register set. sched_barrier pins the read / MFMA order so hipcc cannot sink the reads to
        // their first use (which exposes the LDS latency every group).
        constexpr int NKK = BK / 32, NG = L.FM / 2;
        static_assert(L.FM % 2 == 0, "the pipelined loop reads fragment rows in pairs");
        constexpr bool BDB = L.FN <= 5 && !G::KEEP;  // second B set: +4*FN VGPRs (the masked modes need those registers)
        half8 bcur[L.FN], bnxt[L.FN];
#pragma unroll
        for (int j = 0; j < L.FN; ++j) bcur[j] = read_b(0, j);
        half8 a0 = read_a(0, 0), a1 = read_a(0, 1);
        if constexpr (LATE_DMA) {
          __builtin_amdgcn_sched_barrier(0);
          asm volatile("" ::: "memory");
          issue_next();
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            half8 n0 = a0, n1 = a1;
            if (g + 1 < NG) {
              n0 = read_a(kk, 2 * g + 2);
              n1 = read_a(kk, 2 * g + 3);
            } else if (kk + 1 < NKK) {
              if constexpr (BDB) {
#pragma unroll
                for (int j = 0; j < L.FN; ++j) bnxt[j] = read_b(kk + 1, j);
              }
              n0 = read_a(kk + 1, 0);
              n1 = read_a(kk + 1, 1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < L.FN; ++j)
              acc[2 * g][j] = mfma16x16x32(bcur[j], a0, acc[2 * g][j]);
#pragma unroll
            for (int j = 0; j < L.FN; ++j)
              acc[2 * g + 1][j] = mfma16x16x32(bcur[j], a1, acc[2 * g + 1][j]);
            __builtin_amdgcn_sched_barrier(0);
            a0 = n0;
            a1 = n1;
          }
          if (kk + 1 < NKK) {
#pragma unroll
            for (int j = 0; j < L.FN; ++j) bcur[j] = BDB ? bnxt[j] : read_b(kk + 1, j);
          }
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
          half8 af[L.FM], bf[L.FN];
#pragma unroll
          for (int i = 0; i < L.FM; ++i) af[i] = read_a(kk, i);
#pragma unroll
          for (int j = 0; j < L.FN; ++j) bf[j] = read_b(kk, j);
#pragma unroll
          for (int i = 0; i < L.FM; ++i)
#pragma unroll
            for (int j = 0; j < L.FN; ++j)
              acc[i][j] = mfma16x16x32(bf[j], af[i], acc[i][j]);
        }
      }
      if constexpr (G::LN) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 one2 = {(half_t)1.f, (half_t)1.f};
#pragma unroll
        for (int t = 0; t < L.LN_IPL; ++t) {
          const int row = tid / 8 + (L.NT / 8) * t, ch = tid & 7;
          const half8 x = *reinterpret_cast<const half8*>(sa + row * L.RB + ((ch ^ G::swzk(row)) << 4));
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const h2 x2 = {x[2 * q], x[2 * q + 1]};
            ln_s1[t] = __builtin_amdgcn_fdot2(x2, one2, ln_s1[t], false);
            ln_s2[t] = __builtin_amdgcn_fdot2(x2, x2, ln_s2[t], false);
          }
        }
      }
    }
  }

  // ---- epilogue
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (p.diag & 4) {  // diagnostics: keep the accumulators live, store nothing
#pragma unroll
    for (int i = 0; i < L.FM; ++i)
#pragma unroll
      for (int j = 0; j < L.FN; ++j) asm volatile("" ::"v"(acc[i][j]));
    return;
  }
  const int mw = m0 + wr * L.WM, nw = n0 + wc * L.WN;  // this wave's output tile origin
  if (p.part) {  // split-K: fp32 partial slab [split][M][N], 16-B stores straight from the accumulators
#pragma unroll
    for (int i = 0; i < L.FM; ++i)
#pragma unroll
      for (int j = 0; j < L.FN; ++j) {
        const int m = mw + 16 * i + fr, n = nw + 16 * j + 4 * fg;
        if (m < p.M && n < p.N) *reinterpret_cast<float4v*>(p.part + ((long)split * p.M + m) * p.N + n) = acc[i][j];
      }
    return;
  }
  float* ln_row = reinterpret_cast<float*>(smem + L.LN_ROW_OFF);  // [BM][2]: rstd, -mean * rstd
  float* ln_col = reinterpret_cast<float*>(smem + L.LN_COL_OFF);  // [BN] wsum, then [BN] ln_bias
  if constexpr (G::LN) {
#pragma unroll
    for (int t = 0; t < L.LN_IPL; ++t) {
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        ln_s1[t] += __shfl_xor(ln_s1[t], o, 64);
        ln_s2[t] += __shfl_xor(ln_s2[t], o, 64);
      }
      if ((tid & 7) == 0) {
        const int row = tid / 8 + (L.NT / 8) * t;
        const float mean = ln_s1[t] / (float)p.K;
        const float var = fmaxf(ln_s2[t] / (float)p.K - mean * mean, 0.f);
        const float rstd = rsqrtf(var + p.ln_eps);
        ln_row[2 * row] = rstd;
        ln_row[2 * row + 1] = -mean * rstd;
      }
    }
    for (int c = tid; c < BN; c += L.NT) {
      const bool ok = n0 + c < p.N;
      ln_col[c] = ok ? p.ln_wsum[n0 + c] : 0.f;
      ln_col[BN + c] = ok ? p.ln_bias[n0 + c] : 0.f;
    }
  }
  __syncthreads();
  constexpr int CPR = L.WN / 8;
  if (!G::GEGLU && p.act == ACT_NONE && (!p.R || p.res16 != 0)) {
    // fp16 path: bias and per-image column add in registers on each lane's 4-column row piece (one rounding, as
    // epilogue8), staged as fp16 (one ds_write_b64 per fragment: 1/2.5 of the LDS time of staging fp32 with 4
    // ds_write_b32), then copied out in 16-B row chunks: 175 -> 166 us for the M = 65536, N = 2560, K = 320 linear,
    // 1-3 % on the convs. Measured slower and therefore not used: residual loads in registers (8-B pieces of 16
    // rows: 29 -> 33 us for linear+res at 64x64) and the GEGLU epilogue on fp16 staging (170 -> 179 us); an
    // activation's code keeps the unrolled fragment loop from unrolling (acc then lives in scratch).
    half4 b4[L.FN];
    // MODE_CONV_UP2X: GEMM column n = phase * Cout + channel -> bias and output column n - ncol0, output row by the map
    const int ncol0 = G::UP2X ? up_ph * (p.N >> 2) : 0;
    auto c_at = [&](int m, int n) -> half_t* {
      if constexpr (G::UP2X) return p.C + up2x_out_row(m, p.H, p.Wd, up_ph) * p.ldc + (n - ncol0);
      else return p.C + (long)m * p.ldc + n;
    };
#pragma unroll
    for (int j = 0; j < L.FN; ++j) {
      const int n = nw + 16 * j + 4 * fg;
      b4[j] = (!G::LN && p.bias && n < p.N) ? *reinterpret_cast<const half4*>(p.bias + (n - ncol0)) : (half4){0, 0, 0, 0};
    }
    if (!G::WKEEP && p.epi_direct) {  // (the Wanda-masked tiles: no registers to spare for it)
      // Direct fp16 stores, no LDS staging (sdmoe_tune knob 23): per fragment row and pair of fragments (j, j + 1)
      // two v_permlane16_swap per lane leave each lane 8 consecutive output columns of its row -- lane group g:
      // fragment j + (g & 1), columns 8 (g >> 1) .. +7 -- stored as one 16-B piece (the T21 widening on the 16x16
      // fragment layout); an unpaired last fragment stores 8 B per lane. Residual: loaded in the same layout and added
      // to the fp16-rounded output in fp16 arithmetic, as the staged path.
      const bool res = p.R != nullptr;
#pragma unroll
      for (int i = 0; i < L.FM; ++i) {
        __builtin_amdgcn_sched_barrier(0);
        const int m = mw + 16 * i + fr;
        const half_t* cap = (p.coladd && m < p.M) ? p.coladd + (long)(m / p.rows_per_batch) * p.coladd_bstride : nullptr;
        const float* cfp = (p.colf && m < p.M) ? p.colf + (long)(m / p.rows_per_batch) * p.colf_bstride : nullptr;
        float a = 0.f, c = 0.f;
        if constexpr (G::LN) {
          const int rl = wr * L.WM + 16 * i + fr;
          a = ln_row[2 * rl];
          c = ln_row[2 * rl + 1];
        }
        auto frag16 = [&](int j) -> uint2v {  // fragment j of row block i: + bias / column adds (/ LN), rounded
          const int n = nw + 16 * j + 4 * fg;
          float4v v = acc[i][j];
          if constexpr (G::LN) {
            const int cl = wc * L.WN + 16 * j + 4 * fg;
            const float4v ws = *reinterpret_cast<const float4v*>(ln_col + cl);
            const float4v lb = *reinterpret_cast<const float4v*>(ln_col + BN + cl);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(a, v[r], __builtin_fmaf(c, ws[r], lb[r]));
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)b4[j][r];
          if (cap && n < p.N) {
            const half4 cc = *reinterpret_cast<const half4*>(cap + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += (float)cc[r];
          }
          if (cfp && n < p.N) {
            const float4v cc = *reinterpret_cast<const float4v*>(cfp + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += cc[r];
          }
          half4 y;
#pragma unroll
          for (int r = 0; r < 4; ++r) y[r] = (half_t)v[r];
          return __builtin_bit_cast(uint2v, y);
        };
#pragma unroll
        for (int j = 0; j + 1 < L.FN; j += 2) {
          const uint2v ya = frag16(j), yb = frag16(j + 1);
          const auto s0 = __builtin_amdgcn_permlane16_swap(ya[0], yb[0], false, false);
          const auto s1 = __builtin_amdgcn_permlane16_swap(ya[1], yb[1], false, false);
          const int n = nw + 16 * (j + (fg & 1)) + 8 * (fg >> 1);
          half8 o = __builtin_bit_cast(half8, (uint4v){s0[0], s1[0], s0[1], s1[1]});
          if (m < p.M && n < p.N) {
            if (res) {
              const half8 rr = *reinterpret_cast<const half8*>(p.R + (long)m * p.ldr + n);
#pragma unroll
              for (int r = 0; r < 8; ++r) o[r] = (half_t)((float)o[r] + (float)rr[r]);
            }
            if (p.diag & 8) asm volatile("" ::"v"(o));
            else *reinterpret_cast<half8*>(c_at(m, n)) = o;
          }
        }
        if constexpr (L.FN % 2) {
          const int n = nw + 16 * (L.FN - 1) + 4 * fg;
          half4 o = __builtin_bit_cast(half4, frag16(L.FN - 1));
          if (m < p.M && n < p.N) {
            if (res) {
              const half4 rr = *reinterpret_cast<const half4*>(p.R + (long)m * p.ldr + n);
#pragma unroll
              for (int r = 0; r < 4; ++r) o[r] = (half_t)((float)o[r] + (float)rr[r]);
            }
            if (p.diag & 8) asm volatile("" ::"v"(o));
            else *reinterpret_cast<half4*>(c_at(m, n)) = o;
          }
        }
      }
      return;
    }
    half_t* st = reinterpret_cast<half_t*>(smem) + wave * (L.WM / L.NPASS16) * L.RS16;
    // residual (fp16, 16-B row chunks): this pass's chunks are loaded before its accumulators are staged, so their
    // latency hides behind the staging; added to the staged fp16 output in the copy-out (the output is rounded to
    // fp16 and the residual added in fp16 arithmetic -- diffusers' fp16 `to_out(x) + hidden_states`)
    constexpr int NCH16 = (L.WM / L.NPASS16) * CPR, NIT16 = (NCH16 + 63) / 64;
    const bool res = p.R != nullptr;
#pragma unroll
    for (int h = 0; h < L.NPASS16; ++h) {
      half8 rr[NIT16];
      if (res) {
#pragma unroll
        for (int it = 0; it < NIT16; ++it) {
          const int id = lane + 64 * it;
          const int r = id / CPR, c8 = id - r * CPR;
          const int m = mw + h * (L.WM / L.NPASS16) + r, n = nw + c8 * 8;
          rr[it] = (id < NCH16 && m < p.M && n < p.N) ? *reinterpret_cast<const half8*>(p.R + (long)m * p.ldr + n)
                                                      : (half8){0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
#pragma unroll
      for (int i = 0; i < L.FM / L.NPASS16; ++i) {
        // one fragment row at a time: keeps the hoisted bias / column-add / residual loads to FN pieces (the 8-wave
        // 256x320 tiles hold 160 accumulator VGPRs here and spilled when the compiler hoisted all of them)
        __builtin_amdgcn_sched_barrier(0);
        const int m = mw + 16 * (h * (L.FM / L.NPASS16) + i) + fr;
        const half_t* cap = (p.coladd && m < p.M) ? p.coladd + (long)(m / p.rows_per_batch) * p.coladd_bstride : nullptr;
        const float* cfp = (p.colf && m < p.M) ? p.colf + (long)(m / p.rows_per_batch) * p.colf_bstride : nullptr;
        float a = 0.f, c = 0.f;  // LN: this lane's row (rstd, -mean * rstd), read once per fragment row
        if constexpr (G::LN) {
          const int rl = wr * L.WM + 16 * (h * (L.FM / L.NPASS16) + i) + fr;
          a = ln_row[2 * rl];
          c = ln_row[2 * rl + 1];
        }
#pragma unroll
        for (int j = 0; j < L.FN; ++j) {
          const int n = nw + 16 * j + 4 * fg;
          float4v v = acc[h * (L.FM / L.NPASS16) + i][j];
          if constexpr (G::LN) {  // rstd * (acc - mean * wsum) + ln_bias
            const int cl = wc * L.WN + 16 * j + 4 * fg;
            const float4v ws = *reinterpret_cast<const float4v*>(ln_col + cl);
            const float4v lb = *reinterpret_cast<const float4v*>(ln_col + BN + cl);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(a, v[r], __builtin_fmaf(c, ws[r], lb[r]));
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)b4[j][r];
          if (cap && n < p.N) {
            const half4 c = *reinterpret_cast<const half4*>(cap + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += (float)c[r];
          }
          if (cfp && n < p.N) {
            const float4v c = *reinterpret_cast<const float4v*>(cfp + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += c[r];
          }
          half4 y;
#pragma unroll
          for (int r = 0; r < 4; ++r) y[r] = (half_t)v[r];
          *reinterpret_cast<half4*>(st + (16 * i + fr) * L.RS16 + 16 * j + 4 * fg) = y;
        }
      }
      wave_sync();
#pragma unroll
      for (int it = 0; it < NIT16; ++it) {
        const int id = lane + 64 * it;
        const int r = id / CPR, c8 = id - r * CPR;
        const int m = mw + h * (L.WM / L.NPASS16) + r, n = nw + c8 * 8;
        if (id >= NCH16 || m >= p.M || n >= p.N) continue;
        half8 o = *reinterpret_cast<const half8*>(st + r * L.RS16 + c8 * 8);
        if (res) {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)o[j] + (float)rr[it][j]);
        }
        if (p.diag & 8) asm volatile("" ::"v"(o));
        else *reinterpret_cast<half8*>(c_at(m, n)) = o;
      }
      wave_sync();
    }
    return;
  }
  if constexpr (G::UP2X) return;  // (sdmoe_conv_up2x has no activation and no residual: the fp16 path above)
  if constexpr (G::GEGLU) {
    // lane-derived epilogue values from an opaque copy of the lane id: nothing of this epilogue can be hoisted
    // above the main loop (hoisted addresses kept the table-GELU variant's K loop in scratch)
    int lane_o = lane;
    asm volatile("" : "+v"(lane_o));
    const int fr_e = lane_o & 15, fg_e = lane_o >> 4;
    // Routed GEGLU on the swapped fragments, value and gate paired in registers by the weight layout: lane
    // (fr, fg) holds columns 16 j + 4 fg .. +3 of row 16 i + fr, i.e. [value, value, gate, gate] of neurons
    // 8 j + 2 fg, +1 (W rows interleaved [v 2 | g 2] per neuron pair: no cross-lane move; the [v 8 | g 8] layout
    // of rounds 1-3 needed two v_permlane32_swap per fragment, 2 of its 11 epilogue instructions). The fp16
    // product and the activated gate (both exact fp16 values) are staged in LDS per wave ([RG rows][NH neurons]
    // each; the 16 rows x 4 lanes of a 4-B store phase hit 64 distinct banks at NH = 40), then copied out as 16-B
    // row chunks, and every (row, expert) lane sums its expert's gates in neuron order in fp32 -- the rounding
    // points of sdmoe_linear + sdmoe_geglu_route (bit-identical). LDS traffic per wave tile: 4 x WM x NH x 2 B.
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    constexpr int NH = L.WN / 2;                    // neurons of this wave's tile
    constexpr int FPP = L.FM % 2 == 0 ? 2 : 1;      // fragment rows per staging pass
    constexpr int RG = 16 * FPP;                  // rows per staging pass
    constexpr int GST = L.NW * 2 * RG * NH * 2;     // staging bytes of all waves
    static_assert(NH % 8 == 0, "whole 16-B product chunks per row");
    static_assert(GST + L.NW * L.WN * 4 <= L.SMEM1, "GEGLU staging and bias must fit in the kernel's LDS");
    static_assert(GST + L.NW * L.WN * 4 == L.G_STAGING, "GEGLU staging size as the layout states it");
    // staging base: with the GELU table prefetched into ring stage nk % NSTAGE, the stage of the last K-step (free
    // since the barrier above) holds the staging; otherwise offset 0 and a late-loaded table behind the staging
    constexpr bool gtab = L.TAB_OK;  // MODE_GEGLU_GT: launched only with a registered table and act = GELU
    char* const sbase = (L.TAB_PREFETCH && gtab) ? smem + ((nk - 1) % NSTAGE) * L.STAGE : smem;
    const half_t* const tab = reinterpret_cast<const half_t*>(
        L.TAB_PREFETCH ? smem + (nk % NSTAGE) * L.STAGE + L.STAGE - TAB_BYTES : smem + L.TAB_LATE_OFF);
    if (!L.TAB_PREFETCH && gtab) {  // no stage holds the table: load it now (the ring is idle)
      issue_gelu_tab(smem + L.TAB_LATE_OFF);
    }
    if (gtab) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // every wave's table pieces visible
    }
    half_t* sp = reinterpret_cast<half_t*>(sbase) + wave * 2 * RG * NH;  // products [RG][NH]
    half_t* sg = sp + RG * NH;                                           // activated gates [RG][NH]
    float* gbias = reinterpret_cast<float*>(sbase + GST) + wave * L.WN;    // this wave's WN bias values (fp32)
    for (int c = lane_o; c < L.WN; c += 64) gbias[c] = G::LN ? p.ln_bias[nw + c] : (float)p.bias[nw + c];
    wave_sync();
    const int nsel = 2 * fg_e;  // this lane's neuron pair in every fragment: 8 j + nsel, +1
    constexpr int CPO = NH / 8, RPI = 64 / CPO;  // copy-out: 16-B chunks per staged row, rows per 64-lane round
    const int lr = lane_o / CPO, lc = lane_o - (lane_o / CPO) * CPO;
    half_t* const cout = p.C + (long)(mw + lr) * p.ldc + nw / 2 + 8 * lc;
    // this lane's bias quads in every fragment (columns 16 j + 4 fg .. +3: value, value, gate, gate), hoisted out
    // of the rows (the table GELU's epilogue reads them from LDS per fragment instead: its temporaries need those
    // 20 VGPRs)
    float4v bq[L.FN];
#pragma unroll
    for (int j = 0; j < L.FN; ++j)
      bq[j] = gtab ? (float4v){0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const float4v*>(gbias + 16 * j + 4 * fg_e);
    auto stage_pass = [&](int h, auto act_tag) {
      constexpr int ACTK = decltype(act_tag)::value;  // 0: ReLU, 1: GELU from the LDS table, 2: apply_act
      constexpr bool RELU = ACTK == 0;
#pragma unroll
      for (int ii = 0; ii < FPP; ++ii) {
        const int i = h * FPP + ii;
        float la = 0.f, lc = 0.f;
        if constexpr (G::LN) {
          const int rl = wr * L.WM + 16 * i + fr_e;
          la = ln_row[2 * rl];
          lc = ln_row[2 * rl + 1];
        }
#pragma unroll
        for (int j = 0; j < L.FN; ++j) {
          float4v v = acc[i][j];
          if constexpr (G::LN) {  // rstd * (acc - mean * wsum); ln_bias is the bias below
            const float4v ws = *reinterpret_cast<const float4v*>(ln_col + wc * L.WN + 16 * j + 4 * fg_e);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(la, v[r], lc * ws[r]);
          }
          const float4v b = ACTK == 1 ? *reinterpret_cast<const float4v*>(gbias + 16 * j + 4 * fg_e) : bq[j];
          const h2 yv = {(half_t)(v[0] + b[0]), (half_t)(v[1] + b[1])};
          const h2 yg = {(half_t)(v[2] + b[2]), (half_t)(v[3] + b[3])};
          h2 ga;
          if constexpr (RELU) ga = __builtin_elementwise_max(yg, (h2){(half_t)0.f, (half_t)0.f});
          else if constexpr (ACTK == 1) ga = (h2){gelu_tab_h(yg[0], tab), gelu_tab_h(yg[1], tab)};
          else ga = (h2){(half_t)apply_act((float)yg[0], p.act), (half_t)apply_act((float)yg[1], p.act)};
          const int off = (16 * ii + fr_e) * NH + 8 * j + nsel;
          *reinterpret_cast<h2*>(sp + off) = yv * ga;  // fp16 x fp16 is exact in fp32: rounds like the unfused path
          *reinterpret_cast<h2*>(sg + off) = ga;
          // the table GELU's temporaries: one fragment at a time (interleaving all FN pushed 256x320 into scratch)
          if constexpr (ACTK == 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
    };
#pragma unroll
    for (int h = 0; h < L.FM / FPP; ++h) {
      if constexpr (gtab) stage_pass(h, std::integral_constant<int, 1>());
      else if (p.act == ACT_RELU) stage_pass(h, std::integral_constant<int, 0>());
      else stage_pass(h, std::integral_constant<int, 2>());
      wave_sync();
      const int mr0 = mw + h * RG;
      // copy-out: lane -> (row lr + RPI it, 16-B chunk lc) with a fixed per-lane chunk, so the global address is the
      // hoisted per-lane pointer plus a uniform row offset (no per-chunk 64-bit index arithmetic)
#pragma unroll
      for (int it = 0; it < (RG + RPI - 1) / RPI; ++it) {
        const int r = it * RPI + lr;
        if (lr < RPI && r < RG) {
          const half8 o = *reinterpret_cast<const half8*>(sp + r * NH + 8 * lc);
          if (p.diag & 8) asm volatile("" ::"v"(o));
          else if (mr0 + r < p.M) *reinterpret_cast<half8*>(cout + (long)(h * RG + it * RPI) * p.ldc) = o;
        }
      }
      if (p.score) {
        switch (p.esize) {
          case 20: expert_sums<20, NH, RG>(p, sg, mr0, nw, lane_o); break;
          case 10: expert_sums<10, NH, RG>(p, sg, mr0, nw, lane_o); break;
          case 40: expert_sums<40, NH, RG>(p, sg, mr0, nw, lane_o); break;
          case 8: expert_sums<8, NH, RG>(p, sg, mr0, nw, lane_o); break;
          case 5: expert_sums<5, NH, RG>(p, sg, mr0, nw, lane_o); break;
          case 4: expert_sums<4, NH, RG>(p, sg, mr0, nw, lane_o); break;
          case 2: expert_sums<2, NH, RG>(p, sg, mr0, nw, lane_o); break;
          default: expert_sums<1, NH, RG>(p, sg, mr0, nw, lane_o); break;
        }
      }
      wave_sync();
    }
    return;
  }
  // fp32 path (activation, residual): stage the raw accumulators (one b128 per fragment), then epilogue8 on
  // 8-column row chunks
  float* st = reinterpret_cast<float*>(smem) + wave * (L.WM / L.NPASS) * L.WN_PAD;
#pragma unroll
  for (int h = 0; h < L.NPASS; ++h) {
#pragma unroll
    for (int i = 0; i < L.FM / L.NPASS; ++i)
#pragma unroll
      for (int j = 0; j < L.FN; ++j)
        *reinterpret_cast<float4v*>(st + (16 * i + fr) * L.WN_PAD + 16 * j + 4 * fg) = acc[h * (L.FM / L.NPASS) + i][j];
    wave_sync();
    for (int id = lane; id < (L.WM / L.NPASS) * CPR; id += 64) {
      const int r = id / CPR, c8 = id - r * CPR;
      const int m = mw + h * (L.WM / L.NPASS) + r, n = nw + c8 * 8;
      if (m >= p.M || n >= p.N) continue;
      const float* sp = st + r * L.WN_PAD + c8 * 8;
      const float4v v0 = *reinterpret_cast<const float4v*>(sp), v1 = *reinterpret_cast<const float4v*>(sp + 4);
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      epilogue8(p, m, n, v);
    }
    wave_sync();
  }
}

// split-K combine: ordered (deterministic) sum of the fp32 slabs + the fused epilogue
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmParams p) {
  const long nchunk = (long)p.M * (p.N / 8);
  for (long id = blockIdx.x * 256L + threadIdx.x; id < nchunk; id += (long)gridDim.x * 256) {
    const int m = (int)(id / (p.N / 8)), n = (int)(id % (p.N / 8)) * 8;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < p.ksplit; ++s) {
      const float* sp = p.part + ((long)s * p.M + m) * p.N + n;
      float4v a = *reinterpret_cast<const float4v*>(sp), b = *reinterpret_cast<const float4v*>(sp + 4);
      v[0] += a[0]; v[1] += a[1]; v[2] += a[2]; v[3] += a[3];
      v[4] += b[0]; v[5] += b[1]; v[6] += b[2]; v[7] += b[3];
    }
    epilogue8(p, m, n, v);
  }
}

// the same combine for MODE_CONV_UP2X: slab column n = phase * Cout + channel (Cout % 8 == 0: a chunk lies in one
// phase), + bias[channel], stored at the phase's output row (up2x_out_row, as the fp16 epilogue)
__global__ __launch_bounds__(256) void splitk_reduce_up2x_kernel(GemmParams p) {
  const long nchunk = (long)p.M * (p.N / 8);
  const int cout = p.N >> 2;
  for (long id = blockIdx.x * 256L + threadIdx.x; id < nchunk; id += (long)gridDim.x * 256) {
    const int m = (int)(id / (p.N / 8)), n = (int)(id % (p.N / 8)) * 8;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < p.ksplit; ++s) {
      const float* sp = p.part + ((long)s * p.M + m) * p.N + n;
      float4v a = *reinterpret_cast<const float4v*>(sp), b = *reinterpret_cast<const float4v*>(sp + 4);
      v[0] += a[0]; v[1] += a[1]; v[2] += a[2]; v[3] += a[3];
      v[4] += b[0]; v[5] += b[1]; v[6] += b[2]; v[7] += b[3];
    }
    const int ph = n / cout, c = n - ph * cout;
    if (p.bias) {
      const half8 bb = *reinterpret_cast<const half8*>(p.bias + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += (float)bb[j];
    }
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)v[j];
    if (p.diag & 8) asm volatile("" ::"v"(o));
    else *reinterpret_cast<half8*>(p.C + up2x_out_row(m, p.H, p.Wd, ph) * p.ldc + c) = o;
  }
}

}  // namespace
