// MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950, fp16 in / fp32 accumulate / fp16 out.
//
// One kernel template covers every dense projection of the SD U-Net step:
//   * Linear layers (attention q/k/v/out, proj_in/proj_out 1x1 convs, GEGLU proj, FFN down-proj, time MLP):
//     activations [M, K] row-major (any row stride), weights [N, K] (nn.Linear layout);
//   * ResNet 3x3 convolutions (stride 1/2, fused nearest-2x upsample) on NHWC activations: weights
//     [Cout][Cin/64][3][3][64] so K = 9*Cin is contiguous per output channel, every 64-wide K-step is one tap of
//     one 64-channel slice, and the 9 taps of a slice are consecutive K-steps (L2 reuse of the activation rows).
// Main loop: 256 threads = 2x2 waves, BK = 64, 16x16x32 f16 MFMA. Both operand tiles go HBM -> LDS with
// global_load_lds_dwordx4 (LDS-DMA, no register staging), one 1-KiB wave-instruction per 8 rows; conv halo
// rows and M/N tails point at a zero line. A 3-stage LDS ring keeps two K-steps in flight behind a counted
// `s_waitcnt vmcnt` and one raw s_barrier per K-step. The LDS image is XOR-swizzled by pre-swizzling the
// per-lane SOURCE chunk (LDS-DMA writes lane-linearly), so 16 consecutive rows read conflict-free.
// BN = 160 divides every SD channel count (320*k), so N = 320/640/1280/2560/... tiles exactly.
// Small grids (8x8 / 16x16 latents, K up to 23040) split K over workgroups: fp32 partial slabs + a
// deterministic ordered reduce kernel that also runs the epilogue.
// Epilogue (fused): + bias[n] + coladd[image][n] (time embedding) -> activation -> + residual[m][n],
// staged through LDS so stores are 16 B per lane.
#include <array>
#include <utility>

#include "tune.h"
#include "../../include/sdmoe.h"
#include "gemm_kernel.h"

namespace {

// ---- launch planning (host only) ----------------------------------------------------------------------------
// A launch is a Plan: everything the host decides about it. Three planners make one from the GemmParams shape fields,
// the knobs, device_cus() and the workspace's presence and size, dereferencing no pointer and launching nothing:
// plan_launch (dense and masked linears, shifted-tile convs), plan_geglu, plan_halo. launch() runs a plan;
// sdmoe_gemm_plan / sdmoe_conv_plan report one.
// The split (with the K walk every tile of a family shares) is the only thing that decides each output's fp32
// summation order -- tile shape and wave arrangement do not -- so the dense split is computed by ONE function
// (plan_split) from the chosen tile, and the masked modes (MODE_KEEP / WMASK / KEEPW) take the plain GEMM's plan for
// their shape: a keep- or Wanda-masked product is bit-identical to masking the operand first and running sdmoe_linear
// by construction, not by a restated copy of the plain rules.
enum TileId { T128x160, T64x160, T256x320, T256x160_42, T256x320_42, T128x320, T128x160_42, T64x320, T128x32, T128x64,
              T128x128, T64x128, NTILE };
struct TileShape { int bm, bn, wmw, wnw; };
constexpr TileShape kTile[NTILE] = {{128, 160, 2, 2}, {64, 160, 2, 2}, {256, 320, 2, 4}, {256, 160, 4, 2},
                                    {256, 320, 4, 2}, {128, 320, 2, 4}, {128, 160, 4, 2}, {64, 320, 2, 4},
                                    {128, 32, 2, 2},  {128, 64, 2, 2},  {128, 128, 2, 2}, {64, 128, 2, 2}};
struct Plan {
  int mode;     // the kernel's MODE; mode_halo(mode) = the halo-conv family, else the shifted / plain tile family
  int tile;     // TileId (halo: BM x 320 on 2 x 4 waves, T128x320 or T256x320)
  int bk, stages;  // the LDS ring: K depth of one stage, 64 (tiles) or 32 (halo), and its slots
  int ksplit;   // split-K factor (> 1: fp32 slabs in the workspace + splitk_reduce_kernel)
  int kchunk;   // K units per split: 64-deep K-steps (tiles) or 32-channel slices of the main input (halo)
  int kchunk2;  // halo: folded-shortcut K-steps per split
  int mfast;    // tile order M-fastest
};
// a tile rule's choice: the tile, its split-K wish (0 = plan_split's policy), its ring depth wish (0 = tile_plan's)
struct TileRule { int tile, ks_want, stages_want; };

// the gemm_kernel instantiations the library is built with: launch() reaches exactly these
constexpr bool built(int mode, int tile) {
  if (mode_halo(mode)) return (tile == T128x320 && mode != MODE_CONVHUP64) || (tile == T256x320 && mode != MODE_CONVHUP16);
  if (mode == MODE_CONV_UP2X)  // the tiles choose_tile's dense rules and the tile knob's values 1-4 and 6 reach
    return tile == T128x160 || tile == T64x160 || tile == T256x320 || tile == T256x160_42 || tile == T128x320 ||
           tile == T128x64 || tile == T128x128 || tile == T64x128;
  if (mode_geglu(mode))  // BN in {160, 320} only (wave tile width 80 = 40 neurons = whole experts)
    return tile == T128x160 || tile == T64x160 || tile == T256x320 || tile == T256x160_42 || tile == T256x320_42 ||
           (tile == T128x160_42 && mode != MODE_GEGLU_GT);  // (no room for the GELU table behind that tile's staging)
  if (tile == T128x160_42 || tile == T64x320) return mode == MODE_GEMM || mode == MODE_CONV || mode == MODE_GEMM_LN;
  if (tile == T128x32) return mode == MODE_CONV;
  return true;
}
// whether the kernel's layout with a 3-slot ring of 64-deep stages fits the 160 KiB of LDS (the answer of the formula
// this replaced on every (mode, tile) pair: a changed answer would add or drop a 3-stage kernel symbol in launch_kernel)
constexpr bool fits3(const TileShape& t, int mode) {
  return GemmLayout{t.bm, t.bn, t.wmw, t.wnw, mode, 3, 64}.SMEM <= 160 * 1024;
}

// compute units of the current device (both split policies size their grids by it; 256 on MI355X), latched after the
// first query that succeeds; 256 while no device answers, e.g. sdmoe_gemm_plan on a CPU host. Splits -- hence the fp32
// summation order of split-K outputs -- are per-device-SKU by design.
int device_cus() {
  static int cus = 0;
  int dev = 0, n = 0;
  if (!cus && hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
    cus = n;
  return cus ? cus : 256;
}

// split-K factor of a launch on tile t (mode: the tile rule's MODE; ws: whether a slab workspace was handed in)
int plan_split(const TileShape& t, int mode, const GemmParams& p, bool ws, long ws_floats, int ks_want) {
  const int ntiles = ((p.M + t.bm - 1) / t.bm) * ((p.N + t.bn - 1) / t.bn);
  const int nk = p.K / 64;
  const int cus = device_cus();
  int ksplit = 1;
  // fill the chip: split K when the tile grid covers well under one wave of CUs
  const int forced = knob(KNOB_KSPLIT);
  if (ws && (forced > 0 || ks_want > 0)) {
    ksplit = forced > 0 ? forced : ks_want;
    if (ksplit > nk) ksplit = nk;
  } else if (ws && (mode == MODE_CONV || mode == MODE_CONV_UP) && ntiles <= 16 && nk >= 64) {
    // latency regime (one prompt per call, base_receiver.py:73: 8x8 / 16x16 / 32x32 convs at batch 2): up to two
    // workgroups per CU, >= 11 K-steps per split, <= 64 MB of fp32 slabs -- B = 1 sweep (profiles/r05_b1_split_sweep.txt):
    // 8x8 1280 -> 1280 28.1 -> 23.5 us, 2560 -> 1280 44.3 -> 29.6, 16x16 stride 2 39.9 -> 22.0, 32x32 1280 -> 640
    // 64.2 -> 55.2 (at most 8 splits before)
    ksplit = (2 * cus + ntiles - 1) / ntiles;
    if (ksplit > 24) ksplit = 24;
    if (ksplit > nk / 11) ksplit = nk / 11;
    while (ksplit > 1 && (long)ksplit * p.M * p.N * 4 > (64L << 20)) --ksplit;
  } else if (ws && ntiles < 3 * cus / 4 && nk >= 16) {
    ksplit = (cus + ntiles - 1) / ntiles;
    if (ksplit > 8) ksplit = 8;
    if (ksplit > nk / 4) ksplit = nk / 4;
  }
  while (ksplit > 1 && (long)ksplit * p.M * p.N > ws_floats) --ksplit;  // the slabs fit the workspace
  if (ksplit < 1) ksplit = 1;
  // no empty trailing split: ceil(nk / ksplit) K-steps per split, as many splits as that takes (e.g. nk = 180 at 16
  // wanted: 12 per split -> 15 splits, not a 16th that writes a zero slab the reduce then reads)
  const int kchunk = (nk + ksplit - 1) / ksplit;
  return (nk + kchunk - 1) / kchunk;
}

// the plan of a tile-family launch from its tile, split and ring-depth wish
Plan tile_plan(int mode, int tile, const GemmParams& p, int ksplit, int stages_want) {
  const TileShape& t = kTile[tile];
  const int ntiles = ((p.M + t.bm - 1) / t.bm) * ((p.N + t.bn - 1) / t.bn);
  const int nk = p.K / 64;
  Plan pl{};
  pl.mode = mode; pl.tile = tile; pl.bk = 64; pl.ksplit = ksplit;
  pl.kchunk = (nk + ksplit - 1) / ksplit;
  // M-fastest order for split-K convs only: their weight slices (up to 29 MB at the 16x16 level) were re-fetched by
  // every XCD (PMC FETCH_SIZE of the split-K conv launches 140 -> 46 MB, time neutral); the M = 1024 split-K linears
  // measured 2 us slower with it
  pl.mfast = (pl.ksplit > 1 && knob(KNOB_MFAST) && (mode == MODE_CONV || mode == MODE_CONV_UP || mode == MODE_CONV_UP2X)) ? 1 : 0;
  // 64-deep K-steps (a 32-deep 4/5-stage ring measured slower on every shape; the kernel is generic in BK).
  // 4-wave tiles: 2-stage ring (2 workgroups/CU) when the grid has >= ~300 workgroups, else 3-stage; 8-wave
  // tiles: 3-stage where it fits in LDS -- measured crossovers on MI355X.
  const int stages = knob(KNOB_STAGES) ? knob(KNOB_STAGES)
                                       : (stages_want ? stages_want : ((t.wmw * t.wnw == 4 && ntiles * pl.ksplit >= 300) ? 2 : 3));
  pl.stages = (stages == 2 || !fits3(t, mode)) ? 2 : 3;
  return pl;
}

// Halo policy (KNOB_HALO, values in include/sdmoe.h): the default takes halo tiles where they measured faster than the
// shifted-tile kernel: 64-wide outputs (256-row tiles), 16-wide ones on 256-row tiles (a whole image), the 32 -> 64,
// 16 -> 32 (256-row tiles) and 8 -> 16 upsample convs, 32-wide outputs with Cin >= 1280 (256-row tiles). Every 128-row
// tile instead (2) ran 5-17 % slower on 32- / 16-wide outputs (their 32-deep K-steps carry half the MFMAs per barrier);
// every 32-wide output on 256-row tiles (3) 135.1 vs 118.0 us at 640 -> 640.

// the plan of a halo conv on tile (BM x 320, 8 waves 2 x 4, BK 32, 4-slot B ring): K split over whole 32-channel slices
// when the tile grid is under ~one wave of CUs
Plan halo_plan(int tile, int mode, const GemmParams& p, bool ws, long ws_floats) {
  const int cus = device_cus();
  const int ntiles = (p.M / kTile[tile].bm) * (p.N / 320);
  const int nsl = p.Cin / 32;
  int ksplit = 1;
  const int forced = knob(KNOB_KSPLIT);
  if (ws && forced > 0) {  // sweeps: at most one 32-channel slice per split
    ksplit = forced < nsl ? forced : nsl;
  } else if (ws && ntiles <= 32) {
    // latency regime (batch 2: whole 16x16 images, the 8 -> 16 upsample, 64x64 at 32 tiles): up to two workgroups
    // per CU, >= 2 slices per split, <= 96 MB of fp32 slabs -- B = 1 sweep: 16x16 1280 -> 1280 56.1 -> 40.9 us
    // (20 splits), 2560 -> 1280 91.7 -> 55.3, 8 -> 16 upsample 38.0 -> 31.7 (at most 8 splits before)
    ksplit = (2 * cus + ntiles - 1) / ntiles;
    if (ksplit > 32) ksplit = 32;
    if (ksplit > nsl / 2) ksplit = nsl / 2;
    // whole rounds of one 8-wave workgroup per CU: 16 tiles x 20 splits left 64 workgroups alone in a second
    // round (8 -> 16 upsample at one prompt: 43.2 vs 30.9 us with 16 splits, profiles/r05_b1_conv_split_sweep.txt)
    if (ntiles * ksplit > cus && ntiles <= cus) ksplit = (cus / ntiles) * ((ksplit * ntiles) / cus);
    while (ksplit > 1 && (long)ksplit * p.M * p.N * 4 > (96L << 20)) --ksplit;
  } else if (ws && ntiles < 200) {
    ksplit = (cus + ntiles - 1) / ntiles;  // 6 / 8 splits: 172 vs 128 us at 16x16 x 1280 (r04)
    if (ksplit > 8) ksplit = 8;
    if (ksplit > nsl / 2) ksplit = nsl / 2;
  }
  while (ksplit > 1 && (long)ksplit * p.M * p.N > ws_floats) --ksplit;  // the slabs fit the workspace
  if (ksplit < 1) ksplit = 1;
  Plan pl{};
  pl.mode = mode; pl.tile = tile; pl.bk = 32; pl.stages = 4;
  pl.kchunk = (nsl + ksplit - 1) / ksplit;
  pl.ksplit = (nsl + pl.kchunk - 1) / pl.kchunk;
  pl.kchunk2 = ((p.K - 9 * p.Cin) / 32 + pl.ksplit - 1) / pl.ksplit;
  pl.mfast = pl.ksplit > 1 ? knob(KNOB_MFAST) : 0;
  return pl;
}

// stride-1 or upsampling 3x3 conv (+ folded shortcut: the K-steps past 9 * Cin) on halo tiles: output widths 64, 32
// and 16, N a multiple of 320; false = not a halo shape (the shifted-tile path, plan_launch). gn: the conv applies a
// GroupNorm to its staged input (sdmoe_conv3x3_gn), which only the 64-wide tiles over whole 256-row groups do, for up
// to the kernel's GN_MAXC = 1280 channels of fp32 scale + shift in LDS
bool plan_halo(const GemmParams& p, bool ws, long ws_floats, bool gn, Plan* pl) {
  const int halo = knob(KNOB_HALO);
  if (!halo || knob(KNOB_TILE) || p.stride != 1 || p.N % 320 || p.Cin % 32 || (p.K - 9 * p.Cin) % 32) return false;
  if (gn && (p.upsample || p.Wd != 64 || (p.H * p.Wd) % 256 || p.Cin > 1280)) return false;
  const auto take = [&](int tile, int mode) { *pl = halo_plan(tile, mode, p, ws, ws_floats); return true; };
  if (p.upsample) {  // output width 2 W, output rows per image 2 H
    if (p.K != 9 * p.Cin) return false;
    const int ohw = 4 * p.H * p.Wd;
    if (p.Wd == 32 && ohw % 256 == 0) return take(T256x320, MODE_CONVHUP64);
    if (p.Wd == 8 && ohw % 128 == 0) return take(T128x320, MODE_CONVHUP16);  // 125.6 vs 137.0
    // one prompt per call (<= 32 tiles of 256 output rows): 128-row tiles, 68.8 vs 72.5 us at 2 images
    if (halo == 1 && p.Wd == 16 && ohw % 128 == 0 && (p.M / 256) * (p.N / 320) <= 32)
      return take(T128x320, MODE_CONVHUP32);
    // 16 -> 32 upsample on 256-row tiles (8 output rows, K split over slices): 360.3 vs 383.1-395.8 us
    if (halo != 2 && p.Wd == 16 && ohw % 256 == 0) return take(T256x320, MODE_CONVHUP32);
    if (halo < 2) return false;
    if (p.Wd == 16 && ohw % 128 == 0) return take(T128x320, MODE_CONVHUP32);  // 449 vs 383 us
    return false;
  }
  const int hw = p.H * p.Wd;
  // 64-wide outputs at one prompt (<= 32 tiles of 256 rows): 128-row tiles (two output rows), twice the workgroups
  // for the split to fill the chip with: 33.6 vs 41.0 us (320 -> 320) and 43.5 vs 51.1 (640 -> 320) at 2 images,
  // --batch 1 +0.8 % (profiles/r05_halo64_b1.txt)
  if (halo == 1 && p.Wd == 64 && hw % 128 == 0 && (p.M / 256) * (p.N / 320) <= 32)
    return take(T128x320, MODE_CONVH64);
  if (p.Wd == 64 && hw % 256 == 0) return take(T256x320, MODE_CONVH64);
  // one prompt per call (<= 32 tiles of 256 rows): 128-row tiles for the 16-wide and the narrow-input 32-wide convs,
  // twice the workgroups for the split -- 31.9 vs 39.9 us (16x16 1280 -> 1280), 32.3 vs 35.2 (32x32 640 -> 640), 38.9
  // vs 41.3 (960 -> 640) at 2 images; the Cin >= 1280 32-wide convs keep 256-row tiles (57.8 vs 52.0 us)
  // (profiles/r05_halo128_b1.txt)
  const bool small = (p.M / 256) * (p.N / 320) <= 32;
  if (halo == 1 && small && p.Wd == 16 && hw % 128 == 0) return take(T128x320, MODE_CONVH16);
  if (halo == 1 && small && p.Wd == 32 && hw % 128 == 0 && p.Cin < 1280) return take(T128x320, MODE_CONVH32);
  // 16-wide outputs: a whole 16x16 image per 256-row tile, K split over slices (1280 -> 1280: 127.6 vs 133.0 us)
  if (halo != 2 && p.Wd == 16 && hw % 256 == 0) return take(T256x320, MODE_CONVH16);
  // 32-wide outputs: halo tiles (8 output rows) for the wide-input convs only (up-block conv1, Cin 1920 / 1280): 292 vs
  // 307 us and 206 vs 208 at 16 images, 62 vs 66 and 52 vs 54 at 2; at Cin 640 / 960 they ran 10-14 % slower
  // (profiles/r05_halo32_geglu_diag.txt)
  if (halo == 1 && p.Wd == 32 && hw % 256 == 0 && p.Cin >= 1280) return take(T256x320, MODE_CONVH32);
  if (halo == 3 && p.Wd == 32 && hw % 256 == 0) return take(T256x320, MODE_CONVH32);
  if (halo < 2) return false;
  if (p.Wd == 32 && hw % 128 == 0) return take(T128x320, MODE_CONVH32);
  if (p.Wd == 16 && hw % 128 == 0) return take(T128x320, MODE_CONVH16);
  return false;
}

// routed-GEGLU linear (MODE_GEGLU / GEGLU_LN / GEGLU_GT): BN in {160, 320} tiles only, no split-K. KNOB_GT320 defaults
// to the table-GELU GEGLU on the 256x320 2x4-wave tiles like the ReLU one (no scratch since the [v 2 | g 2] layout:
// 150.9-154.3 vs 178.2-186.2 us at M = 16384, C = 640; SDXL pipeline +4.0 %, same box); its 256x160 4x2 tiles were
// rounds 3-4's until the layout change (364 B/lane of scratch on 256x320)
Plan plan_geglu(int mode, const GemmParams& p) {
  const int nt320 = ((p.M + 255) / 256) * (p.N / 320);
  const int nt160_128 = ((p.M + 127) / 128) * (p.N / 160);
  const auto on = [&](int tile) { return tile_plan(mode, tile, p, 1, 0); };
  const int forced = knob(KNOB_TILE);
  if (forced == 1) return on(T128x160);
  if (forced == 4) return on(T256x160_42);
  if (mode != MODE_GEGLU_GT && forced == 7) return on(T128x160_42);  // sweep: two workgroups per CU
  if (mode == MODE_GEGLU_GT && forced == 0 && !knob(KNOB_GT320) && p.N % 320 == 0 && nt320 >= 240)
    // the same rows on 256x160 tiles, 8 waves 4 x 2 (wave tile 64 x 80)
    return on(T256x160_42);
  if (p.N % 320 == 0 && nt320 >= 240) {
    // 2x4 waves (wave tile 128 rows x 40 neurons): with the row-fastest epilogue its 32-row staging passes are
    // conflict-free (4x2's 16-row passes are not: two 16-lane b128 groups mix column pairs); 174.6 vs 181.2 us at
    // M = 65536, 129.8 vs 132.9 at 16384, 103.4 vs 106.4 at 4096 (same box)
    return on(forced == 5 ? T256x320_42 : T256x320);
  }
  // one prompt per call at the 16x16 level (M = 512, N = 10240): 8-wave 128x160 tiles, 20.5 vs 27.3 us on the 4-wave
  // ones (the 32x32 level's M = 2048 measured 24.3 vs 19.0 with them; profiles/r05_b1_geglu_keep_tiles.txt)
  if (mode != MODE_GEGLU_GT && p.M <= 1024 && nt160_128 >= 128) return on(T128x160_42);
  if (nt160_128 >= 200 || p.M > 2048) return on(T128x160);
  return on(T64x160);
}

// Tile rule of the dense modes (GEMM, CONV, CONV_UP, GEMM_LN); the masked modes plan as MODE_GEMM (plan_launch).
TileRule choose_tile(int mode, const GemmParams& p) {
  const int tm256 = (p.M + 255) / 256;
  const int forced = knob(KNOB_TILE);
  if (forced == 1) return {T128x160, 0, 0};
  if (forced == 2) return {T64x160, 0, 0};
  if (forced == 3 && p.N % 320 == 0) return {T256x320, 0, 0};
  if (forced == 4 && p.N % 160 == 0) return {T256x160_42, 0, 0};
  if (forced == 5 && p.N % 320 == 0) return {T256x320_42, 0, 0};
  if (forced == 6 && p.N % 320 == 0) return {T128x320, 0, 0};
  // sweep-only 8-wave tiles with a 32x80 wave tile (two workgroups per CU on a 2-stage ring)
  if (mode != MODE_CONV_UP && forced == 7 && p.N % 160 == 0) return {T128x160_42, 0, 0};
  if (mode != MODE_CONV_UP && forced == 8 && p.N % 320 == 0) return {T64x320, 0, 0};
  // 8-wave 256x320 tile (wave tile 128x80: 2.5x the MFMA work per LDS byte of 64x80) whenever it alone fills
  // the chip; 256x160 8-wave + split-K for long-K problems whose 128x160 grid is under ~1.2 waves of CUs.
  // Measured on MI355X with tools/gemm_bench.py --tile.
  const int nt320 = tm256 * (p.N / 320);
  const int nt160_128 = ((p.M + 127) / 128) * ((p.N + 159) / 160);
  // (180: the 16x16-level fused QKV, M = 4096 x N = 3840 x K = 1280 -- also SDXL's 32x32 level -- 43.8 vs 49.9 us on
  // 128x160; every other U-Net shape is outside 180..240)
  // 32x32-level projections (M = 16384): the LayerNorm-folded QKV / Q and the plain (no residual) N = 640 GEMM on
  // 128x320 8-wave tiles (wave tile 64x80, one workgroup per CU): 58.8 vs 62.7 us (QKV, N = 1920), 19.5 vs 22.1 us
  // (N = 640) in a same-box tools/gpu_tile_sweep.sh run; the residual / conv shapes measured neutral or slower there
  if ((mode == MODE_GEMM_LN && p.M >= 8192 && p.M <= 16384 && p.N % 320 == 0) ||
      (mode == MODE_GEMM && !p.R && p.act == ACT_NONE && p.M >= 8192 && p.M <= 16384 && p.N == 640 && p.K == 640))
    return {T128x320, 0, 0};
  if (p.N % 320 == 0 && nt320 >= 180) return {T256x320, 0, 0};
  // 1-1.25 waves of 128x160 tiles (M = 4096 x N = 1280 projections at the 16x16 level): 64x160 tiles double
  // the grid to two workgroups per CU — 15-18 % faster in isolation (tools/gpu_tiles_all.sh). Convs keep their
  // tiles: with the convs included the same-box pipeline A/B measured 0.5 % slower.
  if ((mode == MODE_GEMM || mode == MODE_GEMM_LN) && p.N % 160 == 0 && nt160_128 >= 200 && nt160_128 < 320 &&
      p.K <= 5120)
    return {T64x160, 0, 0};
  // convs (tools/gemm_bench.py --tile/--stages sweep, same box): the 16x16-level 3x3 convs (M = 4096, N = 1280,
  // K = 9 x 1280 / 9 x 2560) on the 8-wave 256x320 tile with a 4-way split-K: 120 / 205 us vs 135 / 237 us on
  // 256x160 with a 2-way split (the 32x32 level's 1280 -> 640 conv stays on 128x160: 207 vs 221 us); the
  // 64x64 -> 32x32 stride-2 conv (M = 16384, N = 320) on 64x160 tiles at two workgroups per CU: 38 vs 57 us on
  // 128x160 with a 3-stage ring
  if (mode == MODE_CONV) {
    // 8x8-level 3x3 convs (M = 1024, K = 9 x 1280 / 9 x 2560): 8-wave 128x160 tiles (wave tile 32x80), 2-stage ring
    // (two workgroups per CU), 8-way split-K: 44.6 / 68.2 us vs 51.2 / 72.8 on 256x160 4x2 waves (tile_sweep.py)
    // At one prompt per call (M = 128: 8 tiles) the fixed 8-way split left 64 workgroups streaming ~23 K-steps each
    // behind a 2-stage ring; such grids (<= 16 tiles) take plan_split's latency-regime split instead (16-24 ways)
    if (p.stride == 1 && p.N % 160 == 0 && p.M <= 1024 && p.K >= 9 * 1280)
      return {T128x160_42, nt160_128 <= 16 ? 0 : 8, 2};
    if (p.stride == 1 && p.N % 320 == 0 && nt320 < 240 && p.K >= 9 * 1280 && p.M >= 2048 && p.M <= 4096)
      return {T256x320, 0, 0};
    if (p.stride == 2 && p.N % 160 == 0 && p.M >= 8192) return {T64x160, 0, 0};
    // the 32x32 -> 16x16 and 16x16 -> 8x8 downsamplers (M = 4096 / 1024): a 4-way split-K, two workgroups per CU
    // (their strided-tap A loads want the extra waves in flight): 46.1-46.7 vs 65.7-66.3 us and 46.4-46.9 vs
    // 78.4-80.1 us with the auto ~one-per-CU split of 2, on every tile shape (same box)
    if (p.stride == 2 && p.N % 160 == 0 && p.M < 8192) {
      if (p.M > 2048) return {T128x160, 4, 0};
      // (<= 16 tiles, the 16x16 -> 8x8 downsampler at one prompt: plan_split's latency-regime split)
      const int nt64 = ((p.M + 63) / 64) * (p.N / 160);
      return {T64x160, nt64 <= 16 ? 0 : 4, 0};
    }
  }
  // (the keep-masked down projection at one prompt, <= 128 tiles of 128x160, runs on 64x160 tiles through the plain
  // rule below: 22.3 vs 29.5 us at the 64x64 level, profiles/r05_b1_geglu_keep_tiles.txt)
  // (the collapsed upsample convs under 180 tiles of 256x320 take this rule too: 128x320 tiles ran 62.5 vs 68.0 us in a
  // warm loop but 66.9 vs 62.9 us in the pipeline's kernel trace, 8 -> 16 at 16 images, profiles/upconv_collapse_ab.txt)
  if (p.N % 160 == 0 && p.K >= 2560 && nt160_128 < 300 && !(mode == MODE_CONV && p.stride == 2))
    return {T256x160_42, 0, 0};
  if (mode == MODE_CONV_UP) return {p.N % 160 == 0 ? T128x160 : T128x128, 0, 0};
  // conv_out (N = 8 padded channels): a quarter of 128x64's MFMA padding (31.9 vs 34.8-35.1 us at 64x64 x 320 -> 8,
  // same box)
  if (mode == MODE_CONV && p.N <= 32 && knob(KNOB_NARROW)) return {T128x32, 0, 0};
  if (p.N <= 64) return {T128x64, 0, 0};
  if (p.N % 160 == 0) {
    // plain GEMMs under ~one wave of 128x160 tiles take 64x160 at any M: the 64x64 level's K = 320 projections at one
    // prompt (M = 8192, N = 320: 128 tiles) 7.8 vs 10.6 us, 8.4 vs 11.8 with the residual (r05_b1_linear_tiles.txt)
    if (nt160_128 >= 200 || (p.M > 2048 && mode != MODE_GEMM)) return {T128x160, 0, 0};
    return {T64x160, 0, 0};
  }
  const int nt128 = ((p.M + 127) / 128) * ((p.N + 127) / 128);
  if (nt128 >= 200 || p.M > 2048) return {T128x128, 0, 0};
  return {T64x128, 0, 0};
}

// the tile a masked mode runs the plain GEMM's plan on: the same one where it is instantiated for the mode, with the
// keep-masked A operand on the 4x2-wave arrangement of 256x320 (wave tile 64x160: half the A fragments to mask per
// wave, 61 vs 69 us at M = 65536, N = 320, K = 1280); the split stays the plain GEMM's, so the bits do too
int masked_tile(int mode, int t, const GemmParams& p) {
  if (mode_akeep(mode) && t == T256x320) return T256x320_42;
  if (t == T128x320 || t == T128x160_42 || t == T64x320 || t == T128x32) return p.N % 160 == 0 ? T128x160 : T128x128;
  return t;
}

// plan of a dense or masked launch; masked modes plan as the plain GEMM of the shape
Plan plan_launch(int mode, const GemmParams& p, bool ws, long ws_floats) {
  const bool masked = mode_akeep(mode) || mode_wmask(mode);
  const int pm = masked ? MODE_GEMM : mode;
  const TileRule r = choose_tile(pm, p);
  const int ksplit = plan_split(kTile[r.tile], pm, p, ws, ws_floats, r.ks_want);
  return tile_plan(mode, masked ? masked_tile(mode, r.tile, p) : r.tile, p, ksplit, r.stages_want);
}

// plan of a masked launch with one Wanda mask per rows_per_img-row image (sdmoe_linear_masked_sets): the shape's own
// masked plan where its tile's rows divide an image -- tile and split, hence the bits, of sdmoe_linear_masked -- else a
// 64-row tile (built for every masked mode) with plan_split's split for THAT tile; false = rows_per_img % 64 != 0, a
// tile would straddle two images' masks
bool plan_sets(int mode, const GemmParams& p, int rows_per_img, bool ws, long ws_floats, Plan* pl) {
  *pl = plan_launch(mode, p, ws, ws_floats);
  if (rows_per_img % kTile[pl->tile].bm == 0) return true;
  if (rows_per_img % 64) return false;
  const int tile = p.N % 160 == 0 ? T64x160 : T64x128;
  *pl = tile_plan(mode, tile, p, plan_split(kTile[tile], MODE_GEMM, p, ws, ws_floats, 0), 0);
  return true;
}

// plan of a 3x3 conv: halo tiles where plan_halo takes the shape, else shifted tiles
Plan plan_conv(const GemmParams& p, bool ws, long ws_floats) {
  Plan pl;
  if (plan_halo(p, ws, ws_floats, false, &pl)) return pl;
  return plan_launch(p.upsample ? MODE_CONV_UP : MODE_CONV, p, ws, ws_floats);
}

// ---- the launch -----------------------------------------------------------------------------------------------
template <int MODE, int TILE>
int launch_kernel(const Plan& pl, const GemmParams& p, dim3 grid, hipStream_t s) {
  constexpr TileShape t = kTile[TILE];
  constexpr int NTH = 64 * t.wmw * t.wnw;
  if constexpr (!built(MODE, TILE)) return SDMOE_EUNSUP;
  else if constexpr (mode_halo(MODE)) gemm_kernel<t.bm, t.bn, t.wmw, t.wnw, MODE, 4, 32><<<grid, NTH, 0, s>>>(p);
  else if constexpr (!fits3(t, MODE)) gemm_kernel<t.bm, t.bn, t.wmw, t.wnw, MODE, 2, 64><<<grid, NTH, 0, s>>>(p);
  else if (pl.stages == 2) gemm_kernel<t.bm, t.bn, t.wmw, t.wnw, MODE, 2, 64><<<grid, NTH, 0, s>>>(p);
  else gemm_kernel<t.bm, t.bn, t.wmw, t.wnw, MODE, 3, 64><<<grid, NTH, 0, s>>>(p);
  return SDMOE_OK;
}

// launch_kernel<MODE, tile> at MODE * NTILE + tile
constexpr int NMODE = MODE_CONV_UP2X + 1;
using LaunchFn = int (*)(const Plan&, const GemmParams&, dim3, hipStream_t);
template <int... KEY>
constexpr std::array<LaunchFn, sizeof...(KEY)> launch_table(std::integer_sequence<int, KEY...>) {
  return {{&launch_kernel<KEY / NTILE, KEY % NTILE>...}};
}
constexpr auto kLaunch = launch_table(std::make_integer_sequence<int, NMODE * NTILE>{});

// Runs a plan: the kernel over ntiles x ksplit workgroups and, for a split, the reduce. ws: the slab workspace.
int launch(const Plan& pl, GemmParams p, float* ws, hipStream_t s) {
  const TileShape& t = kTile[pl.tile];
  if (p.w_bstride && p.rows_per_batch % t.bm) return SDMOE_EUNSUP;  // a tile would straddle two images' weights
  if (p.image_set && p.rows_per_batch % t.bm) return SDMOE_EUNSUP;  // ... or two images' Wanda masks
  if (pl.ksplit > 1 && !ws) return SDMOE_EARG;
  p.ksplit = pl.ksplit; p.kchunk = pl.kchunk; p.kchunk2 = pl.kchunk2; p.mfast = pl.mfast;
  p.part = pl.ksplit > 1 ? ws : nullptr;
  p.diag = knob(KNOB_DIAG); p.res16 = knob(KNOB_RES16);
  // fp16 epilogues storing 16-B row pieces straight from the fragments, by default only without a residual: LN-folded
  // projections 4-12 %, plain K = 320 linears ~3 % faster; with a residual its 16-B residual loads measured 3-7 %
  // slower than the staged copy-out. Decided host-side: a device test of R spilled
  const int direct = knob(KNOB_EPI_DIRECT);
  p.epi_direct = direct == 2 || (direct == 1 && p.R == nullptr);
  const dim3 grid(((p.M + t.bm - 1) / t.bm) * ((p.N + t.bn - 1) / t.bn) * pl.ksplit);
  if (const int st = kLaunch[pl.mode * NTILE + pl.tile](pl, p, grid, s)) return st;
  SDMOE_CHECK_LAUNCH();
  if (pl.ksplit > 1) {
    long nchunk = (long)p.M * (p.N / 8);
    int g = (int)((nchunk + 255) / 256);
    if (g > 2048) g = 2048;
    if (pl.mode == MODE_CONV_UP2X) splitk_reduce_up2x_kernel<<<g, 256, 0, s>>>(p);
    else splitk_reduce_kernel<<<g, 256, 0, s>>>(p);
    SDMOE_CHECK_LAUNCH();
  }
  return SDMOE_OK;
}


// ---- elementwise helpers for the GEMM operands ------------------------------------------------------

// GroupNorm apply (+SiLU): Y = act(X * scale[img, c] + shift[img, c]) on [nimg*HW, C] (16 B per thread)
__global__ __launch_bounds__(256) void gn_apply_kernel(const half_t* __restrict__ X, long ldx, int HW, int C,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       int silu, half_t* __restrict__ Y, long ldy, long rows) {
  const int cpr = C / 8;
  const long n = rows * cpr;
  for (long id = blockIdx.x * 256L + threadIdx.x; id < n; id += (long)gridDim.x * 256) {
    const long r = id / cpr;
    const int c = (int)(id - r * cpr) * 8;
    const int img = (int)(r / HW);
    half8 x = *reinterpret_cast<const half8*>(X + r * ldx + c);
    const float* sc = scale + (long)img * C + c;
    const float* sh = shift + (long)img * C + c;
    float4v s0 = *reinterpret_cast<const float4v*>(sc), s1 = *reinterpret_cast<const float4v*>(sc + 4);
    float4v h0 = *reinterpret_cast<const float4v*>(sh), h1 = *reinterpret_cast<const float4v*>(sh + 4);
    float s[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
    float h[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = (float)x[j] * s[j] + h[j];
      if (silu) f = silu_f(f);
      o[j] = (half_t)f;
    }
    *reinterpret_cast<half8*>(Y + r * ldy + c) = o;
  }
}

// Wanda weight mask: Wm[n, k] = bit(n, k) ? 0 : W[n, k]   (bits [N][K/8], little-endian within a byte)
__global__ __launch_bounds__(256) void mask_weight_kernel(const half_t* __restrict__ W, const uint8_t* __restrict__ bits,
                                                          half_t* __restrict__ Wm, long n8) {
  for (long id = blockIdx.x * 256L + threadIdx.x; id < n8; id += (long)gridDim.x * 256) {
    half8 w = reinterpret_cast<const half8*>(W)[id];
    const unsigned b = bits[id];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if ((b >> j) & 1u) w[j] = (half_t)0.f;
    reinterpret_cast<half8*>(Wm)[id] = w;
  }
}

// Wanda bits [N][K/8] (bit k%8 of byte (n, k/8) = W[n, k] removed) -> the GEMM's K-step-major layout
// out[s][n] (uint64) bit j = mask(n, k = perm ? perm[64 s + j] : 64 s + j): one thread per output word. perm maps a
// permuted column position to the original column (the routed FFN down projection's expert-major neuron order).
__global__ __launch_bounds__(256) void wmask_kmajor_kernel(const uint8_t* __restrict__ bits, long ldb, int N, int K,
                                                           const int* __restrict__ perm, unsigned long long* __restrict__ out) {
  const long nwords = (long)(K / 64) * N;
  for (long id = blockIdx.x * 256L + threadIdx.x; id < nwords; id += (long)gridDim.x * 256) {
    const int s = (int)(id / N), n = (int)(id - (long)s * N);
    const uint8_t* row = bits + (long)n * ldb;
    unsigned long long w = 0;
    if (perm) {
      for (int j = 0; j < 64; ++j) {
        const int k = perm[64 * s + j];
        w |= (unsigned long long)((row[k >> 3] >> (k & 7)) & 1u) << j;
      }
    } else {
#pragma unroll
      for (int b = 0; b < 8; ++b) w |= (unsigned long long)row[8 * s + b] << (8 * b);
    }
    out[id] = w;
  }
}

// Unions of concept masks (sdmoe_wmask_union_sets): out[s][w] = OR of masks[c][w] over the concepts c whose bit is set
// in select[s]; one thread per output word, the concepts' words streamed (sets of one launch re-read them from L2)
__global__ __launch_bounds__(256) void wmask_union_sets_kernel(const unsigned long long* __restrict__ masks,
                                                               long mask_stride, const unsigned* __restrict__ select,
                                                               unsigned cmask, int nsets, long words,
                                                               unsigned long long* __restrict__ out) {
  const long n = (long)nsets * words;
  for (long id = blockIdx.x * 256L + threadIdx.x; id < n; id += (long)gridDim.x * 256) {
    const long s = id / words, w = id - s * words;
    unsigned sel = select[s] & cmask;  // (bits past nconcepts name no mask)
    unsigned long long acc = 0;
    while (sel) {
      const int c = __builtin_ctz(sel);
      sel &= sel - 1;
      acc |= masks[c * mask_stride + w];
    }
    out[id] = acc;
  }
}

// LayerNorm fold (sdmoe_ln_fold): one block per output row n of W [N, K]:
//   Wf[n, k] = fp16(W[n, k] * gamma[k]); wsum[n] = sum_k Wf[n, k]; bias_f[n] = bias[n] + sum_k W[n, k] * beta[k]
// (fp32; fixed-order block reduction, so the fold is deterministic)
__global__ __launch_bounds__(256) void ln_fold_kernel(const half_t* __restrict__ W, long ldw, int K,
                                                      const half_t* __restrict__ gamma, const half_t* __restrict__ beta,
                                                      const half_t* __restrict__ bias, half_t* __restrict__ Wf, long ldf,
                                                      float* __restrict__ bias_f, float* __restrict__ wsum) {
  __shared__ float red[2][256];
  const int n = blockIdx.x, tid = threadIdx.x;
  float sw = 0.f, sb = 0.f;
  for (int k = tid; k < K; k += 256) {
    const float w = (float)W[(long)n * ldw + k];
    const half_t wf = (half_t)(w * (float)gamma[k]);
    Wf[(long)n * ldf + k] = wf;
    sw += (float)wf;
    sb = __builtin_fmaf(w, (float)beta[k], sb);
  }
  red[0][tid] = sw;
  red[1][tid] = sb;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    wsum[n] = red[0][0];
    bias_f[n] = red[1][0] + (bias ? (float)bias[n] : 0.f);
  }
}

// GroupNorm fold (sdmoe_gn_fold): one wave per (image, output row n): Wf[i][n, k] = fp16(W[n, k] * scale[i, k]) and
// colbias[i][n] = bias[n] + sum_k float(Wf[i][n, k]) * (shift[i, k] / scale[i, k]) (fp32, fixed-order lane sums + xor
// tree: deterministic). The bias is taken from the ROUNDED weights so that the GEMM computes sum_k Wf * (x + shift /
// scale) with -shift / scale = mean - beta std / gamma, a centre within about one std of the group mean: the fp16
// rounding of Wf then multiplies a centred value. (From the unrounded W -- sum_k W * shift -- the rounding was
// multiplied by the activation's mean with nothing to cancel it: 1.3e-2 relative L2 at a group |mean| / std of 64.)
// Where |scale| < GN_FOLD_MIN_SCALE (scale == 0 above all: a zero gamma) Wf is 0 or an fp16 subnormal, there is
// nothing worth cancelling, shift / scale has no meaning, and the term is W[n, k] * shift[i, k].
// The ratio is one v_rcp_f32 (1 ulp) and a multiply per element; it costs this kernel 3-5 % (DESIGN.md section 4,
// where the mappings that share the ratio between rows are measured too: all slower).
constexpr float GN_FOLD_MIN_SCALE = 6.103515625e-05f;  // 2^-14, the smallest normal fp16
__global__ __launch_bounds__(256) void gn_fold_kernel(const half_t* __restrict__ W, long ldw, int N, int K,
                                                      const half_t* __restrict__ bias, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, half_t* __restrict__ Wf,
                                                      float* __restrict__ colbias) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), img = blockIdx.y;
  if (n >= N) return;
  const float* sc = scale + (long)img * K;
  const float* sh = shift + (long)img * K;
  half_t* wo = Wf + ((long)img * N + n) * K;
  float acc = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    const half8 w = *reinterpret_cast<const half8*>(W + (long)n * ldw + k);
    const float4v s0 = *reinterpret_cast<const float4v*>(sc + k), s1 = *reinterpret_cast<const float4v*>(sc + k + 4);
    const float4v h0 = *reinterpret_cast<const float4v*>(sh + k), h1 = *reinterpret_cast<const float4v*>(sh + k + 4);
    const float s[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
    const float h[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)w[j] * s[j]);
    // The bias must be taken from the very bits that are stored. Left free, the compiler forms the product twice,
    // once fused into the fp16 conversion (v_fma_mixlo_f16) and once as multiply + v_cvt_pk_f16_f32, and the two
    // differ in the last bit for some elements: one ulp of a |Wf| of 16 times a ratio of 2 put the bias 1.6e-2 off
    // the stored weights on a constant group.
    asm volatile("" : "+v"(o));
    *reinterpret_cast<half8*>(wo + k) = o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool centred = __builtin_fabsf(s[j]) >= GN_FOLD_MIN_SCALE;
      acc = __builtin_fmaf(centred ? (float)o[j] : (float)w[j], centred ? h[j] * __builtin_amdgcn_rcpf(s[j]) : h[j],
                           acc);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) colbias[(long)img * N + n] = acc + (bias ? (float)bias[n] : 0.f);
}

// fp16 GELU tables registered per device (sdmoe_set_gelu_table)
constexpr int MAX_DEV = 64;
const void* g_gelu_tab[MAX_DEV] = {};

int grid_for(long n) {
  long g = (n + 255) / 256;
  return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

}  // namespace

const half_t* sdmoe_gelu_tab_current() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return nullptr;
  return (const half_t*)g_gelu_tab[dev];
}

extern "C" int sdmoe_set_gelu_table(const void* table) {
  int dev = 0;
  const hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  if (dev < 0 || dev >= MAX_DEV) return SDMOE_EARG;
  if (table && (reinterpret_cast<uintptr_t>(table) & 15)) return SDMOE_ESHAPE;
  g_gelu_tab[dev] = table;
  return SDMOE_OK;
}

// ---- entry points: validate -> fill -> plan -> launch -----------------------------------------------------------
namespace {

// linear-style operands: A [M, K] (row stride lda), W [N, K] (ldw), C [M, N] (ldc), bias / residual R (ldr) or null;
// SDMOE_ESHAPE when an operand's extent does not fit a buffer descriptor (num_records < OOB)
int fill_linear(GemmParams& p, const void* A, long lda, const void* W, long ldw, const void* bias, const void* R,
                long ldr, void* C, long ldc, int M, int N, int K, int act) {
  p.A = (const half_t*)A; p.lda = lda; p.W = (const half_t*)W; p.ldw = ldw; p.C = (half_t*)C; p.ldc = ldc;
  p.bias = (const half_t*)bias; p.R = (const half_t*)R; p.ldr = ldr;
  p.M = M; p.N = N; p.K = K; p.act = act; p.rows_per_batch = 1;
  const long ab = ((long)(M - 1) * lda + K) * 2, wb = ((long)(N - 1) * ldw + K) * 2;
  if (ab >= (long)OOB || wb >= (long)OOB) return SDMOE_ESHAPE;
  p.a_bytes = (int)ab; p.w_bytes = (int)wb;
  return SDMOE_OK;
}

// the implicit GEMM of a 3x3 conv (pad 1) of nimg H x W x Cin images, K-steps of a Cin2-channel folded 1x1 shortcut
// appended (Cin2 = 0: none): everything the planners read
void conv_shape(GemmParams& p, int nimg, int H, int W, int Cin, int Cin2, int Cout, int stride, int upsample, int act) {
  const int OH = upsample ? 2 * H : (H - 1) / stride + 1, OW = upsample ? 2 * W : (W - 1) / stride + 1;
  p.M = nimg * OH * OW; p.N = Cout; p.K = 9 * Cin + Cin2; p.act = act;
  p.ldw = 9L * Cin + Cin2; p.rows_per_batch = OH * OW;
  p.H = H; p.Wd = W; p.Cin = Cin; p.OH = OH; p.OW = OW; p.stride = stride; p.upsample = upsample;
}

// conv-style operands of a conv_shape()d p: X [nimg*H*W, Cin] (ldx), the weights, bias, per-image column add, residual R
// (ldr) or the shortcut input X2 [nimg*H*W, Cin2] (ldx2), each possibly null, Y (ldy); SDMOE_ESHAPE as fill_linear
int fill_conv(GemmParams& p, const void* X, long ldx, const void* Wt, const void* bias, const void* coladd,
              long coladd_bstride, const void* R, long ldr, const void* X2, long ldx2, void* Y, long ldy) {
  p.A = (const half_t*)X; p.lda = ldx; p.W = (const half_t*)Wt; p.C = (half_t*)Y; p.ldc = ldy;
  p.bias = (const half_t*)bias; p.coladd = (const half_t*)coladd; p.coladd_bstride = coladd_bstride;
  p.R = (const half_t*)R; p.ldr = ldr; p.A2 = (const half_t*)X2; p.lda2 = ldx2;
  const long rows = (long)(p.M / p.rows_per_batch) * p.H * p.Wd;
  const long ab = (rows - 1) * ldx * 2 + (long)p.Cin * 2, wb = (long)p.N * p.ldw * 2;
  const long a2b = X2 ? (rows - 1) * ldx2 * 2 + (long)(p.K - 9 * p.Cin) * 2 : 0;
  if (ab >= (long)OOB || wb >= (long)OOB || a2b >= (long)OOB) return SDMOE_ESHAPE;
  p.a_bytes = (int)ab; p.w_bytes = (int)wb; p.a2_bytes = (int)a2b;
  return SDMOE_OK;
}

}  // namespace

extern "C" int sdmoe_linear(const void* A, long lda, const void* W, long ldw, const void* bias,
                            const void* coladd, long coladd_bstride, int rows_per_batch,
                            const void* R, long ldr, void* C, long ldc, int M, int N, int K, int act,
                            float* workspace, long workspace_floats, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!A || !W || !C || M < 0 || N <= 0 || K <= 0) return SDMOE_EARG;
  if (K % 64 || N % 8 || lda % 8 || ldw % 8 || ldc % 8 || (R && ldr % 8)) return SDMOE_ESHAPE;
  if (coladd && rows_per_batch <= 0) return SDMOE_EARG;
  GemmParams p{};
  if (const int st = fill_linear(p, A, lda, W, ldw, bias, R, ldr, C, ldc, M, N, K, act)) return st;
  p.coladd = (const half_t*)coladd; p.coladd_bstride = coladd_bstride;
  if (rows_per_batch > 0) p.rows_per_batch = rows_per_batch;
  return launch(plan_launch(MODE_GEMM, p, workspace, workspace_floats), p, workspace, (hipStream_t)stream);
}

extern "C" int sdmoe_gn_fold(const void* W, long ldw, int N, int K, const void* bias, const float* scale,
                             const float* shift, int nimg, void* Wf, float* colbias, void* stream) {
  if (N == 0 || nimg == 0) return SDMOE_OK;
  if (!W || !scale || !shift || !Wf || !colbias || N < 0 || K <= 0 || nimg < 0) return SDMOE_EARG;
  if (K % 8 || ldw % 8 || ldw < K) return SDMOE_ESHAPE;
  gn_fold_kernel<<<dim3((N + 3) / 4, nimg), 256, 0, (hipStream_t)stream>>>(
      (const half_t*)W, ldw, N, K, (const half_t*)bias, scale, shift, (half_t*)Wf, colbias);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_linear_per_image(const void* A, long lda, const void* Wf, long ldw, long w_bstride,
                                      const float* colbias, long colbias_bstride, int rows_per_batch, const void* R,
                                      long ldr, void* C, long ldc, int M, int N, int K, float* workspace,
                                      long workspace_floats, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!A || !Wf || !C || M < 0 || N <= 0 || K <= 0 || rows_per_batch <= 0 || w_bstride <= 0) return SDMOE_EARG;
  if (K % 64 || N % 8 || lda % 8 || ldw % 8 || ldc % 8 || (R && ldr % 8) || rows_per_batch % 256 ||
      M % rows_per_batch || w_bstride % 8 || (colbias && colbias_bstride % 4))
    return SDMOE_ESHAPE;
  GemmParams p{};
  if (const int st = fill_linear(p, A, lda, Wf, ldw, nullptr, R, ldr, C, ldc, M, N, K, ACT_NONE)) return st;
  if ((long)(M / rows_per_batch) * w_bstride * 2 >= (long)OOB) return SDMOE_ESHAPE;
  p.w_bstride = w_bstride; p.colf = colbias; p.colf_bstride = colbias_bstride; p.rows_per_batch = rows_per_batch;
  return launch(plan_launch(MODE_GEMM, p, workspace, workspace_floats), p, workspace, (hipStream_t)stream);
}

extern "C" int sdmoe_linear_masked(const void* A, long lda, const void* keep, const void* W, long ldw,
                                   const void* wmask, const void* bias, const void* R, long ldr, void* C, long ldc,
                                   int M, int N, int K, float* workspace, long workspace_floats, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!A || !W || !C || M < 0 || N <= 0 || K <= 0) return SDMOE_EARG;
  if (K % 64 || N % 8 || lda % 8 || ldw % 8 || ldc % 8 || (R && ldr % 8)) return SDMOE_ESHAPE;
  GemmParams p{};
  if (const int st = fill_linear(p, A, lda, W, ldw, bias, R, ldr, C, ldc, M, N, K, ACT_NONE)) return st;
  const long kb = (long)(K / 64) * M * 8, mb = (long)(K / 64) * N * 8;
  if (kb >= (long)OOB || mb >= (long)OOB) return SDMOE_ESHAPE;
  p.keep = (const uint8_t*)keep; p.keep_bytes = keep ? (int)kb : 0;
  p.wmask = (const uint8_t*)wmask; p.wmask_bytes = wmask ? (int)mb : 0;
  const int mode = keep ? (wmask ? MODE_KEEPW : MODE_KEEP) : (wmask ? MODE_WMASK : MODE_GEMM);
  return launch(plan_launch(mode, p, workspace, workspace_floats), p, workspace, (hipStream_t)stream);
}

extern "C" int sdmoe_gemm_plan(int mode, int M, int N, int K, int has_residual, int act, long workspace_floats,
                               int* out) {
  if (!out || M <= 0 || N <= 0 || K <= 0 || workspace_floats < 0) return SDMOE_EARG;
  if (K % 64 || N % 8 || (mode_geglu(mode) && N % 160)) return SDMOE_ESHAPE;
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.act = act; p.rows_per_batch = 1;
  p.R = has_residual ? reinterpret_cast<const half_t*>(out) : nullptr;  // (only its presence enters the plan)
  Plan pl;
  if (mode_geglu(mode)) pl = plan_geglu(mode, p);
  else if (mode == MODE_GEMM_LN) pl = plan_launch(mode, p, false, 0);  // (as sdmoe_linear_ln)
  else if (mode == MODE_GEMM || mode_akeep(mode) || mode_wmask(mode))
    pl = plan_launch(mode, p, workspace_floats > 0, workspace_floats);
  else return SDMOE_EUNSUP;
  const TileShape& t = kTile[pl.tile];
  out[0] = t.bm; out[1] = t.bn; out[2] = t.wmw; out[3] = t.wnw; out[4] = pl.ksplit;
  return SDMOE_OK;
}

extern "C" int sdmoe_linear_masked_sets(const void* A, long lda, const void* keep, const void* W, long ldw,
                                        const void* wmasks, long set_stride, const int* image_set, int nsets,
                                        int rows_per_img, const void* bias, const void* R, long ldr, void* C, long ldc,
                                        int M, int N, int K, float* workspace, long workspace_floats, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!A || !W || !C || !wmasks || !image_set || M < 0 || N <= 0 || K <= 0 || nsets <= 0 || rows_per_img <= 0)
    return SDMOE_EARG;
  if (K % 64 || N % 8 || lda % 8 || ldw % 8 || ldc % 8 || (R && ldr % 8) || M % rows_per_img) return SDMOE_ESHAPE;
  GemmParams p{};
  if (const int st = fill_linear(p, A, lda, W, ldw, bias, R, ldr, C, ldc, M, N, K, ACT_NONE)) return st;
  const long kb = (long)(K / 64) * M * 8, mb = (long)(K / 64) * N * 8;
  if (kb >= (long)OOB || mb >= (long)OOB) return SDMOE_ESHAPE;
  if (set_stride < mb / 8) return SDMOE_EARG;  // (sets would overlap)
  p.keep = (const uint8_t*)keep; p.keep_bytes = keep ? (int)kb : 0;
  p.wmask = (const uint8_t*)wmasks; p.wmask_bytes = (int)mb;
  p.image_set = image_set; p.wset_bytes = set_stride * 8; p.rows_per_batch = rows_per_img;
  Plan pl;
  if (!plan_sets(keep ? MODE_KEEPW : MODE_WMASK, p, rows_per_img, workspace, workspace_floats, &pl)) return SDMOE_EUNSUP;
  return launch(pl, p, workspace, (hipStream_t)stream);
}

extern "C" int sdmoe_gemm_plan_sets(int has_keep, int M, int N, int K, int rows_per_img, int has_residual,
                                    long workspace_floats, int* out) {
  if (!out || M <= 0 || N <= 0 || K <= 0 || rows_per_img <= 0 || workspace_floats < 0) return SDMOE_EARG;
  if (K % 64 || N % 8 || M % rows_per_img) return SDMOE_ESHAPE;
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.act = ACT_NONE; p.rows_per_batch = rows_per_img;
  p.R = has_residual ? reinterpret_cast<const half_t*>(out) : nullptr;  // (only its presence enters the plan)
  Plan pl;
  if (!plan_sets(has_keep ? MODE_KEEPW : MODE_WMASK, p, rows_per_img, workspace_floats > 0, workspace_floats, &pl))
    return SDMOE_EUNSUP;
  const TileShape& t = kTile[pl.tile];
  out[0] = t.bm; out[1] = t.bn; out[2] = t.wmw; out[3] = t.wnw; out[4] = pl.ksplit;
  return SDMOE_OK;
}

extern "C" int sdmoe_wmask_union_sets(const void* masks, long mask_stride, int nconcepts, const unsigned* select,
                                      int nsets, long words, void* out, void* stream) {
  if (nsets == 0 || words == 0) return SDMOE_OK;
  if (!select || !out || nsets < 0 || words < 0 || nconcepts < 0 || nconcepts > 32 || (nconcepts && !masks) ||
      mask_stride < words)
    return SDMOE_EARG;
  const unsigned cmask = nconcepts == 32 ? ~0u : (1u << nconcepts) - 1u;
  wmask_union_sets_kernel<<<grid_for((long)nsets * words), 256, 0, (hipStream_t)stream>>>(
      (const unsigned long long*)masks, mask_stride, select, cmask, nsets, words, (unsigned long long*)out);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_conv_plan(int nimg, int H, int W, int Cin, int Cin2, int Cout, int stride, int upsample,
                               int has_residual, int gn, int act, long workspace_floats, int* out) {
  if (!out || nimg <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin2 < 0 || Cout <= 0 || workspace_floats < 0 ||
      (Cin2 && has_residual))
    return SDMOE_EARG;
  if (Cin % 64 || Cin2 % 64 || Cout % 8) return SDMOE_ESHAPE;
  // (the folded shortcut and the in-kernel GroupNorm exist for plain stride-1 convs only: sdmoe_conv3x3_sc / _gn)
  if (!(stride == 1 || stride == 2) || (upsample && stride != 1) || ((Cin2 || gn) && (stride != 1 || upsample)) ||
      (gn && act != ACT_NONE))
    return SDMOE_EUNSUP;
  GemmParams p{};
  conv_shape(p, nimg, H, W, Cin, Cin2, Cout, stride, upsample, act);
  p.R = has_residual ? reinterpret_cast<const half_t*>(out) : nullptr;  // (only its presence enters the plan)
  Plan pl;
  if (!gn) pl = plan_conv(p, workspace_floats > 0, workspace_floats);
  else if (!plan_halo(p, workspace_floats > 0, workspace_floats, true, &pl)) return SDMOE_EUNSUP;
  const TileShape& t = kTile[pl.tile];
  out[0] = mode_halo(pl.mode); out[1] = t.bm; out[2] = t.bn; out[3] = t.wmw; out[4] = t.wnw;
  out[5] = pl.bk; out[6] = pl.stages; out[7] = pl.ksplit; out[8] = pl.kchunk; out[9] = pl.kchunk2;
  return SDMOE_OK;
}

extern "C" int sdmoe_linear_keep(const void* A, long lda, const void* keep, const void* W, long ldw, const void* bias,
                                 const void* R, long ldr, void* C, long ldc, int M, int N, int K, float* workspace,
                                 long workspace_floats, void* stream) {
  if (M != 0 && !keep) return SDMOE_EARG;
  return sdmoe_linear_masked(A, lda, keep, W, ldw, nullptr, bias, R, ldr, C, ldc, M, N, K, workspace,
                             workspace_floats, stream);
}

extern "C" int sdmoe_linear_geglu(const void* A, long lda, const void* W, long ldw, const void* bias, void* P,
                                  long ldp, int M, int F, int K, int act, void* score, long ld_score, int esize,
                                  void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!A || !W || !bias || !P || M < 0 || F <= 0 || K <= 0) return SDMOE_EARG;
  if (K % 64 || F % 80 || lda % 8 || ldw % 8 || ldp % 8) return SDMOE_ESHAPE;
  if (score && (esize <= 0 || 40 % esize || ld_score < F / esize)) return SDMOE_ESHAPE;
  if (!(act == ACT_GELU || act == ACT_RELU || act == ACT_NONE || act == ACT_SILU)) return SDMOE_EUNSUP;
  GemmParams p{};
  if (const int st = fill_linear(p, A, lda, W, ldw, bias, nullptr, 0, P, ldp, M, 2 * F, K, act)) return st;
  p.score = (half_t*)score; p.ld_score = ld_score; p.esize = esize;
  if (act == ACT_GELU) p.gelu_tab = sdmoe_gelu_tab_current();
  return launch(plan_geglu(p.gelu_tab ? MODE_GEGLU_GT : MODE_GEGLU, p), p, nullptr, (hipStream_t)stream);
}

extern "C" int sdmoe_ln_fold(const void* W, long ldw, int N, int K, const void* gamma, const void* beta,
                             const void* bias, void* Wf, long ldf, float* bias_f, float* wsum, void* stream) {
  if (N == 0) return SDMOE_OK;
  if (!W || !gamma || !beta || !Wf || !bias_f || !wsum || N < 0 || K <= 0 || ldw < K || ldf < K) return SDMOE_EARG;
  ln_fold_kernel<<<N, 256, 0, (hipStream_t)stream>>>((const half_t*)W, ldw, K, (const half_t*)gamma,
                                                     (const half_t*)beta, (const half_t*)bias, (half_t*)Wf, ldf,
                                                     bias_f, wsum);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_linear_ln(const void* A, long lda, const void* Wf, long ldw, const float* bias_f,
                               const float* wsum, float eps, void* C, long ldc, int M, int N, int K, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!A || !Wf || !bias_f || !wsum || !C || M < 0 || N <= 0 || K <= 0) return SDMOE_EARG;
  if (K % 64 || N % 8 || lda % 8 || ldw % 8 || ldc % 8) return SDMOE_ESHAPE;
  GemmParams p{};
  if (const int st = fill_linear(p, A, lda, Wf, ldw, nullptr, nullptr, 0, C, ldc, M, N, K, ACT_NONE)) return st;
  p.ln_wsum = wsum; p.ln_bias = bias_f; p.ln_eps = eps;
  // no split-K (no workspace): a tile's K loop sees whole rows
  return launch(plan_launch(MODE_GEMM_LN, p, false, 0), p, nullptr, (hipStream_t)stream);
}

extern "C" int sdmoe_linear_geglu_ln(const void* A, long lda, const void* W, long ldw, const float* bias_f,
                                     const float* wsum, float eps, void* P, long ldp, int M, int F, int K, int act,
                                     void* score, long ld_score, int esize, void* stream) {
  if (M == 0) return SDMOE_OK;
  if (!A || !W || !bias_f || !wsum || !P || M < 0 || F <= 0 || K <= 0) return SDMOE_EARG;
  if (K % 64 || F % 80 || lda % 8 || ldw % 8 || ldp % 8) return SDMOE_ESHAPE;
  if (score && (esize <= 0 || 40 % esize || ld_score < F / esize)) return SDMOE_ESHAPE;
  if (!(act == ACT_GELU || act == ACT_RELU || act == ACT_NONE || act == ACT_SILU)) return SDMOE_EUNSUP;
  GemmParams p{};
  if (const int st = fill_linear(p, A, lda, W, ldw, nullptr, nullptr, 0, P, ldp, M, 2 * F, K, act)) return st;
  p.score = (half_t*)score; p.ld_score = ld_score; p.esize = esize;
  p.ln_wsum = wsum; p.ln_bias = bias_f; p.ln_eps = eps;  // (GELU from erfc here: the LN variant has no table form)
  return launch(plan_geglu(MODE_GEGLU_LN, p), p, nullptr, (hipStream_t)stream);
}

extern "C" int sdmoe_conv3x3(const void* X, long ldx, int nimg, int H, int W, int Cin,
                             const void* Wt, const void* bias, const void* coladd, long coladd_bstride,
                             const void* R, long ldr, void* Y, long ldy, int Cout, int stride, int upsample,
                             int act, float* workspace, long workspace_floats, void* stream) {
  if (nimg == 0) return SDMOE_OK;
  if (!X || !Wt || !Y || nimg < 0 || H <= 0 || W <= 0 || Cout <= 0) return SDMOE_EARG;
  if (Cin % 64 || Cout % 8 || ldx % 8 || ldy % 8 || (R && ldr % 8)) return SDMOE_ESHAPE;
  if (!(stride == 1 || stride == 2) || (upsample && stride != 1)) return SDMOE_EUNSUP;
  GemmParams p{};
  conv_shape(p, nimg, H, W, Cin, 0, Cout, stride, upsample, act);
  if (const int st = fill_conv(p, X, ldx, Wt, bias, coladd, coladd_bstride, R, ldr, nullptr, 0, Y, ldy)) return st;
  return launch(plan_conv(p, workspace, workspace_floats), p, workspace, (hipStream_t)stream);
}

// the implicit GEMM of the phase-collapsed nearest-2x upsample conv (MODE_CONV_UP2X): rows = low-res pixels, columns =
// (phase, output channel), K = (64-channel slice, 2x2 tap, channel)
namespace {

void up2x_shape(GemmParams& p, int nimg, int H, int W, int Cin, int Cout) {
  p.M = nimg * H * W; p.N = 4 * Cout; p.K = 4 * Cin; p.act = ACT_NONE;
  p.ldw = 4L * Cin; p.rows_per_batch = H * W;
  p.H = H; p.Wd = W; p.Cin = Cin; p.OH = H; p.OW = W; p.stride = 1; p.upsample = 0;
}

// the plan of sdmoe_conv_up2x: the dense tile rules on the collapsed GEMM; false where the chosen tile's columns would
// straddle two phases (Cout % BN != 0) or the tile is not built for the mode
bool plan_up2x(const GemmParams& p, int Cout, bool ws, long ws_floats, Plan* pl) {
  *pl = plan_launch(MODE_CONV_UP2X, p, ws, ws_floats);
  return built(MODE_CONV_UP2X, pl->tile) && Cout % kTile[pl->tile].bn == 0;
}

}  // namespace

extern "C" int sdmoe_conv_up2x(const void* X, long ldx, int nimg, int H, int W, int Cin, const void* Wc, const void* bias,
                               void* Y, long ldy, int Cout, float* workspace, long workspace_floats, void* stream) {
  if (nimg == 0) return SDMOE_OK;
  if (!X || !Wc || !Y || nimg < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return SDMOE_EARG;
  if (Cin % 64 || Cout % 8 || ldx % 8 || ldy % 8) return SDMOE_ESHAPE;
  if (4L * nimg * H * W >= (long)OOB) return SDMOE_ESHAPE;
  GemmParams p{};
  up2x_shape(p, nimg, H, W, Cin, Cout);
  Plan pl;
  if (!plan_up2x(p, Cout, workspace, workspace_floats, &pl)) return SDMOE_EUNSUP;
  if (const int st = fill_conv(p, X, ldx, Wc, bias, nullptr, 0, nullptr, 0, nullptr, 0, Y, ldy)) return st;
  return launch(pl, p, workspace, (hipStream_t)stream);
}

extern "C" int sdmoe_conv_up2x_plan(int nimg, int H, int W, int Cin, int Cout, long workspace_floats, int* out) {
  if (!out || nimg <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || workspace_floats < 0) return SDMOE_EARG;
  if (Cin % 64 || Cout % 8) return SDMOE_ESHAPE;
  GemmParams p{};
  up2x_shape(p, nimg, H, W, Cin, Cout);
  Plan pl;
  if (!plan_up2x(p, Cout, workspace_floats > 0, workspace_floats, &pl)) return SDMOE_EUNSUP;
  const TileShape& t = kTile[pl.tile];
  out[0] = t.bm; out[1] = t.bn; out[2] = t.wmw; out[3] = t.wnw; out[4] = pl.stages; out[5] = pl.ksplit; out[6] = pl.kchunk;
  return SDMOE_OK;
}

extern "C" int sdmoe_conv3x3_sc(const void* X, long ldx, int nimg, int H, int W, int Cin, const void* Wt,
                                const void* bias, const void* coladd, long coladd_bstride, const void* X2, long ldx2,
                                int Cin2, void* Y, long ldy, int Cout, int act, float* workspace,
                                long workspace_floats, void* stream) {
  if (nimg == 0) return SDMOE_OK;
  if (!X || !Wt || !X2 || !Y || nimg < 0 || H <= 0 || W <= 0 || Cout <= 0 || Cin2 <= 0) return SDMOE_EARG;
  if (Cin % 64 || Cin2 % 64 || Cout % 8 || ldx % 8 || ldx2 % 8 || ldy % 8) return SDMOE_ESHAPE;
  GemmParams p{};
  conv_shape(p, nimg, H, W, Cin, Cin2, Cout, 1, 0, act);
  if (const int st = fill_conv(p, X, ldx, Wt, bias, coladd, coladd_bstride, nullptr, 0, X2, ldx2, Y, ldy)) return st;
  return launch(plan_conv(p, workspace, workspace_floats), p, workspace, (hipStream_t)stream);
}

extern "C" int sdmoe_conv3x3_gn(const void* X, long ldx, int nimg, int H, int W, int Cin, const float* gn_scale,
                                const float* gn_shift, int silu, const void* Wt, const void* bias, const void* coladd,
                                long coladd_bstride, const void* R, long ldr, const void* X2, long ldx2, int Cin2,
                                void* Y, long ldy, int Cout, float* workspace, long workspace_floats, void* stream) {
  if (nimg == 0) return SDMOE_OK;
  if (!X || !gn_scale || !gn_shift || !Wt || !Y || nimg < 0 || H <= 0 || W <= 0 || Cout <= 0 || Cin2 < 0) return SDMOE_EARG;
  if (Cin % 64 || Cin2 % 64 || Cout % 8 || ldx % 8 || ldy % 8 || (R && ldr % 8) || (X2 && ldx2 % 8)) return SDMOE_ESHAPE;
  if ((X2 != nullptr) != (Cin2 > 0) || (X2 && R)) return SDMOE_EARG;
  GemmParams p{};
  conv_shape(p, nimg, H, W, Cin, Cin2, Cout, 1, 0, ACT_NONE);
  // only the halo tiles apply the GroupNorm in the kernel: the caller falls back to apply + conv on EUNSUP
  Plan pl;
  if (!plan_halo(p, workspace, workspace_floats, true, &pl)) return SDMOE_EUNSUP;
  if (const int st = fill_conv(p, X, ldx, Wt, bias, coladd, coladd_bstride, R, ldr, X2, ldx2, Y, ldy)) return st;
  p.gn_scale = gn_scale; p.gn_shift = gn_shift; p.gn_silu = silu;
  return launch(pl, p, workspace, (hipStream_t)stream);
}

extern "C" int sdmoe_groupnorm_apply(const void* X, long ldx, int nimg, int HW, int C, const float* scale,
                                     const float* shift, int silu, void* Y, long ldy, void* stream) {
  if (!X || !Y || !scale || !shift || nimg <= 0 || HW <= 0 || C <= 0) return SDMOE_EARG;
  if (C % 8 || ldx % 8 || ldy % 8) return SDMOE_ESHAPE;
  const long rows = (long)nimg * HW;
  gn_apply_kernel<<<grid_for(rows * (C / 8)), 256, 0, (hipStream_t)stream>>>(
      (const half_t*)X, ldx, HW, C, scale, shift, silu, (half_t*)Y, ldy, rows);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_wmask_kmajor(const void* bits, long ldb, int N, int K, const int* perm, void* out, void* stream) {
  if (N == 0) return SDMOE_OK;
  if (!bits || !out || N < 0 || K <= 0) return SDMOE_EARG;
  if (K % 64 || ldb < K / 8) return SDMOE_ESHAPE;
  wmask_kmajor_kernel<<<grid_for((long)(K / 64) * N), 256, 0, (hipStream_t)stream>>>(
      (const uint8_t*)bits, ldb, N, K, perm, (unsigned long long*)out);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_mask_weight(const void* W, const void* bits, long N, long K, void* Wm, void* stream) {
  if (!W || !bits || !Wm || N <= 0 || K <= 0) return SDMOE_EARG;
  if (K % 8) return SDMOE_ESHAPE;
  const long n8 = N * K / 8;
  mask_weight_kernel<<<grid_for(n8), 256, 0, (hipStream_t)stream>>>((const half_t*)W, (const uint8_t*)bits,
                                                                   (half_t*)Wm, n8);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
