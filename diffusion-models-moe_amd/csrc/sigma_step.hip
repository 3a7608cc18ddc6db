// Sigma-parameterised scheduler steps for gfx950: EulerDiscreteScheduler and DPM-Solver++ 2M (midpoint), each with
// prediction_type "epsilon" or "v_prediction", as ONE per-element form whose six coefficients the host computes per
// step (pipeline.euler_schedule / pipeline.dpmpp_2m_schedule):
//   m       = CFG(model_out)                    eu + g * (ec - eu), as cfg_ddim_kernel / cfg_multistep_kernel
//   x0      = cx * x + cm * m                   model output -> denoised sample (epsilon or v)
//   x'      = a * x + b0 * x0 + b1 * prev_x0    the b1 term only when use_prev (DPM++ second order)
//   prev_x0 = x0                                only when store_prev
//   next_in = fp16(x' * in_scale)               scale_model_input of the next step, both CFG copies
// and the matching first-input kernel (latents * init_noise_sigma, then scale_model_input of step 0).
// Plain streaming kernels: the layouts, the half4 accesses and the grid-stride loop of misc.hip's step kernels; no
// LDS, no atomics.
#include "common.h"
#include "../../include/sdmoe.h"

namespace {

struct X0Coef {
  float cx, cm, a, b0, b1, in_scale;
  int use_prev, store_prev;
};

// Order within an element (include/sdmoe.h): read x (and prev_x0 when use_prev) -> x0 -> x' -> store prev_x0 (when
// store_prev) -> lat -> next_in. prev_x0 is never read when use_prev == 0, so a buffer the schedule has not written
// yet (whatever it holds) cannot reach lat.
__global__ void cfg_x0_kernel(const half_t* __restrict__ eps, long lde, float* __restrict__ lat, int B, int HW,
                              int do_cfg, float guidance, float* __restrict__ prev_x0, X0Coef k,
                              half_t* __restrict__ next_in, long ldn) {
  const long n = (long)B * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW), p = (int)(i % HW);
    half4 eu = *reinterpret_cast<const half4*>(eps + ((long)b * HW + p) * lde);
    half4 ec = eu;
    if (do_cfg) ec = *reinterpret_cast<const half4*>(eps + ((long)(B + b) * HW + p) * lde);
    half4 nx;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float m = do_cfg ? (float)eu[c] + guidance * ((float)ec[c] - (float)eu[c]) : (float)eu[c];
      const long li = ((long)b * 4 + c) * HW + p;
      const float x = lat[li];
      const float x0 = k.cx * x + k.cm * m;
      float xp = k.a * x + k.b0 * x0;
      if (k.use_prev) xp += k.b1 * prev_x0[li];
      if (k.store_prev) prev_x0[li] = x0;
      lat[li] = xp;
      nx[c] = (half_t)(xp * k.in_scale);
    }
    if (next_in) {
      *reinterpret_cast<half4*>(next_in + ((long)b * HW + p) * ldn) = nx;
      if (do_cfg) *reinterpret_cast<half4*>(next_in + ((long)(B + b) * HW + p) * ldn) = nx;
    }
  }
}

// lat *= lat_scale in place (fp32), then out = fp16(lat * in_scale) for every copy. One thread owns a pixel of one
// image and writes all its copies, so the in-place product is taken once however many copies there are. Two separately
// rounded fp32 products, then the fp16 rounding. The empty statement on y is common.h's register barrier (gelu_tab_h):
// it holds no instruction, it only keeps the compiler from selecting v_fma_mixlo_f16 for the product and its
// conversion (x * in_scale + 0 rounded to fp16, which turns -0 * 1 into +0: not sdmoe_prepare_input's bits, and
// `#pragma clang fp contract(off)` does not stop that selection).
__global__ void prepare_input_scaled_kernel(float* __restrict__ lat, half_t* __restrict__ out, int B, int HW, long ldo,
                                            int ncopy, float lat_scale, float in_scale) {
  const long n = (long)B * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW), p = (int)(i % HW);
    half4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long li = ((long)b * 4 + c) * HW + p;
      const float x = lat[li] * lat_scale;
      lat[li] = x;
      float y = x * in_scale;
      asm volatile("" : "+v"(y));  // round to fp32 first
      v[c] = (half_t)y;
    }
    for (int k = 0; k < ncopy; ++k) *reinterpret_cast<half4*>(out + ((long)k * n + i) * ldo) = v;
  }
}

int grid_for(long n) {
  long g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" int sdmoe_cfg_x0_step(const void* eps, long lde, float* lat, int B, int HW, int do_cfg, float guidance,
                                 float* prev_x0, const float* coef, const int* flags, void* next_in, long ldn,
                                 void* stream) {
  if (!eps || !lat || !coef || !flags || B <= 0 || HW <= 0) return SDMOE_EARG;
  if (lde % 4 || (next_in && ldn % 4)) return SDMOE_ESHAPE;
  X0Coef k;
  k.cx = coef[0];
  k.cm = coef[1];
  k.a = coef[2];
  k.b0 = coef[3];
  k.b1 = coef[4];
  k.in_scale = coef[5];
  k.use_prev = flags[0] != 0;
  k.store_prev = flags[1] != 0;
  if (!prev_x0 && (k.use_prev || k.store_prev)) return SDMOE_EARG;
  cfg_x0_kernel<<<grid_for((long)B * HW), 256, 0, (hipStream_t)stream>>>((const half_t*)eps, lde, lat, B, HW, do_cfg,
                                                                         guidance, prev_x0, k, (half_t*)next_in, ldn);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}

extern "C" int sdmoe_prepare_input_scaled(float* lat, void* out, int B, int HW, long ldo, int ncopy, float lat_scale,
                                          float in_scale, void* stream) {
  if (!lat || !out || B <= 0 || HW <= 0 || ncopy <= 0) return SDMOE_EARG;
  if (ldo % 4) return SDMOE_ESHAPE;
  prepare_input_scaled_kernel<<<grid_for((long)B * HW), 256, 0, (hipStream_t)stream>>>(lat, (half_t*)out, B, HW, ldo,
                                                                                       ncopy, lat_scale, in_scale);
  SDMOE_CHECK_LAUNCH();
  return SDMOE_OK;
}
