/*
 * sdmoe.h — C ABI of libsdmoe_hip.so, the MI355X (gfx950) kernels behind the MoE-fied Stable-Diffusion
 * denoising step of ruchikachavhan/diffusion-models-moe.
 *
 * Conventions (every entry point):
 *   - plain device pointers (fp16 = IEEE binary16, fp32, int32) and sizes; no framework types;
 *   - activations are row-major [rows, channels] with an explicit row stride `ld*` in ELEMENTS, so a
 *     channel slice of a wider buffer (zero-copy skip concatenation, fused QKV) is passed as (ptr, ld);
 *     spatial tensors are NHWC, i.e. [images * H * W, C];
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); every call is asynchronous,
 *     allocates nothing, never synchronises and is safe under hipGraph stream capture;
 *   - return 0 on success, >0 a hipError_t from the launch, <0 an argument error:
 *     -1 bad pointer/size, -2 unsupported shape/alignment, -3 unsupported mode;
 *   - an empty problem (zero rows / images / sequences) is a no-op that returns 0 before any pointer is checked
 *     (an empty framework tensor may carry a NULL data pointer).
 *   The library neither frees nor retains caller buffers.
 */
#ifndef SDMOE_H
#define SDMOE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Activation codes for `act` arguments. */
#define SDMOE_ACT_NONE 0
#define SDMOE_ACT_SILU 1
#define SDMOE_ACT_GELU 2 /* exact erf GELU, diffusers GEGLU.gelu / F.gelu */
#define SDMOE_ACT_RELU 3 /* relufied U-Net, sparsity/relufy_model.py:8-15 */
#define SDMOE_ACT_QUICK_GELU 4 /* x*sigmoid(1.702x), CLIP ViT-L text encoder MLP (transformers ACT2FN['quick_gelu']) */

const char* sdmoe_version(void);

/*
 * C[m, n] = act( sum_k A[m, k] * W[n, k] + bias[n] + coladd[m / rows_per_batch][n] ) + R[m, n]
 * W is nn.Linear layout [N, K]. workspace (optional, fp32, workspace_floats elements) enables split-K for
 * small tile grids; pass NULL/0 to disable.
 * Replaces: torch.nn.Linear / LoRACompatibleLinear.forward on the U-Net hot path (diffusers, external), the
 * GEGLU projection recomputed by MOEFy.hook_fn (neuron_receivers/moefy.py:12) and RemoveExperts.hook_fn
 * (neuron_receivers/remove_skilled_experts.py:26), and F.linear(x, W*(1-M), b) of
 * WandaRemoveNeuronsFast.linear_hook_fn (neuron_receivers/remove_wanda_neurons_fast.py:76, with
 * sdmoe_mask_weight). Requires K % 64 == 0, N % 8 == 0, strides % 8 == 0.
 */
int sdmoe_linear(const void* A, long lda, const void* W, long ldw, const void* bias, const void* coladd,
                 long coladd_bstride, int rows_per_batch, const void* R, long ldr, void* C, long ldc, int M, int N,
                 int K, int act, float* workspace, long workspace_floats, void* stream);

/*
 * 3x3 convolution, padding 1, on NHWC X [nimg, H, W, Cin] (pixel stride ldx): stride 1 or 2, or a fused
 * nearest-neighbour 2x upsample in front (upsample=1, output 2H x 2W). Weights [Cout][Cin/64][3][3][64]
 * (torch [Cout, Cin, 3, 3] -> permute(0, 2, 3, 1) -> [Cout, 9, Cin/64, 64] -> [Cout, Cin/64, 9, 64]).
 * Same fused epilogue as sdmoe_linear (bias, per-image coladd = time embedding, activation, residual R).
 * Replaces: diffusers ResnetBlock2D conv1/conv2 (+temb add/residual), Downsample2D, Upsample2D,
 * conv_in/conv_out of UNet2DConditionModel (external). Requires Cin % 64 == 0, Cout % 8 == 0.
 */
int sdmoe_conv3x3(const void* X, long ldx, int nimg, int H, int W, int Cin, const void* Wt, const void* bias,
                  const void* coladd, long coladd_bstride, const void* R, long ldr, void* Y, long ldy, int Cout,
                  int stride, int upsample, int act, float* workspace, long workspace_floats, void* stream);

/*
 * sdmoe_conv3x3 (stride 1) with a 1x1 projection shortcut folded in as extra K-steps:
 *   Y = conv3x3(X; Wt[:, :9 Cin]) + X2 Wt[:, 9 Cin:]^T + bias + coladd, X2 [nimg*H*W, Cin2] (row stride ldx2).
 * Wt [Cout][9 Cin + Cin2]: the conv weights in the sdmoe_conv3x3 layout followed by the shortcut's [Cout, Cin2]
 * columns; bias = conv2.bias + conv_shortcut.bias. Cin2 % 64 == 0.
 * Replaces: diffusers ResnetBlock2D conv2 + conv_shortcut + the residual add (`output_tensor = input_tensor +
 * hidden_states` with input_tensor = conv_shortcut(input_tensor); external) — no shortcut output is written or re-read.
 */
int sdmoe_conv3x3_sc(const void* X, long ldx, int nimg, int H, int W, int Cin, const void* Wt, const void* bias,
                     const void* coladd, long coladd_bstride, const void* X2, long ldx2, int Cin2, void* Y, long ldy,
                     int Cout, int act, float* workspace, long workspace_floats, void* stream);

/*
 * Y = conv3x3(act(GroupNorm(X))) [+ X2 W_sc^T] (+ bias + coladd + R): the ResNet conv with the GroupNorm(+SiLU)
 * in front of it applied INSIDE the conv (diffusers ResnetBlock2D: conv1(silu(norm1(x))), conv2(silu(norm2(h)))):
 * gn_scale / gn_shift are the per-image, per-channel fp32 affine of sdmoe_groupnorm_stats ([nimg][Cin]); the
 * normalised tensor is never written. Each 32-channel slice of the staged input halo is normalised once in LDS
 * (zero padding stays zero), with sdmoe_groupnorm_apply's arithmetic, so Y equals sdmoe_groupnorm_apply followed by
 * sdmoe_conv3x3 / sdmoe_conv3x3_sc bit for bit. X2 / Cin2: the optional folded 1x1 shortcut (raw input, not
 * normalised; then R must be NULL). Only the halo-tiled shapes take it (W = 64, Cout % 320 == 0, Cin <= 1280):
 * -3 (unsupported) otherwise -- the caller then applies the GroupNorm and calls sdmoe_conv3x3.
 */
int sdmoe_conv3x3_gn(const void* X, long ldx, int nimg, int H, int W, int Cin, const float* gn_scale,
                     const float* gn_shift, int silu, const void* Wt, const void* bias, const void* coladd,
                     long coladd_bstride, const void* R, long ldr, const void* X2, long ldx2, int Cin2, void* Y,
                     long ldy, int Cout, float* workspace, long workspace_floats, void* stream);

/*
 * sdmoe_conv_up2x — the nearest-2x upsample + 3x3 conv (sdmoe_conv3x3 with upsample = 1, no coladd / activation /
 * residual) collapsed to four 2x2 convs on the LOW-resolution image: output pixel (2r + py, 2q + px) reads only input
 * pixels (r + py + a - 1, q + px + c - 1), a, c in {0, 1} (zero outside), so the taps that land on one input pixel
 * have their weights summed ahead of time and the conv runs 4/9 of the MFMA work. X [nimg*H*W, Cin] (pixel stride
 * ldx), Y [nimg*2H*2W, Cout] (row stride ldy), bias [Cout] or NULL.
 * Wc [4][Cout][Cin/64][2][2][64] fp16: phase 2 py + px, then sdmoe_conv3x3's K order (64-channel slice, tap, channel);
 * row a of phase row py sums kh {0} | {1, 2} (py = 0) or {0, 1} | {2} (py = 1), columns likewise (fp32 sums, rounded
 * once: sdmoe/ops.py conv_up2x_weight). An implicit GEMM of M = nimg*H*W, N = 4 Cout, K = 4 Cin on the dense tile
 * rules; every tile lies in one phase: -3 (unsupported) when Cout is no multiple of the chosen tile's columns -- the
 * caller then runs sdmoe_conv3x3. Cin % 64 == 0, Cout % 8 == 0.
 * Replaces: diffusers Upsample2D (F.interpolate(scale_factor=2.0, mode="nearest") + conv; external).
 */
int sdmoe_conv_up2x(const void* X, long ldx, int nimg, int H, int W, int Cin, const void* Wc, const void* bias, void* Y,
                    long ldy, int Cout, float* workspace, long workspace_floats, void* stream);
/* the launch sdmoe_conv_up2x would make: out[0..6] = tile rows, tile columns, waves along M, waves along N, ring
 * stages, split-K factor, 64-deep K-steps per split; -3 where it refuses. Queries the CU count as sdmoe_gemm_plan. */
int sdmoe_conv_up2x_plan(int nimg, int H, int W, int Cin, int Cout, long workspace_floats, int* out);

/* Y = (SiLU?)(X * scale[img, c] + shift[img, c]) on [nimg*HW, C] (the GroupNorm apply; scale/shift from
 * sdmoe_groupnorm_stats). C % 8 == 0. */
int sdmoe_groupnorm_apply(const void* X, long ldx, int nimg, int HW, int C, const float* scale, const float* shift,
                          int silu, void* Y, long ldy, void* stream);

/* Wm = W with every weight whose bit is set in bits [N][K/8] (little-endian bit order) zeroed: the device form
 * of W * (1 - M) (remove_wanda_neurons_fast.py:75, 80). */
int sdmoe_mask_weight(const void* W, const void* bits, long N, long K, void* Wm, void* stream);

/*
 * GroupNorm statistics of X [nimg, HW, C] (row stride ldx) with `groups` groups: writes per (image, channel)
 * scale = rstd*gamma and shift = beta - mean*scale (fp32 [nimg, C]) consumed by sdmoe_groupnorm_apply.
 * workspace: >= nimg*groups*64*2 floats.
 * Replaces: torch.nn.GroupNorm in ResnetBlock2D / Transformer2DModel / conv_norm_out (external).
 */
int sdmoe_groupnorm_stats(const void* X, long ldx, int nimg, int HW, int C, int groups, const void* gamma,
                          const void* beta, float eps, float* scale, float* shift, float* workspace,
                          long workspace_floats, void* stream);

/*
 * GroupNorm (+SiLU) in one call: Y = act(X * scale + shift) with the statistics of sdmoe_groupnorm_stats (scale /
 * shift are written too), i.e. sdmoe_groupnorm_stats followed by sdmoe_groupnorm_apply. Y must not alias X. Same
 * workspace as _stats.
 * Replaces: GroupNorm(+SiLU) in front of ResnetBlock2D conv1/conv2, Transformer2DModel.proj_in, conv_norm_out.
 */
int sdmoe_groupnorm(const void* X, long ldx, int nimg, int HW, int C, int groups, const void* gamma, const void* beta,
                    float eps, int silu, void* Y, long ldy, float* scale, float* shift, float* workspace,
                    long workspace_floats, void* stream);

/*
 * GroupNorm folded into the linear (1x1 conv) that consumes it — Transformer2DModel.norm -> proj_in (diffusers,
 * external): the normalised activation is never written or re-read.
 *  sdmoe_gn_fold (per call, after sdmoe_groupnorm_stats): for each image i, Wf[i][n, k] = fp16(W[n, k] * scale[i, k])
 *    (Wf [nimg][N][K], dense) and colbias[i][n] = bias[n] + sum_k float(Wf[i][n, k]) * (shift[i, k] / scale[i, k])
 *    (fp32 [nimg][N]; bias may be NULL; the term is W[n, k] * shift[i, k] where |scale[i, k]| < 2^-14, e.g. gamma == 0),
 *    so proj_in(GN(x)) = x . Wf[i]^T + colbias[i] on the rows of image i. The bias comes from the ROUNDED weights:
 *    the GEMM then computes sum_k Wf (x + shift / scale), the fp16 rounding of Wf multiplies an activation centred to
 *    within about one std of its group mean, and the fold is as accurate as GroupNorm + linear whatever the group's
 *    |mean| / std (from the unrounded W it left the suite's bar at |mean| / std ~ 16). K % 8 == 0, ldw % 8 == 0.
 *  sdmoe_linear_per_image: C[m, n] = sum_k A[m, k] Wf[m / rows_per_batch][n, k] + colbias[m / rows_per_batch][n]
 *    + R[m, n] (weights of image i at Wf + i * w_bstride elements, row stride ldw; colbias row stride
 *    colbias_bstride). rows_per_batch % 256 == 0 (no GEMM tile straddles two images), K % 64 == 0, N % 8 == 0.
 * Replaces sdmoe_groupnorm + sdmoe_linear of Transformer2DModel (GroupNorm(32, C) -> proj_in).
 */
int sdmoe_gn_fold(const void* W, long ldw, int N, int K, const void* bias, const float* scale, const float* shift,
                  int nimg, void* Wf, float* colbias, void* stream);
int sdmoe_linear_per_image(const void* A, long lda, const void* Wf, long ldw, long w_bstride, const float* colbias,
                           long colbias_bstride, int rows_per_batch, const void* R, long ldr, void* C, long ldc, int M,
                           int N, int K, float* workspace, long workspace_floats, void* stream);

/* LayerNorm over the last dimension (C % 64 == 0, C <= 2048). Replaces BasicTransformerBlock norm1/2/3. */
int sdmoe_layernorm(const void* X, long ldx, void* Y, long ldy, int M, int C, const void* gamma, const void* beta,
                    float eps, void* stream);

/*
 * LayerNorm folded into the GEMM that consumes it (BasicTransformerBlock norm1 -> attn1 QKV, norm2 -> attn2 Q,
 * norm3 -> ff.net.0 GEGLU projection): no normalised activation is written or re-read.
 *  sdmoe_ln_fold (once per weight set): Wf[n, k] = fp16(W[n, k] * gamma[k]) (row stride ldf), wsum[n] = sum_k
 *    Wf[n, k] and bias_f[n] = bias[n] + sum_k W[n, k] * beta[k] (fp32; bias may be NULL).
 *  sdmoe_linear_ln: C[m, n] = rstd_m * (sum_k A[m, k] Wf[n, k] - mean_m * wsum[n]) + bias_f[n]
 *    = LayerNorm(A)[m] . W[n] + bias[n], mean_m / rstd_m = 1 / sqrt(var_m + eps) over the K channels of row m,
 *    accumulated (v_dot2_f32_f16 sums of x and x^2) from the A tiles the GEMM already stages in LDS.
 *  sdmoe_linear_geglu_ln: sdmoe_linear_geglu with the same fold (W / bias_f / wsum interleaved like W and bias).
 * K % 64 == 0 and K = the normalised dimension. Replaces sdmoe_layernorm + sdmoe_linear / sdmoe_linear_geglu
 * (diffusers BasicTransformerBlock.norm1/2/3 + to_q/k/v / GEGLU.proj).
 */
int sdmoe_ln_fold(const void* W, long ldw, int N, int K, const void* gamma, const void* beta, const void* bias,
                  void* Wf, long ldf, float* bias_f, float* wsum, void* stream);
int sdmoe_linear_ln(const void* A, long lda, const void* Wf, long ldw, const float* bias_f, const float* wsum,
                    float eps, void* C, long ldc, int M, int N, int K, void* stream);
int sdmoe_linear_geglu_ln(const void* A, long lda, const void* W, long ldw, const float* bias_f, const float* wsum,
                          float eps, void* P, long ldp, int M, int F, int K, int act, void* score, long ld_score,
                          int esize, void* stream);

/*
 * Scaled-dot-product attention, fp16: O[b, q, h*d:(h+1)*d] = softmax(Q K^T * scale) V per (image b, head h),
 * with Q [nimg*Nq, *] (stride ldq), K/V [nimg*Nk, *] (strides ldk/ldv), head h at column offset h*head_dim.
 * head_dim in {32, 40, 64, 80, 160}.
 * Replaces: diffusers Attention (attn1 self / attn2 cross) + AttnProcessor softmax(QK^T/sqrt(d))V (external;
 * SURVEY §2.3 K10).
 */
int sdmoe_attention(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo,
                    int nimg, int Nq, int Nk, int heads, int head_dim, float scale, void* stream);

/*
 * MoE-fied GEGLU routing over Y = proj(x) [M, 2F] (value | gate halves, row stride ldy), F = 4C inner neurons:
 *   g = act(gate); score[e] = sum_{n: labels[n]==e} g[n]; removed experts score 0; sel = top-k(score) with
 *   ties toward the lowest expert id; keep[n] = sel[labels[n]] && !removed[labels[n]];
 *   out[m, n] = keep ? value*g : 0.
 * labels [F] int32 (0..E-1); e_off [E+1] / e_nid [F]: neurons grouped per expert (ascending neuron id);
 * removed_bits [ceil(E/32)] (bit e => expert e removed) or NULL; E == 0 => dense GEGLU (value * act(gate)).
 * Optional outputs: gate_out [M, F] (the masked gate the reference appends to self.gates), sel_out
 * [M, ceil(E/32)] uint32 top-k bitmask, score_out [M, E] fp16 scores. E <= 256, F % 8 == 0.
 * Replaces: MOEFy.hook_fn (neuron_receivers/moefy.py:10-27) and RemoveExperts.hook_fn
 * (neuron_receivers/remove_skilled_experts.py:24-55) after the projection: gelu, matmul(gate, patterns^T),
 * torch.topk, F.embedding(...).sum(-2), gate[mask==0]=0, hidden_states*gate, gate.cpu().
 */
int sdmoe_geglu_route(const void* Y, long ldy, int M, int F, int E, int k, int act, const int* labels,
                      const int* e_off, const int* e_nid, const unsigned* removed_bits, void* out, long ldo,
                      void* gate_out, long ldg, unsigned* sel_out, void* score_out, void* stream);

/*
 * Per-expert score bias: AddExperts.hook_fn (neuron_receivers/add_skilled_experts.py:35-71), the counterpart of
 * RemoveExperts that pushes a concept's experts INTO every token's top-k. Its one line over MOEFy.hook_fn,
 *   score[:, expert_indx] = score[:, expert_indx] + 5.0 * std[expert_indx]          (:55)
 * is one more rounding point on the fp16 score, between the kernel that produces it and the kernel that ranks it;
 * the reference's k' = int(0.8 * k) (:57) is the run-time k of the existing top-k entry points.
 *   bias [E] fp16: fp16(5.0 * fp16(std[e])) at the listed experts, +0 elsewhere (the host forms it with the
 *   reference's own torch operations: first rounding point). A listed duplicate is applied once.
 *
 *  sdmoe_score_bias: out[m, e] = fp16(score[m, e] + bias[e]) for m < M, e < E (second rounding point: the fp16 + fp16
 *    sum is exact in fp32, so one round-to-nearest-even conversion is the reference's fp16 add). score / out [M, E]
 *    fp16 with row strides ld_score / ld_out >= E; columns >= E of a strided row are neither read nor written.
 *    out == score (in place) is allowed; any other overlap is not. 1 <= E <= 256, any M. 16-byte loads and stores
 *    when E, both strides are multiples of 8 and all three pointers 16-byte aligned, else 2-byte ones. Feeds
 *    sdmoe_moe_topk_keep / sdmoe_moe_topk_mask (fused path: sdmoe_linear_geglu -> sdmoe_score_bias -> top-k at k').
 *  sdmoe_geglu_route_bias: sdmoe_geglu_route with that add inside the kernel (unfused path): after the
 *    removed-expert zeroing, score[e] = fp16(score[e] + bias[e]) before score_out is written and before the top-k
 *    ranks it. bias == NULL: bit-identical to sdmoe_geglu_route (which is this entry point with bias NULL).
 */
int sdmoe_score_bias(const void* score, long ld_score, int M, int E, const void* bias, void* out, long ld_out,
                     void* stream);
int sdmoe_geglu_route_bias(const void* Y, long ldy, int M, int F, int E, int k, int act, const int* labels,
                           const int* e_off, const int* e_nid, const unsigned* removed_bits, void* out, long ldo,
                           void* gate_out, long ldg, unsigned* sel_out, void* score_out, const void* bias,
                           void* stream);

/*
 * Fused form of the same routing for balanced experts (the reference's KMeansConstrained split: every expert
 * has esize neurons, esize | 40), in two launches and without the [M, 2F] projection output:
 *  1. sdmoe_linear_geglu: P[m, n] = fp16(fp16(x W_v^T + b_v) * fp16(act(fp16(x W_g^T + b_g)))) for all F neurons
 *     and score[m, e] = fp16(sum over expert e's neurons of act(gate)) in the GEMM epilogue. W [2F, K] / bias
 *     [2F] hold the neurons permuted so every expert is contiguous (expert-major, ascending neuron id), value
 *     and gate rows interleaved in pairs ([v 2 | g 2] per neuron pair, sdmoe/ops.py geglu_rows). F % 80 == 0. score
 *     may be NULL
 *     (dense GEGLU). Same rounding points as sdmoe_linear + sdmoe_geglu_route.
 *  2. sdmoe_moe_topk_mask: per token, removed experts score 0, top-k (ties toward the lowest expert id) and
 *     zero every neuron of P whose expert is not selected or removed. sel_out as above (may be NULL).
 * The permuted P feeds the down projection with W_down's columns permuted the same way.
 * Replaces: the same reference hooks as sdmoe_geglu_route (moefy.py:10-27, remove_skilled_experts.py:24-55),
 * with SURVEY §3 K1+K2+K3 fused into the projection GEMM.
 */
int sdmoe_linear_geglu(const void* A, long lda, const void* W, long ldw, const void* bias, void* P, long ldp,
                       int M, int F, int K, int act, void* score, long ld_score, int esize, void* stream);
int sdmoe_moe_topk_mask(void* P, long ldp, int M, int F, int E, int esize, int k, const void* score,
                        long ld_score, const unsigned* removed_bits, unsigned* sel_out, void* stream);

/*
 * The same routing with the mask moved into the FFN down projection (ff.net.2) instead of a pass over P:
 *  sdmoe_moe_topk_keep: the selection of sdmoe_moe_topk_mask (removed experts score 0, top-k, ties toward the
 *    lowest id) written as keep bits of the expert-major permuted neurons: keep [F/64][M] 64-bit words, bit j of
 *    word (s, m) = neuron 64 s + j of token m is kept (selected and not removed). P is not touched. F % 64 == 0.
 *  sdmoe_linear_keep: C = (A with every dropped neuron zeroed) @ W^T + bias + R, the zeroing applied to the A
 *    fragments after their LDS read, so the result is bit-identical to sdmoe_moe_topk_mask followed by
 *    sdmoe_linear. A [M, K] (K = F), keep as above, W [N, K]. K % 64 == 0.
 * Replaces: gate[cur_mask == 0] = 0 and hidden_states * gate of MOEFy / RemoveExperts.hook_fn (moefy.py:23-26,
 * remove_skilled_experts.py:49-55) feeding ff.net.2 (diffusers FeedForward), without a pass over the product.
 */
int sdmoe_moe_topk_keep(int M, int F, int E, int esize, int k, const void* score, long ld_score,
                        const unsigned* removed_bits, void* keep, unsigned* sel_out, void* stream);
int sdmoe_linear_keep(const void* A, long lda, const void* keep, const void* W, long ldw, const void* bias,
                      const void* R, long ldr, void* C, long ldc, int M, int N, int K, float* workspace,
                      long workspace_floats, void* stream);

/*
 * sdmoe_linear_masked — SURVEY §8b's masked linear: C = (A ⊙ keep) @ (W ⊙ (1 - M))^T + bias + R with both masks
 * applied to the MFMA fragments after their LDS read (no masked copy of A or W is ever written):
 *   keep  (nullable): the A operand's per-(row, k) keep bits, layout of sdmoe_moe_topk_keep ([K/64][M] 64-bit words);
 *   wmask (nullable): the Wanda weight mask in the same K-step-major layout over W's rows ([K/64][N] 64-bit words,
 *     bit j of word (s, n) SET = W[n, 64 s + j] removed), made once per mask by sdmoe_wmask_kmajor.
 * Both NULL = sdmoe_linear without coladd/act. K % 64 == 0, N % 8 == 0, strides % 8 == 0.
 * Replaces: F.linear(input[0], W.clone() * (1 - M[t][l]), b) of WandaRemoveNeuronsFast.linear_hook_fn
 * (neuron_receivers/remove_wanda_neurons_fast.py:69-83) -- no W clone, no mask H2D copy, no second GEMM -- and,
 * with keep, that hook under MoE routing (the union remover of multi_concept_remover.py:43-53 on a MoE-fied U-Net,
 * BASELINE config 4).
 */
int sdmoe_linear_masked(const void* A, long lda, const void* keep, const void* W, long ldw, const void* wmask,
                        const void* bias, const void* R, long ldr, void* C, long ldc, int M, int N, int K,
                        float* workspace, long workspace_floats, void* stream);

/*
 * sdmoe_linear_masked_sets — sdmoe_linear_masked with one Wanda mask per image of the call:
 *   C[m] = (A[m] ⊙ keep[m]) @ (W ⊙ (1 - Mask[image_set[m / rows_per_img]]))^T + bias + R[m].
 *   wmasks: nsets masks in sdmoe_wmask_kmajor's layout ([K/64][N] 64-bit words each), set s at wmasks + s * set_stride
 *     words (set_stride >= K/64 * N); an all-zero set is the unmasked product;
 *   image_set: device int32 [M / rows_per_img], 0 <= image_set[i] < nsets (the caller's guarantee: the kernel does
 *     not range-check it); keep nullable as in sdmoe_linear_masked. M % rows_per_img == 0.
 * One launch at the full grid: every row tile reads its image's set id (one scalar load per workgroup) and stages its
 * mask bytes from that set. No tile straddles two images: the launch is sdmoe_linear_masked's own plan where that
 * tile's rows divide rows_per_img -- then a uniform image_set gives sdmoe_linear_masked's bits -- else a 64-row tile
 * with the split-K policy applied to that tile (SD-1.4 / SDXL: only the mid block, rows_per_img = 64); SDMOE_EUNSUP
 * when rows_per_img % 64 != 0 (the caller then runs sdmoe_linear_masked per run of images, sdmoe/ops.py).
 * Replaces: the one-prompt-per-call loop of benchmarks/unified_editing.py:106-126, where every prompt goes through
 * MultiConceptRemoverWanda.remove_concepts (neuron_receivers/multi_concept_remover.py:55-99) with its own concept
 * list, i.e. its own F.linear(input[0], W.clone() * (1 - M[t][l]), b) (remove_wanda_neurons_fast.py:69-83).
 */
int sdmoe_linear_masked_sets(const void* A, long lda, const void* keep, const void* W, long ldw, const void* wmasks,
                             long set_stride, const int* image_set, int nsets, int rows_per_img, const void* bias,
                             const void* R, long ldr, void* C, long ldc, int M, int N, int K, float* workspace,
                             long workspace_floats, void* stream);

/*
 * sdmoe_gemm_plan_sets — sdmoe_gemm_plan for sdmoe_linear_masked_sets (has_keep: with the A keep bits): out[0..4] as
 * there; out[0] divides rows_per_img. SDMOE_EUNSUP exactly where the launch would refuse (rows_per_img % 64 != 0 and
 * the shape's own tile does not divide it).
 */
int sdmoe_gemm_plan_sets(int has_keep, int M, int N, int K, int rows_per_img, int has_residual, long workspace_floats,
                         int* out);

/*
 * sdmoe_wmask_union_sets — the masks of sdmoe_linear_masked_sets from per-concept masks, one streaming launch for all
 * sets of a (t, l): out[s * words + w] = OR over the concepts c with bit c of select[s] set of
 * masks[c * mask_stride + w] (64-bit words; select: device uint32 [nsets], nconcepts <= 32, bits past nconcepts
 * ignored; mask_stride >= words). select[s] == 0 gives the all-zero (unmasked) set.
 * Replaces: MultiConceptRemoverWanda.handle_multiple_concepts (multi_concept_remover.py:43-53), the host-side
 * element-wise OR over every (t, l) mask per request -- here exactly the listed concepts, per prompt, on the device.
 */
int sdmoe_wmask_union_sets(const void* masks, long mask_stride, int nconcepts, const unsigned* select, int nsets,
                           long words, void* out, void* stream);

/*
 * sdmoe_gemm_plan — query (no device memory, no launch): the launch sdmoe_linear (mode 0), sdmoe_linear_masked
 * with keep (4), wmask (5) or both (6), or sdmoe_linear_ln (7) would make for an M x N x K product with / without a
 * residual and activation act, given workspace_floats of split-K workspace (0 = none), or sdmoe_linear_geglu (3; 15 =
 * with the registered GELU table) / sdmoe_linear_geglu_ln (8) for M x 2F x K (pass N = 2F):
 * out[0..4] = tile rows, tile columns, waves along M, waves along N, split-K factor. Masked modes take the plain
 * GEMM's plan (its split, hence each output's fp32 summation order), so sdmoe_linear_masked is bit-identical to
 * masking A / W first and calling sdmoe_linear; the tests check that over every U-Net shape. Splits depend on the
 * current device's CU count: the call queries it, which starts the HIP runtime (256, the MI355X's count, is assumed
 * while no device answers, so the query also works on a host without a GPU).
 */
int sdmoe_gemm_plan(int mode, int M, int N, int K, int has_residual, int act, long workspace_floats, int* out);

/*
 * sdmoe_conv_plan — the same query for the 3x3 convs: the launch sdmoe_conv3x3 (Cin2 = 0), sdmoe_conv3x3_sc
 * (Cin2 > 0: the folded shortcut's channels; stride 1, no upsample, no residual) or, with gn = 1, sdmoe_conv3x3_gn
 * would make for nimg H x W x Cin images: out[0..9] = halo tiles (1) or shifted tiles (0), tile rows, tile columns,
 * waves along M, waves along N, K depth of one LDS ring stage, ring stages, split-K factor, K units per split
 * (64-deep K-steps; halo: 32-channel slices of the main input), folded-shortcut K-steps per split (halo only).
 * SDMOE_EUNSUP for gn = 1 on a shape sdmoe_conv3x3_gn refuses. Queries the CU count as sdmoe_gemm_plan does.
 */
int sdmoe_conv_plan(int nimg, int H, int W, int Cin, int Cin2, int Cout, int stride, int upsample, int has_residual,
                    int gn, int act, long workspace_floats, int* out);

/*
 * sdmoe_wmask_kmajor — packed Wanda bits [N][K/8] (row stride ldb bytes; bit k%8 of byte (n, k/8) = W[n, k] removed;
 * the layout of the reference's [C, 4C] masks bit-packed, sdmoe/mask_io.py) -> out [K/64][N] 64-bit words for
 * sdmoe_linear_masked. perm (nullable, int32 [K]) permutes the columns: bit j of word (s, n) = mask(n, perm[64 s + j])
 * -- the FFN down projection's expert-major neuron order of the fused routed path. K % 64 == 0.
 */
int sdmoe_wmask_kmajor(const void* bits, long ldb, int N, int K, const int* perm, void* out, void* stream);

/*
 * Skill discovery on the same hook seam.
 * sdmoe_expert_mean_topk — GetExperts.hook_fn (neuron_receivers/get_experts.py:50-83): mean over tokens of the
 *   fp16 expert scores [M, E] (score_within_bb.mean(0): fp32 accumulate, one rounding to fp16), restricted to the
 *   bounding-box positions row_idx[0..n_idx) of every rows_per_img-row image when row_idx != NULL, then the k
 *   best experts (descending; ties toward the lowest id) into topk_out[k]; mean_out (fp16 [E]) optional.
 *   E <= 1024. workspace >= ceil(selected rows / 256) * E floats.
 * sdmoe_colnorm_accum — Wanda.hook_fn (neuron_receivers/wanda_receiver.py:37-57) + ColumnNormCalculator
 *   (utils.py:321-341): sumsq[f] += sum_m (P[m,f] / max(||P[m,:]||_2, 1e-12))^2 (the squared running column
 *   norm). workspace >= M + ceil(M / 256) * F floats.
 * sdmoe_wanda_mask — modularity/wanda.py:140-160: per row n of the down projection W [C, F], metric = fp16(|W| *
 *   norm) for the base and adjusted prompts (fp16 norms [F]); bit (n, f) = f among the kprune largest adjusted
 *   metrics of the row (ties toward the lowest column) AND metric_adj > metric_base. bits [C, F/8], the
 *   bit-packed layout WandaRemoveNeuronsFast consumes. F % 8 == 0, F <= 8192.
 */
int sdmoe_expert_mean_topk(const void* score, long ld_score, int M, int E, int rows_per_img, const int* row_idx,
                           int n_idx, int k, void* mean_out, int* topk_out, float* workspace, long workspace_floats,
                           void* stream);
/*
 * sdmoe_expert_stats — the expert-level statistics of ExpertPredictivity.hook_fn (neuron_receivers/
 * expert_activation.py:51-59) and FrequencyMeasure.hook_fn (neuron_receivers/frequency_measure.py:53-57) as one
 * streaming pass over what the routing kernels already produce: score [M, E] fp16 (row stride ld_score) and sel
 * [M, ceil(E / 32)] uint32 words, bit e % 32 of word e / 32 = expert e among the token's top-k (the sel_out of
 * sdmoe_geglu_route, sdmoe_moe_topk_mask and sdmoe_moe_topk_keep; nullable).
 *   colmax (nullable, fp16 [ngroups, E]): colmax[g][e] = max of score[m][e] over every row of every image i with
 *     img_group[i] == g (image i = rows [i * rows_per_img, (i + 1) * rows_per_img); img_group NULL = one group;
 *     rows_per_img 0 = one image of M rows) -- torch.max(score, dim=0). The maximum starts from -inf (a GELU expert's
 *     score can be negative on every row); a group without an image gets -inf.
 *   count (nullable, int32 [M / rows_per_img, E]): count[i][e] = rows of image i whose sel bit e is set; bits at or
 *     above E in the last word are ignored. count without sel is SDMOE_EARG.
 * No atomics: deterministic. E <= 256 (SDMOE_ESHAPE); M == 0 is a no-op; M % rows_per_img == 0 (SDMOE_EARG).
 * workspace >= c * [count != NULL] + ceil(c / 2) * [colmax != NULL] floats, c = (M / rows_per_img) *
 * ceil(rows_per_img / 16) * E (SDMOE_ESHAPE).
 */
int sdmoe_expert_stats(const void* score, long ld_score, const unsigned* sel, int M, int E, int rows_per_img,
                       const int* img_group, int ngroups, void* colmax, int* count, float* workspace,
                       long workspace_floats, void* stream);
int sdmoe_colnorm_accum(const void* P, long ldp, int M, int F, float* sumsq, float* workspace, long workspace_floats,
                        void* stream);
int sdmoe_wanda_mask(const void* W, long ldw, int C, int F, const void* norm_base, const void* norm_adj, int kprune,
                     void* bits, void* stream);

/*
 * sdmoe_geglu_neurons — the neuron-level path: NeuronPredictivity / NeuronPredictivityBB.hook_fn
 * (neuron_receivers/predictivity.py:42-53, neuron_predictivity_bb.py:43-63) and RemoveNeurons.hook_fn
 * (neuron_receivers/remove_skilled_neurons.py:26-42) as one streaming pass over Y = proj(x) = [value | gate]
 * [M, 2F] (row stride ldy):
 *   g   = fp16(act(gate))                  the activation of sdmoe_geglu_route (the registered GELU table, else erf)
 *   g'  = override bit n set ? fp16(override_value) : g      override_bits [F/32] words, bit n % 32 of word n / 32;
 *                                                            NULL = no override
 *   out = fp16(float(value) * float(g'))   [M, F] (ldo); gate_out (nullable, ldg) = g'
 *   colmax (nullable, fp16 [ngroups, F]): colmax[img_group[i]][n] = max of g (BEFORE the override) over the rows of
 *     image i = rows [i * rows_per_img, (i + 1) * rows_per_img) whose position has its bit set in pos_bits
 *     [ceil(rows_per_img / 32)] (NULL = every position); img_group NULL = every image in group 0; rows_per_img 0 =
 *     one image of M rows. A group without a selected row gets -inf. No atomics: deterministic.
 * With override_bits == NULL and colmax == NULL, out is bit-identical to sdmoe_geglu_route(E = 0).
 * F % 32 == 0, ldy % 8 == 0 (SDMOE_ESHAPE); M % rows_per_img == 0 (SDMOE_EARG).
 * workspace (used for colmax only) >= (M / rows_per_img) * ceil(rows_per_img / 64) * F / 2 floats.
 */
int sdmoe_geglu_neurons(const void* Y, long ldy, int M, int F, int act, const unsigned* override_bits,
                        float override_value, void* out, long ldo, void* gate_out, long ldg, int rows_per_img,
                        const int* img_group, int ngroups, const unsigned* pos_bits, void* colmax, float* workspace,
                        long workspace_floats, void* stream);

/*
 * sdmoe_geglu_sparsity — the gate-sparsity measurement: SparsityMeasure.hook_fn / .test (neuron_receivers/
 * sparsity_measure.py:13-18, :39-41) and the per-call count of sparsity/check_sparsity.py:41-46 as one streaming pass
 * over Y = proj(x) = [value | gate] [M, 2F] (row stride ldy), in place of a host copy of every activated gate:
 *   g   = fp16(act(gate))                  the activation of sdmoe_geglu_neurons (the registered GELU table, else erf)
 *   out = fp16(float(value) * float(g))    [M, F] (ldo), bit-identical to sdmoe_geglu_neurons without an override;
 *                                          gate_out (nullable, ldg) = g
 *   col_zero (nullable, int32 [ngroups, F]): col_zero[img_group[i]][n] = rows of image i = rows [i * rows_per_img,
 *     (i + 1) * rows_per_img) with |float(g)| <= threshold (fp32 compare; threshold 0 counts +0 and -0: `gate == 0.0`);
 *     img_group NULL = every image in group 0; rows_per_img 0 = one image of M rows; a group without an image gets 0
 *   col_neg (nullable, int32 [ngroups, F]): the rows with float(g) < 0 (-0 is not counted: `gate >= 0` holds for it)
 *   totals (nullable, int64 [ngroups, 2]): {sum_n col_zero[g][n], sum_n col_neg[g][n]}
 * col_zero and col_neg may be NULL when totals is given; totals may be NULL when both arrays are given (else
 * SDMOE_EARG). Every output is written in full by each call (no buffer is assumed zeroed); integer sums only, so the
 * results do not depend on the order of the blocks. threshold >= 0 (SDMOE_EARG); M == 0 is a no-op.
 * F % 32 == 0, ldy % 8 == 0 (SDMOE_ESHAPE); M % rows_per_img == 0 (SDMOE_EARG).
 * workspace >= (M / rows_per_img) * ceil(rows_per_img / 64) * F floats (SDMOE_ESHAPE).
 */
int sdmoe_geglu_sparsity(const void* Y, long ldy, int M, int F, int act, float threshold, void* out, long ldo,
                         void* gate_out, long ldg, int rows_per_img, const int* img_group, int ngroups, int* col_zero,
                         int* col_neg, int64_t* totals, float* workspace, long workspace_floats, void* stream);

/*
 * Offline MoE-fication: ParamSplit.split (moefication/moe_utils.py:97-107) clusters the
 * L2-normalised gate rows of each GEGLU with KMeansConstrained(size_min = size_max = expert_size).
 * sdmoe_sqdist_f32 — D[i][c] = max(|x_i|^2 + |c_c|^2 - 2 x_i.c_c, 0), fp32 device arrays (exact fp32 MFMA
 *   dot products); X [n, d] (ld ldx), C [k, d] (ld ldc), D [n, k] (ld ldd).
 * sdmoe_balanced_assign — HOST function: labels[n] minimising sum cost[i][labels[i]] subject to every cluster
 *   holding exactly n/k points (the min-cost flow of k_means_constrained); cost [n, k] host doubles >= 0.
 *   Epsilon-scaling auction on integer costs (cost * scale; scale 0 = auto), exact for the integer costs.
 *   prices [n] (int64, optional) carries the slot prices across calls: warm = 1 starts from them.
 */
int sdmoe_sqdist_f32(const float* X, long ldx, const float* C, long ldc, int n, int k, int d, float* D, long ldd,
                     void* stream);
int sdmoe_balanced_assign(const double* cost, int n, int k, double scale, int64_t* prices, int warm, int* labels);

/*
 * Static "union-timesteps" mask (benchmarks/save_union_over_time.py:189-207): out bit =
 * (number of the T per-timestep Wanda masks with that bit set) > threshold, threshold = select_ratio * timesteps.
 * bits: T bit-packed masks of nbytes each (mask t at bits + t * t_stride_bytes, the [C, F/8] layout of
 * sdmoe_mask_weight); out: nbytes. Baking the result into ff.net.2 (W * (1 - M), :214-221) is sdmoe_mask_weight
 * with Wm = W. nbytes % 4 == 0.
 */
int sdmoe_union_over_time(const void* bits, long t_stride_bytes, int T, long nbytes, float threshold, void* out,
                          void* stream);

/*
 * VAE decoder helpers (diffusers AutoencoderKL.decode, external): the decoder mid-block's
 * single 512-wide attention head runs as sdmoe_linear (S = Q K^T) -> sdmoe_softmax_rows -> sdmoe_linear (O = P V,
 * with V^T from sdmoe_transpose).
 * sdmoe_softmax_rows — Y[r, :] = softmax(X[r, :]) for R rows of N (fp16, fp32 math; N % 8 == 0, N <= 8192).
 * sdmoe_transpose — Y [C, R] = X [R, C]^T, fp16, any leading dimensions.
 */
int sdmoe_softmax_rows(const void* X, long ldx, void* Y, long ldy, int R, int N, void* stream);
int sdmoe_transpose(const void* X, long ldx, void* Y, long ldy, int R, int C, void* stream);

/*
 * CLIP text encoder helpers (transformers CLIPTextModel, external — the pipelines' text_encoder
 * and the reference's hook_module='text' seam, base_receiver.py:59-65, remove_wanda_neurons_fast.py:114-120).
 * sdmoe_gather_rows — out[r, :C] = table[idx[r], :C] (+ add[r % period, :C] when add != NULL), fp16, C % 8 == 0.
 *   Replaces CLIPTextEmbeddings (token_embedding(ids) + position_embedding(arange)) and the pooled-output gather
 *   last_hidden_state[arange(B), eos_position].
 * sdmoe_attention_short — O = softmax(Q K^T * scale [+ causal mask]) V per (sequence, head) for N <= 128 tokens,
 *   head_dim <= 128 (% 8); same operand layout as sdmoe_attention. Replaces CLIPAttention with the causal mask of
 *   CLIPTextTransformer (_create_4d_causal_attention_mask).
 */
int sdmoe_gather_rows(const void* table, long ld_table, const int* idx, int R, int C, const void* add, long ld_add,
                      int period, void* out, long ld_out, void* stream);
int sdmoe_attention_short(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O,
                          long ldo, int nseq, int N, int heads, int head_dim, float scale, int causal, void* stream);

/* diffusers get_timestep_embedding for one timestep (t_dev if non-NULL, else t), fp16 [dim]. */
int sdmoe_timestep_embedding(void* out, const float* t_dev, float t, int dim, int flip_sin_to_cos, float freq_shift,
                             void* stream);
/* n timestep embeddings (t_dev[0..n)), row r written at out + (r/group)*ldo + (r%group)*dim: SDXL's add_time_proj
 * over the 6 micro-conditioning time ids per image (diffusers UNet2DConditionModel.get_aug_embed, "text_time";
 * the reference loads SDXL at utils.py:111-112). */
int sdmoe_timestep_embedding_rows(void* out, long ldo, const float* t_dev, int n, int group, int dim,
                                  int flip_sin_to_cos, float freq_shift, void* stream);

/* latents fp32 NCHW [B,4,H,W] -> U-Net input fp16 NHWC [ncopy*B, HW, ldo] channels 0..3 (CFG copies). */
int sdmoe_prepare_input(const float* lat, void* out, int B, int HW, long ldo, int ncopy, void* stream);

/*
 * Classifier-free guidance + DDIM (eta = 0) update of fp32 NCHW latents in place from eps fp16
 * [ncopy*B, HW, lde] (uncond first); optionally writes the next fp16 U-Net input (both CFG copies).
 * Replaces StableDiffusionPipeline's CFG combine + DDIMScheduler.step (external).
 */
int sdmoe_cfg_ddim_step(const void* eps, long lde, float* lat, int B, int HW, int do_cfg, float guidance,
                        float alpha_t, float alpha_prev, void* next_in, long ldn, void* stream);

/*
 * Classifier-free guidance + one linear multistep update of fp32 NCHW latents in place: the PLMS step of
 * diffusers' PNDMScheduler (skip_prk_steps, prediction_type "epsilon"; SD-1.x's default scheduler, 51 U-Net calls
 * for 50 steps — the reference's T = 51). Host-computed per step:
 *   coef[7] = {c_new, c_hist[0..3], a, b}, flags[3] = {store slot (-1 none), use cur, save cur}:
 *   e = CFG(eps); mo = c_new*e + sum c_hist[j]*hist[j]; hist[store] = e; src = use_cur ? cur : lat;
 *   if save_cur: cur = lat; lat = a*src - b*mo. hist [4][B*4*HW], cur [B*4*HW] fp32 device buffers.
 */
int sdmoe_cfg_multistep_step(const void* eps, long lde, float* lat, int B, int HW, int do_cfg, float guidance,
                             float* hist, float* cur, const float* coef, const int* flags, void* next_in, long ldn,
                             void* stream);

/*
 * Classifier-free guidance + one step of a sigma-parameterised scheduler on fp32 NCHW latents in place: diffusers'
 * EulerDiscreteScheduler and DPMSolverMultistepScheduler (dpmsolver++, order 2, midpoint), each with prediction_type
 * "epsilon" or "v_prediction" (the reference's SDXL, SD-2 and SD-2.1 configurations, utils.py:91-112), reduced to one
 * per-element form. Layouts as sdmoe_cfg_ddim_step: lat and prev_x0 fp32 [B,4,HW]; eps fp16 rows [ncopy*B*HW, lde],
 * uncond images first, channels 0..3; next_in (may be NULL) fp16 rows [ncopy*B*HW, ldn], channels 0..3 written only.
 * Host-computed per step (pipeline.euler_schedule / pipeline.dpmpp_2m_schedule):
 *   coef[6] = {cx, cm, a, b0, b1, in_scale}, flags[2] = {use_prev, store_prev}
 * The order within an element is fixed:
 *   1. m = CFG(eps); read x = lat; read p = prev_x0 if use_prev
 *   2. x0 = cx*x + cm*m;  x' = a*x + b0*x0 (+ b1*p if use_prev)
 *   3. prev_x0 = x0 if store_prev
 *   4. lat = x';  next_in = fp16(x' * in_scale) for both CFG copies
 * With use_prev == 0 the prev_x0 buffer is never read (it may hold anything, NaN included). prev_x0 may be NULL only
 * when both flags are 0 (SDMOE_EARG otherwise). lde and ldn must be multiples of 4.
 */
int sdmoe_cfg_x0_step(const void* eps, long lde, float* lat, int B, int HW, int do_cfg, float guidance,
                      float* prev_x0, const float* coef, const int* flags, void* next_in, long ldn, void* stream);

/*
 * sdmoe_prepare_input for a scheduler with an init_noise_sigma and a scale_model_input: lat = lat * lat_scale in
 * place (diffusers' latents * scheduler.init_noise_sigma), then out = fp16(lat * in_scale) for ncopy copies (the
 * first step's scale_model_input). Two separately rounded fp32 products. With both scales 1 the output is
 * bit-identical to sdmoe_prepare_input's and lat is unchanged.
 */
int sdmoe_prepare_input_scaled(float* lat, void* out, int B, int HW, long ldo, int ncopy, float lat_scale,
                               float in_scale, void* stream);

/*
 * The noise-HPO objective (the reference's modularity/remove_experts_noise_hpo.py:74-84) on device stores of the
 * U-Net's per-step output.
 * sdmoe_noise_capture: channels 0..3 of each of `rows` fp16 rows of eps (leading dimension lde, e.g. the pipeline's
 *   padded eps buffer) -> fp16 row r of store (leading dimension lds; 4 for a compact [rows, 4] step slice of a
 *   [T, nimg * HW, 4] store). lde, lds >= 4 and multiples of 4, both pointers 8-byte aligned. Runs on `stream`.
 * sdmoe_noise_distance: a, b fp16; step t's rows [nimg * HW] start at a + t * step_a (elements), row stride lda
 *   (>= 4, a multiple of 4, as the steps; pointers 8-byte aligned); only channels 0..3 of a row are read. Image i
 *   (rows [i * HW, (i + 1) * HW)) belongs to group img_group[i] (int32 device [nimg]; NULL: one group, ngroups must
 *   be 1; images whose entry is outside [0, ngroups) belong to no group). out: float64 [T, ngroups, 4] =
 *     { S (a - b)^2,  A = S |a|,  B = S |b|,  S (a / max(A, 1e-12) - b / max(B, 1e-12))^2 }
 *   over the elements of the group's images (the host takes the square roots: torch.norm(a - b), and the distance of
 *   the F.normalize(p = 1)'d vectors); a group without images gives zeros. All arithmetic is float64, the fourth
 *   sum is taken element by element with IEEE divisions (no expanded form). Fixed-order partial sums, no atomics:
 *   results are bit-identical from run to run. workspace: 4 * T * nimg * ceil(HW / 1024) doubles, 8-byte aligned.
 */
int sdmoe_noise_capture(const void* eps, long lde, void* store, long lds, long rows, void* stream);
int sdmoe_noise_distance(const void* a, long lda, long step_a, const void* b, long ldb, long step_b, int T, int nimg,
                         int HW, const int* img_group, int ngroups, double* out, double* workspace,
                         long workspace_doubles, void* stream);

/*
 * The CLIP removal-quality scorer's image front end and score reduction (csrc/clip_image.hip). Replaces: the PNG
 * round trip, CLIPProcessor's host-side Pillow bicubic resize / centre crop / normalise and the per-image fp32
 * cosines of benchmarks/artist_removal.py:182-207 and benchmarks/art_removal.py:80-98, 114-125.
 * sdmoe_clip_quantise: x [B, 3, H, W] fp16 (is_fp32 == 0) or fp32, contiguous -> out [B, H, W, 3] uint8,
 *   rint(float(x) * 255.0f) round-half-even, clamped to [0, 255] (NaN -> 0). Replaces diffusers' numpy_to_pil
 *   ((images * 255).round().astype("uint8")).
 * sdmoe_clip_resample_h / _v: Pillow's 8-bit bicubic resampler (libImaging/Resample.c), horizontal pass then
 *   vertical pass with a uint8 intermediate, restricted to the centre-crop window. A pass's table is `bounds` int32
 *   [S, 2] = (first tap, taps) and `kk` int32 [S, ksize] 22-bit fixed-point weights, device memory, built on the host
 *   exactly as precompute_coeffs / normalize_coeffs_8bpc do, for the S outputs inside the crop window; an output is
 *   clip8((2^21 + sum pixel * k) >> 22) in int32. The caller guarantees every tap range lies inside the image
 *   (horizontal: [0, W)) or inside rows [row0, row0 + nrows) (vertical).
 *   _h: in uint8 [B, H, W, 3] (image b at in + b * in_bstride bytes) -> tmp uint8 [B, nrows, S, 3], input rows
 *     [row0, row0 + nrows).
 *   _v: tmp -> u8out uint8 [B, S, S, 3] (optional) and A (optional): fp16 ((u8 * (1/255)) - mean[c]) / std[c],
 *     each step rounded in fp32, at row b G^2 + py G + px (G = S / patch, row stride lda), column
 *     c patch^2 + iy patch + ix -- the flattening of the patch-embedding conv weight [D, 3, patch, patch] -- with
 *     columns [3 patch^2, kpad) written as zero (kpad <= lda; the patch GEMM's K padded to a multiple of 64). mean,
 *     std: 3 host floats. Replaces CLIPImageProcessor.resize / center_crop / rescale / normalize and the unfold of
 *     CLIPVisionEmbeddings.patch_embedding; no fp32 pixel_values tensor exists.
 * sdmoe_clip_scores: T (may be NULL), A, R fp16 [n, D] feature rows (text, original image, removal image; row
 *   strides ldt, lda, ldr) -> out float64 [3 n + 3]: out[i] = cos(T,A), out[n + i] = cos(T,R), out[2 n + i] =
 *   cos(A,R) of row i, cos(x,y) = x.y / (max(|x|, 1e-8) max(|y|, 1e-8)) (torch.nn.functional.cosine_similarity;
 *   0 for the text cosines without T), then out[3 n ..] = sum cos(A,R), sum cos(A,R)^2, count of cos(T,A) > cos(T,R).
 *   float64 throughout, fixed summation order, no atomics: bit-identical from run to run. out 8-byte aligned.
 */
int sdmoe_clip_quantise(const void* x, int is_fp32, int B, int H, int W, void* out, void* stream);
int sdmoe_clip_resample_h(const void* in, long in_bstride, int B, int H, int W, int row0, int nrows,
                          const int* bounds, const int* kk, int ksize, int S, void* tmp, void* stream);
int sdmoe_clip_resample_v(const void* tmp, int B, int row0, int nrows, const int* bounds, const int* kk, int ksize,
                          int S, int patch, const float* mean, const float* std, void* u8out, void* A, long lda,
                          int kpad, void* stream);
int sdmoe_clip_scores(const void* T, long ldt, const void* A, long lda, const void* R, long ldr, int n, int D,
                      double* out, void* stream);

/*
 * The object-erasure scorer's CNN pieces and score reduction (csrc/imagenet.hip): what torchvision's resnet50 needs
 * beyond sdmoe_linear / sdmoe_conv3x3, and the top-k label match. Replaces: the per-image host classifier pass and
 * the Python name matching of benchmarks/object_erase.py:247-302 and benchmarks/save_union_over_time.py:264-276.
 * Streaming kernels, 16-byte accesses where pointers and strides allow (16-byte aligned, strides % 8 == 0) and an
 * element-wise path otherwise; no atomics, fixed summation order: bit-identical from run to run.
 * sdmoe_stem_rows: u8 uint8 [B, S, S, 3] (contiguous) -> A fp16 [B So^2, kpad] (row stride lda), So = (S - 1) / 2 + 1:
 *   the im2col rows of a 7x7 / stride 2 / padding 3 conv. Row b So^2 + oy So + ox, column c 49 + ky 7 + kx (the
 *   flattening of torch's [Cout, 3, 7, 7] weight) = fp16(((u8 * (1/255)) - mean[c]) / std[c]) of input pixel
 *   (2 oy - 3 + ky, 2 ox - 3 + kx), each step rounded in fp32; 0 where the tap lies outside the image (the padding is
 *   applied after the normalisation) and in columns [147, kpad). kpad >= 147, lda >= kpad. mean, std: 3 host floats.
 *   Replaces torchvision's to_tensor / normalize and the unfold of ResNet.conv1; the stem is then one sdmoe_linear.
 * sdmoe_maxpool3x3s2: X fp16 NHWC [B, H, W, C] (pixel stride ldx) -> Y [B, OH, OW, C] (pixel stride ldy), OH =
 *   (H - 1) / 2 + 1, OW likewise: max over the 3x3 window at stride 2, padding 1. Padding never wins (-inf), NaN
 *   propagates, the first of equal values is kept: torch.nn.functional.max_pool2d(x, 3, 2, 1) bit for bit. C % 8 == 0.
 * sdmoe_avgpool_rows: X fp16 [B * HW, C] (row stride ldx) -> Y fp16 [B, C] (row stride ldy): fp16(s / HW) with s the
 *   fp32 sum of the image's HW rows in row order. C % 8 == 0. Replaces AdaptiveAvgPool2d(1) + flatten.
 * sdmoe_add_relu: out[i] = relu(fp16(float(a[i]) + float(b[i]))), i < n, any n and any 2-byte alignment; negative
 *   sums give +0, -0 and NaN pass through (torch.relu(a + b)). out may alias a or b.
 * sdmoe_topk_hits: logits fp16 [n, C] (row stride ldl), 1 <= k <= min(C, 8) -> topk int32 [n, k]: per row the k best
 *   class ids in descending logit order, ties (-0 == +0) to the lower id, NaN above +inf (torch.topk's ranking, so a
 *   broken run shows). table uint32 [G, ceil(C / 32)]: bit c % 32 of word c / 32 of row g is set where class c counts
 *   as a hit for label g; label int32 [n]. hit int32 [n] = 1 if one of the row's k classes is set in row label[i],
 *   else 0; total int32 [1] = sum of hit, taken in image order by one block. label is range-checked on the device:
 *   a label outside [0, G) reads no table row and gives hit[i] = -1 and total = -1 (the error status; the entry
 *   point itself cannot see device data). One wave per image.
 */
int sdmoe_stem_rows(const void* u8, int B, int S, const float* mean, const float* std, void* A, long lda, int kpad,
                    void* stream);
int sdmoe_maxpool3x3s2(const void* X, long ldx, int B, int H, int W, int C, void* Y, long ldy, void* stream);
int sdmoe_avgpool_rows(const void* X, long ldx, int B, int HW, int C, void* Y, long ldy, void* stream);
int sdmoe_add_relu(const void* a, const void* b, void* out, long n, void* stream);
int sdmoe_topk_hits(const void* logits, long ldl, int n, int C, int k, const unsigned* table, int G, const int* label,
                    int* topk, int* hit, int* total, void* stream);

/*
 * The concept checkers' decision step on the device (csrc/concepts.hip): from fp16 text-encoder hidden-state rows to
 * the per-prompt select words of sdmoe_wmask_union_sets, with no host round trip. float64 arithmetic in one fixed
 * order, no atomics: bit-identical from run to run.
 * sdmoe_text_pool: X fp16 [nseq * L, D] (row stride ldx) -> out float64 [nseq / group, D] (row stride ldo). Per
 *   sequence p = mean over its L rows, f = p / |p| (IEEE division, no epsilon: an all-zero block gives NaN, as the
 *   reference); out[g] = mean of f over sequences g * group .. (g + 1) * group - 1, summed in sequence order and
 *   divided by group, then out[g] / |out[g]| if renorm. group = 1: a prompt's feature. group = n_objects, renorm = 0:
 *   one row of embed_all_objects / embed_anchor_prompts; renorm = 1: no_concept_features. The reference normalises
 *   object_features twice (concept_checkers.py:55, :59): the second pass is a no-op to within an ulp, done once here.
 *   nseq % group == 0, ldx >= D, ldo >= D (SDMOE_EARG); D <= 2048 (SDMOE_EUNSUP); X 2-byte and out 8-byte aligned
 *   (SDMOE_ESHAPE). 16-byte loads when X is 16-byte aligned and ldx % 8 == 0, else 2-byte loads.
 * sdmoe_concept_route: one launch for a batch. Prompt b's feature f_b is pooled from its L rows of X (as above,
 *   group = 1); sims[b][r] = f_b . bank[r] over the R float64 rows of bank (row stride ldb), every row summed in the
 *   same lane / column order, so identical bank rows give identical sims; written to sims_out [nprompt, R] if not
 *   NULL. Then, for each of the G records of `groups` (device memory): m = max of sims[b][row0 .. row1 - 1], r* the
 *   FIRST row reaching it (Python's max(sim, key=sim.get), concept_checkers.py:174); the group fires iff
 *   (m > sims[b][neg_row] && m > threshold) || (anchor_row >= 0 && sims[b][anchor_row] > sims[b][neg_row]) --
 *   strict comparisons, false whenever a NaN is involved (:127-133, :179); threshold = -inf for none. A firing group
 *   ORs bit row_bit[r*] (device int32 [R], -1 = none: the arg-max concept is unknown to the remover, nothing is removed
 *   even when the runner-up is known, unified_editing.py:116; rows may share a bit) into select_out[b], which starts
 *   from preset[b] (device uint32 [nprompt], may be NULL: host-side decisions such as MemorizedPromptChecker.decide,
 *   :237-241). G == 0 gives select = preset. A record whose rows lie outside [0, R) never fires; a bit outside
 *   0..31 is ignored. Limits and alignment as sdmoe_text_pool; bank, groups, sims_out 8-byte, the int tables 4-byte
 *   aligned.
 * Replaces: ArtStyleChecker.decide / NudityChecker.decide and BaseConceptChecker.similarity / embed_all_objects /
 *   no_concept_features (benchmarks/concept_checkers.py:32-81, 119-133, 170-184), which run one fp32 CLIP text pass per
 *   prompt and per checker, and the routing lines of benchmarks/unified_editing.py:106-126 that turn their answers
 *   into each prompt's concept list on the host.
 */
typedef struct sdmoe_concept_group {
  int row0, row1;   /* the group's bank rows [row0, row1) */
  int neg_row;      /* the no-concept row */
  int anchor_row;   /* -1 = none */
  double threshold; /* -inf = none */
} sdmoe_concept_group;
int sdmoe_text_pool(const void* X, long ldx, int nseq, int L, int D, int group, int renorm, double* out, long ldo,
                    void* stream);
int sdmoe_concept_route(const void* X, long ldx, int nprompt, int L, int D, const double* bank, long ldb, int R,
                        const int* row_bit, const sdmoe_concept_group* groups, int G, const unsigned* preset,
                        unsigned* select_out, double* sims_out, void* stream);

/*
 * Tuning knobs for A/B experiments: process-wide integers the launch code reads. Ids, legal values and defaults are
 * ABI (recorded command lines name them). This is the one definition of what each value means; the library's table
 * (csrc/tune.hip) holds id, name, default and legal set. sdmoe_tune returns -1 for an unknown knob or an illegal
 * value and then leaves the knob unchanged. Not synchronised: set knobs between launches, from one thread.
 *   0 stages      GEMM LDS ring depth: 0 (default) auto, 2 or 3;
 *   1 tile        forced GEMM tile: 0 (default) auto, 1 = 128x160, 2 = 64x160, 3 = 256x320 8-wave, 4 = 256x160 8-wave,
 *                 5 = 256x320 4x2-wave, 6 = 128x320 8-wave, 7 = 128x160 8-wave, 8 = 64x320 8-wave (7 / 8: plain GEMM /
 *                 conv / LN-folded GEMM only); a forced tile also turns the halo convs off;
 *   4 attn        attention kernel: 0 (default) by shape, 1 = 32x32x16 MFMA kernel, 2 / 4 = 4-wave 16x16x32 kernel with
 *                 32 / 64 queries per wave (64 for head_dim <= 40 only), 8 = 16x16x32 kernel in 8-wave workgroups,
 *                 9 = 32x32x16 kernel in 8-wave workgroups (8 / 9: head_dim <= 80);
 *   6 diag        GEMM diagnostics bits, results garbage, 0..63 (default 0): 1 no K-loop operand loads, 2 no MFMAs,
 *                 4 no epilogue (nothing stored), 8 epilogue without its global stores, 16 no A-operand pieces,
 *                 32 no B-operand pieces;
 *   7 gn_fused    sdmoe_groupnorm at HW <= 256: 1 (default) statistics + apply in one launch with the rows held in
 *                 registers, 2 the same launch re-reading the rows for the apply, 0 two launches;
 *   8 res16       GEMM residual epilogue: 1 (default) output rounded to fp16 then the residual added in fp16 arithmetic
 *                 (diffusers' fp16 `linear(x) + residual`), 0 = accumulator + residual rounded once (fp32 staging);
 *   9 ksplit      forced split-K factor: 0 (default) auto, 1 = never split, 2..32 (clamped to the K-steps; halo convs:
 *                 at most one 32-channel slice per split);
 *  14 mfast       split-K conv tile order: 1 (default) M-tile fastest (one XCD's workgroups share weight slices in its
 *                 L2), 0 split fastest;
 *  15 topk        top-k expert selection kernels: 0 (default) one token per wave at M <= 16384, four above, and the
 *                 keep bits at E <= 64 with one quad of lanes per token; 1 / 4 = always the ballot kernel at one /
 *                 four tokens per wave;
 *  16 halo        halo-tiled 3x3 convs: 1 (default) where measured faster (64- and 16-wide outputs, the upsample convs,
 *                 32-wide outputs with Cin >= 1280; grids of <= 32 256-row tiles -- one prompt per call -- on 128-row
 *                 tiles for the 64-, 16- and narrow-input 32-wide outputs and the 16 -> 32 upsample), 2 = every 128-row
 *                 halo tile instead, 3 = the default plus every 32-wide output on 256-row tiles, 0 = off;
 *  20 gt320       table-GELU routed GEGLU tiles: 1 (default) 256x320 like the ReLU kernel, 0 = 256x160 (4x2 waves);
 *  21 narrow      convs with at most 32 output channels (conv_out): 1 (default) 128x32 tiles, 0 = 128x64;
 *  23 epi_direct  fp16 GEMM / conv epilogues: 1 (default) 16-B row pieces stored straight from the MFMA fragments (two
 *                 v_permlane16_swap per fragment pair, no LDS staging) when there is no residual, 2 = always,
 *                 0 = staged in LDS.
 */
int sdmoe_tune(int knob, int value);

/*
 * Enumerates the knob table: entry `index` (0 .. until it returns -1) gives the knob's id, its short name (a static
 * string), its default and its current value. -1 for an index past the end or a null output pointer. Host only.
 */
int sdmoe_tune_knob(int index, int* id, const char** name, int* default_value, int* value);

/* Sets every knob to its default. Host only. */
int sdmoe_tune_reset(void);

/*
 * Registers, for the calling thread's current HIP device, the fp16 GELU table the GEGLU kernels apply for
 * act == SDMOE_ACT_GELU (sdmoe_linear_geglu / _ln, sdmoe_geglu_route): table[i] = gelu(x) for the 16384 fp16 inputs
 * x with 2^-5 <= |x| < 8, i = ((bits(x) & 0x7fff) - 0x2800) | (sign(x) << 13), device memory, 16-B aligned, kept
 * alive by the caller while registered (NULL unregisters: the kernels then evaluate 0.5 x erfc(-x / sqrt 2) in
 * fp32, within 1 fp16 ulp). The host layer fills it with the reference module's own activation (GEGLU.gelu =
 * F.gelu on fp16 tensors, diffusers activations.py; the hook's module.gelu(gate), remove_skilled_experts.py:27,
 * moefy.py:13) evaluated on every such input, so the fused routed GEGLU reproduces the reference's fp16 gate
 * values bit for bit on all of them; |x| < 2^-5, |x| >= 8 are computed (see csrc/common.h gelu_tab_h).
 * No GPU call; not stream-ordered: register before launching work that reads it.
 */
int sdmoe_set_gelu_table(const void* table);

/* out = a + b (fp16, n % 8 == 0). */
int sdmoe_add(const void* a, const void* b, void* out, long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDMOE_H */
