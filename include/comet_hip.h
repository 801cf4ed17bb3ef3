/*
 * comet_hip.h — C-ABI of libcomet_hip.so, the MI355X (gfx950) kernel library behind the
 * COMET Trajectory-Guided Temporal Modeling path.
 *
 * Conventions (SURVEY.md §8b "C-ABI the HIP library must export"):
 *   - every pointer is a device pointer owned by the caller (PyTorch caching allocator);
 *     the library allocates nothing and keeps no device state between calls;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*), never syncs,
 *     and is safe to capture into a hipGraph;
 *   - return 0 on success, a negative COMET_E* code otherwise; comet_last_error() returns a
 *     thread-local message describing the last failure on the calling thread;
 *   - dtype codes: COMET_F32 = 0, COMET_BF16 = 1. Accumulation is always f32.
 *
 * Each entry point names the reference operator(s) it replaces (file:line under
 * wulibingbinglin/COMET-Pose-Estimation).
 */
#ifndef COMET_HIP_H_
#define COMET_HIP_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COMET_F32 0
#define COMET_BF16 1

#define COMET_OK 0
#define COMET_EINVAL -1     /* bad argument / unsupported shape */
#define COMET_ELAUNCH -2    /* kernel launch failed */

#define COMET_ACT_NONE 0
#define COMET_ACT_GELU 1    /* exact erf GELU, nn.GELU() (modules.py:127) */
#define COMET_ACT_RELU 2
#define COMET_ACT_SIGMOID 3

int comet_version(void);
const char* comet_last_error(void);

/* ---------------------------------------------------------------------------------------
 * GEMM with fused epilogue. Replaces every nn.Linear / packed MHA in_proj / out_proj
 * (modules.py:119-154, 248-344; torch.nn.MultiheadAttention), convolution GEMMs after
 * im2col (blocks.py:27-196, DINOv2 patch-embed) and the head's backward GEMMs.
 *
 *   v = alpha * sum_k A[m,k] * B[k,n]            (f32 accumulate, bf16 or f32 MFMA)
 *   v += bias  (per column n, or per row m)
 *   if aux: aux[m,n] = v                         (pre-activation, for backward)
 *   v = act(v)
 *   if resid: v += beta * resid[m,n]             (resid may alias c)
 *   c[m,n] = v
 *
 * layout_a 0: A[m*lda + k]; 1: A[k*lda + m].  layout_b 0: B[n*ldb + k] (Linear weight
 * [out,in]); 1: B[k*ldb + n]. Two batch dimensions: element base = b0*stride[0] + b1*stride[1].
 * Bias is always f32; c / resid / aux use dtype_c.
 *
 * Split-K: split_k 0 = library heuristic (splits K when the output tiles cannot fill the 256 CUs,
 * e.g. weight gradients reduced over every token), 1 = never, s > 1 = force s splits. A split
 * GEMM needs an f32 workspace of comet_gemm_workspace() bytes; with workspace == NULL (or too
 * small) the GEMM runs unsplit. Partials are summed in a fixed order: results are deterministic.
 * ------------------------------------------------------------------------------------- */
typedef struct comet_gemm_args {
  int32_t dtype_ab;
  int32_t dtype_c;
  int32_t layout_a;
  int32_t layout_b;
  int64_t m, n, k;
  int64_t batch[2];
  const void* a; int64_t lda; int64_t stride_a[2];
  const void* b; int64_t ldb; int64_t stride_b[2];
  void* c; int64_t ldc; int64_t stride_c[2];
  const float* bias; int32_t bias_mode; int64_t stride_bias[2];
  const void* resid; int64_t ldr; int64_t stride_r[2];
  void* aux; int64_t ldaux; int64_t stride_aux[2];
  float alpha; float beta;
  int32_t act;
  void* workspace; int64_t workspace_bytes;
  int32_t split_k;
  int32_t convert_a, convert_b;  /* 1: that operand is f32 in memory, rounded to bf16 on load
                                    (dtype_ab must be COMET_BF16; convert_b: layout_b 1 only) */
} comet_gemm_args;

int comet_gemm(const comet_gemm_args* args, void* stream);
/* Workspace bytes comet_gemm needs for these arguments (0 when it will not split K). */
int comet_gemm_workspace(const comet_gemm_args* args, int64_t* bytes);
/* Same, plus the kernel plan comet_gemm will launch: plan[0] = 0 skinny (N <= 64),
 * 1 256-row tile, 2 128 x 128 tile; plan[1] = the 256-row tile's BN; plan[2] = K splits.
 * Lets a profiler name the kernel instance a call lands on (bench.py roofline). */
int comet_gemm_plan(const comet_gemm_args* args, int64_t* bytes, int32_t* plan);

/* GEMM + row LayerNorm epilogue (AttnBlock / CrossAttnBlock of the tracker's update former,
 * blocks.py:205-348 over modules.py:248-344, all under no_grad): the f32 residual GEMM whose
 * output row v = x @ w^T + bias + beta*resid feeds LayerNorms (norm2 of the same block; norm1 /
 * norm_context of the next blocks) writes those LayerNorms itself:
 *   c   = v when raw_c != 0, else (v - mean(v)) / sqrt(var(v) + eps_y)        [f32]
 *   y16 = (v - mean(v)) / sqrt(var(v) + eps_y)                                  [bf16, optional]
 *   z16 = (v - mean(v)) / sqrt(var(v) + eps_z) * zw + zb                        [bf16, optional]
 * (biased variance, as nn.LayerNorm). Eligible (comet_gemm_rowln_ok): bf16 k-contiguous A / B,
 * K % 64 == 0, M >= 4096, N in {256, 384}, dtype_c f32 with resid, act NONE, no aux, no split. */
typedef struct comet_rowln_args {
  void* y16; int64_t ldy; float eps_y;
  void* z16; int64_t ldz; const float* zw; const float* zb; float eps_z;
  int32_t raw_c;
} comet_rowln_args;
int comet_gemm_rowln_ok(const comet_gemm_args* args);
/* Few rows (M <= 32 x CUs) and a long K: the row-LN GEMM runs as split-K partials + one LN reduce when
 * args->workspace holds comet_gemm_rowln_workspace() bytes (0: no split; without the workspace the
 * single-kernel path runs, same outputs within f32 summation order). */
int comet_gemm_rowln_workspace(const comet_gemm_args* args, int64_t* bytes);
int comet_gemm_rowln(const comet_gemm_args* args, const comet_rowln_args* ln, void* stream);

/* GEMM + activation backward (Mlp.fc2's input gradient fused with fc1's GELU backward and bias
 * gradient, modules.py:18-40 / timm Mlp under loss.backward(), train_eval_func_new_cp5.py:793):
 *   c[m, n]   = bf16( act'(pre[m, n]) * alpha * sum_k A[m, k] B[k, n] )     (act = GELU, erf form)
 *   dbias[n]  = sum_m c[m, n]   (the rounded values; zeroed first; may be NULL)
 * pre: bf16 [M, N] at row pitch ldpre (fc1's saved pre-activation). Replaces the dX GEMM + the
 * comet_act_bwd_colsum pass (the hidden gradient is written once instead of written, read and
 * written again). Eligible (comet_gemm_dact_ok): act GELU, bf16 A / B / C, A k-contiguous, no bias,
 * residual, aux or forward activation, one batch, N % 8 == 0, 16-B aligned C and pre, a 256-row
 * tile plan (comet_gemm_plan kind 1) without split-K. */
int comet_gemm_dact_ok(const comet_gemm_args* args, int32_t act, const void* pre, int64_t ldpre);
int comet_gemm_dact(const comet_gemm_args* args, int32_t act, const void* pre, int64_t ldpre, float* dbias,
                    void* stream);


/* ---------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on channels-last activations (nn.Conv2d of BasicEncoder /
 * ShallowEncoder / ResidualBlock, blocks.py:27-202, modules.py:39-116): the im2col matrix is
 * never materialised; the GEMM's A tiles are gathered from x directly.
 *   y[(n*oh + oy)*ow + ox][co] = act(bias[co] + sum_{ky,kx,ci} x[n][oy*s-p+ky][ox*s-p+kx][ci]
 *                                    * weight[co][(ky*kw + kx)*c + ci]) + beta*resid[...]
 * x [n,h,w,c] bf16 contiguous with c % 8 == 0; weight [cout][ldw] bf16 (K = kh*kw*c <= ldw);
 * y / resid use dtype_y with row pitch ldy / ldr. (f32 or c % 8 != 0: im2col + comet_gemm.)
 * ------------------------------------------------------------------------------------- */
typedef struct comet_conv_args {
  int32_t dtype;      /* x and weight: COMET_BF16 */
  int32_t dtype_y;
  const void* x; int64_t n, h, w, c;
  const void* weight; int64_t cout, ldw;
  int32_t kh, kw, stride, pad;
  const float* bias;
  void* y; int64_t ldy;
  const void* resid; int64_t ldr; float beta;
  int32_t act;
} comet_conv_args;

int comet_conv2d_nhwc(const comet_conv_args* args, void* stream);
/* The kernel comet_conv2d_nhwc will launch for these arguments (host only, launches nothing; the
 * launcher takes the same decision function): plan[0] = 0 128 x 128 implicit GEMM, 1 128 x 64
 * implicit GEMM (cout <= 64), 2 narrow-output kernel (cout <= 64 in 16s, weights in registers,
 * >= 16384 output pixels), 3 3x3 rows in LDS (c = cout = 64); for kind 2, plan[1] = its NT16
 * (cout / 16), plan[2] = its KC template value (32-element k chunks held), plan[3] = 1 when it
 * stores 16 bytes per lane (bf16 output, cout % 32 == 0); 0 otherwise. */
int comet_conv_plan(const comet_conv_args* args, int32_t* plan);

/* ---------------------------------------------------------------------------------------
 * Row LayerNorm over the last dim (nn.LayerNorm; also GroupNorm(1, C) on [rows, C] as used
 * by base_track_predictor.py:81,238). weight/bias f32 or NULL (elementwise_affine=False,
 * modules.py:261-317). mean/rstd (f32, [rows]) are written when non-NULL (for backward).
 * Output dtype may differ from input dtype (f32 residual stream -> bf16 GEMM operand).
 * ldx / ldy are row strides (elements); relu != 0 applies ReLU after the affine
 * (TrajectoryEncoder LN -> ReLU, camera_predictor10.py:79-81).
 * ------------------------------------------------------------------------------------- */
int comet_layernorm_fwd(int dtype_x, int dtype_y, const void* x, const float* weight,
                        const float* bias, void* y, void* y2, float* mean, float* rstd,
                        int64_t rows, int64_t cols, int64_t ldx, int64_t ldy, int64_t ldy2,
                        float eps, int relu, void* stream);
/* y2 (bf16, may be NULL; y may be NULL when y2 is given): a second copy of the output for the GEMM
 * that consumes it (AttnBlock: the normed x is both the in_proj input and the residual).
 * dx (dtype_dx) = LN backward of dy + dy2 (dy2 bf16, may be NULL); dweight/dbias (f32) are
 * ACCUMULATED (+=) when non-NULL. dx_accumulate != 0 adds into dx instead of overwriting. */
int comet_layernorm_bwd(int dtype_x, int dtype_dy, const void* x, const void* dy, const void* dy2,
                        const float* mean, const float* rstd, const float* weight,
                        int dtype_dx, void* dx, float* dweight, float* dbias, int64_t rows, int64_t cols,
                        int dx_accumulate, void* stream);
/* x + f(LN(x)) (modules.py:293-294, 342-343): dx (f32) = dres + LN backward of dy, one pass
 * (x f32, dy f32 / bf16, cols % 8 == 0, 32-B aligned rows). */
int comet_layernorm_bwd_res(int dtype_x, int dtype_dy, const void* x, const void* dy, const float* dres,
                            const float* mean, const float* rstd, const float* weight, float* dx,
                            float* dweight, float* dbias, int64_t rows, int64_t cols, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused multi-head attention forward (flash style: LDS-staged K/V, online softmax, MFMA for
 * Q·Kᵀ and P·V). Replaces the explicit bmm-softmax-bmm path of nn.MultiheadAttention
 *  at every use site (head self/cross/T_P/trunk, tracker time/space,
 * DINOv2). Tensors are addressed [batch, head, token, d] with arbitrary element strides.
 * lse (f32, [batch, head, lq], may be NULL) receives log-sum-exp of the scaled scores.
 * ------------------------------------------------------------------------------------- */
typedef struct comet_attn_args {
  int32_t dtype;      /* q/k/v/o dtype */
  int32_t head_dim;   /* 32, 48, 64, 96 */
  int64_t batch, heads, lq, lk;
  const void* q; int64_t sq_b, sq_h, sq_l;
  const void* k; int64_t sk_b, sk_h, sk_l;
  const void* v; int64_t sv_b, sv_h, sv_l;
  void* o; int64_t so_b, so_h, so_l;
  float* lse;         /* contiguous [batch, heads, lq] */
  float scale;
  /* optional inner batch (0 / 1 = none): batch index b addresses (b / batch_inner) * s*_b +
   * (b % batch_inner) * s*_i -- attention over the tracks of a [B, N, T, C] tensor for every
   * (b, t) (EfficientUpdateFormer space blocks, blocks.py:322-340) without permuting it */
  int64_t batch_inner;
  int64_t sq_i, sk_i, sv_i, so_i;
} comet_attn_args;

int comet_attention_fwd(const comet_attn_args* args, void* stream);

/* Fused attention backward (bf16, flash style, nothing Lq x Lk in HBM): given q/k/v, the
 * forward output o, its lse and the incoming gradient dout, writes dq, dk, dv (bf16, any
 * 16-B-aligned strides). delta: f32 workspace [batch, heads, lq] (receives rowsum(dout*o)).
 * Replaces autograd through nn.MultiheadAttention's bmm-softmax-bmm. */
typedef struct comet_attn_bwd_args {
  int32_t dtype;      /* COMET_BF16 */
  int32_t head_dim;   /* 32, 48, 64, 96 */
  int64_t batch, heads, lq, lk;
  const void* q; int64_t sq_b, sq_h, sq_l;
  const void* k; int64_t sk_b, sk_h, sk_l;
  const void* v; int64_t sv_b, sv_h, sv_l;
  const void* o; int64_t so_b, so_h, so_l;
  const void* dout; int64_t sd_b, sd_h, sd_l;
  void* dq; int64_t sdq_b, sdq_h, sdq_l;
  void* dk; int64_t sdk_b, sdk_h, sdk_l;
  void* dv; int64_t sdv_b, sdv_h, sdv_l;
  const float* lse;   /* [batch, heads, lq], natural log, from comet_attention_fwd */
  float* delta;       /* workspace [batch, heads, lq] */
  float scale;
} comet_attn_bwd_args;

int comet_attention_bwd(const comet_attn_bwd_args* args, void* stream);

/* Attention backward helpers (materialised form, head_dim-agnostic):
 * probs[r, j] = exp(s[r, j]*scale - lse[r]); s is f32, probs has dtype_s (the compute dtype);
 * rows = batch*heads*lq, ld = row stride. */
int comet_attn_probs(int dtype_s, const void* s, const float* lse, void* p, int64_t rows,
                     int64_t cols, int64_t ld_s, int64_t ld_p, float scale, void* stream);
/* dS[r, j] = P[r, j] * (dP[r, j] - delta[r]) * scale, delta[r] = sum_d dO[r,d]*O[r,d]
 * (computed by comet_attn_delta). P and dS have dtype_p, dP is f32. */
int comet_attn_delta(int dtype, const void* dout, const void* out, float* delta, int64_t batch,
                     int64_t heads, int64_t lq, int64_t d, int64_t so_b, int64_t so_h,
                     int64_t so_l, int64_t sdo_b, int64_t sdo_h, int64_t sdo_l, void* stream);
int comet_attn_dsoftmax(int dtype_p, const void* p, const void* dp, const float* delta, void* ds,
                        int64_t rows, int64_t cols, int64_t ld, float scale, void* stream);

/* ---------------------------------------------------------------------------------------
 * Elementwise / reductions.
 * ------------------------------------------------------------------------------------- */
int comet_cast(int dtype_in, int dtype_out, const void* x, void* y, int64_t n, void* stream);
/* dst[i][0:sizes[i]] = bf16(src[i][...]) for n_tensors f32 tensors in few launches (the bf16
 * copies of the trainable camera-head weights, refreshed after each AdamW step). */
int comet_cast_multi_f32_bf16(const float* const* src, void* const* dst, const int64_t* sizes,
                              int n_tensors, void* stream);
/* y = act(x) (f32 or bf16); gelu backward: dx = dy * gelu'(pre) */
int comet_act_bwd(int act, int dtype_pre, int dtype_dy, const void* pre, const void* dy,
                  void* dx, int dtype_dx, int64_t n, void* stream);
/* y = a*x + b*y (f32) */
int comet_axpby(const float* x, float* y, float a, float b, int64_t n, void* stream);
/* column sum: out[c] (+)= sum_r x[r*ld + c]  (bias gradients). */
int comet_colsum(int dtype, const void* x, float* out, int64_t rows, int64_t cols, int64_t ld,
                 int accumulate, void* stream);
/* Linear backward prologue in one pass (cols % 8 == 0, contiguous [rows, cols], 32-B aligned):
 * g = dy * act'(pre) (act NONE: g = dy, pre unused); if out: out = g (dtype_out);
 * if dbias: dbias[c] (+)= sum_r g[r, c] (of the rounded g when out is bf16). */
int comet_act_bwd_colsum(int act, int dtype_pre, const void* pre, int dtype_dy, const void* dy,
                         int dtype_out, void* out, float* dbias, int64_t rows, int64_t cols,
                         int accumulate, void* stream);
/* squared L2 norm of many tensors: out[0] += sum x_i^2  (clip_grad_norm_, train_eval_func_new_cp5.py:797),
 * in a fixed summation order (bit-identical across launches: the clip coefficient of every
 * data-parallel replica); partials: device scratch of COMET_SQ_NORM_PARTIALS floats, stream-ordered. */
#define COMET_SQ_NORM_PARTIALS 1024
int comet_sq_norm_multi(const float* const* ptrs, const int64_t* sizes, int n_tensors,
                        float* out, float* partials, void* stream);
/* fused AdamW over many f32 tensors (torch.optim.AdamW defaults, train_util.py:311-332);
 * grad scaled by clip = min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) when sqnorm != NULL. */
int comet_adamw_multi(float* const* params, const float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const int64_t* sizes, int n_tensors, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step,
                      const float* sqnorm, float max_norm, void* stream);

/* ---------------------------------------------------------------------------------------
 * Convolution / CNN operators (channels-last NHWC activations).
 * ------------------------------------------------------------------------------------- */
/* im2col for conv2d NHWC input [n, h, w, c] -> cols [n*oh*ow, ldc], column (ky*kw+kx)*c+ci,
 * columns [kh*kw*c, ldc) zero-filled (K padded to the GEMM vector width). */
int comet_im2col_nhwc(int dtype_in, int dtype_out, const void* x, void* cols, int64_t n,
                      int64_t h, int64_t w, int64_t c, int kh, int kw, int stride, int pad,
                      int64_t oh, int64_t ow, int64_t ldc, void* stream);
/* InstanceNorm2d (affine=False, eps 1e-5) on NHWC, optional residual add and ReLU:
 * o = IN(x); if res_norm_relu: o = relu(o); if res: o += res; if relu: o = relu(o).
 * (ResidualBlock tail relu(x + relu(IN(conv2(.)))), modules.py:108-116).
 * Large images are split over several workgroups per image; that path needs an f32 workspace
 * of comet_instnorm_workspace() bytes (with a NULL / short workspace one workgroup per image). */
int comet_instnorm_workspace(int64_t n, int64_t hw, int64_t c, int64_t* bytes);
int comet_instnorm_nhwc(int dtype, const void* x, const void* res, void* y, int64_t n,
                        int64_t hw, int64_t c, float eps, int relu, int res_norm_relu,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* bilinear resize, align_corners=True, NCHW or NHWC (F.interpolate, blocks.py:179-202,
 * track_predictor.py:137, camera_predictor10.py:624). add != 0 accumulates into y. */
int comet_resize_bilinear(int dtype_in, int dtype_out, int nhwc, const void* x, void* y,
                          int64_t n, int64_t c, int64_t h, int64_t w, int64_t oh, int64_t ow,
                          int add, void* stream);
/* NHWC resize (align_corners=True) and the 2 x 2 / stride-2 average pool of its output in one pass
 * (refine_track.py fine features + blocks.py:371 F.avg_pool2d): y [n, oh, ow, c], pool
 * [n, oh / 2, ow / 2, c], both equal to comet_resize_bilinear followed by comet_avgpool2_nhwc.
 * c in {8, 16, 32, 64, 128, 256}, 16-B aligned, input image h * w * c elements of at most 32 KiB. */
int comet_resize_bilinear_pool_nhwc(int dtype_in, int dtype_out, const void* x, void* y, void* pool,
                                    int64_t n, int64_t c, int64_t h, int64_t w, int64_t oh, int64_t ow,
                                    void* stream);
/* The fine ShallowEncoder's tail (blocks.py:97-110 + the fine pyramid's pool, refine_track.py):
 * x2 = (x + up(up1)) + up(up2) (each sum rounded to bf16, as two resize-and-add calls; up1 / up2
 * optional, [n, h1, w1, c] / [n, h2, w2, c], align_corners=True), t = x2 + conv1x1(x2; weight
 * [c, c] bf16, bias f32) rounded as comet_gemm's narrow kernel does, y = resize(t) [n, oh, ow, c] and
 * pool = avgpool2(y), and optionally pool2 = avgpool2(pool) [n, oh / 4, ow / 4, c] (the pyramid's
 * next level), without writing x2 or t. bf16 tensors; c in {32, 64}, h * w % 16 == 0,
 * 2 * h * w * c * 2 (+ (oh / 2) * (ow / 2) * c * 2 with pool2) <= 64 KiB, 16-B aligned. */
int comet_conv1x1_resize_pool_nhwc(const void* x, const void* up1, int64_t h1, int64_t w1, const void* up2,
                                   int64_t h2, int64_t w2, const void* weight, const float* bias, void* y,
                                   void* pool, void* pool2, int64_t n, int64_t c, int64_t h, int64_t w,
                                   int64_t oh, int64_t ow, void* stream);
/* The fine ShallowEncoder's front (blocks.py:114-196 with modules.py:39-116): conv1 + InstanceNorm +
 * ReLU and the two stride-2 ResidualBlocks in one kernel, bit for bit the seven comet_conv2d_nhwc
 * (narrow kernel) and seven comet_instnorm_nhwc (one wave per image) calls it replaces, with no map
 * but the three results in HBM. patches [n, 31, 31, 8] (RGB zero-padded to 8 channels), x
 * [n, 16, 16, 32], tmp1 [n, 8, 8, 32], tmp2 [n, 4, 4, 32]: the tensors comet_conv1x1_resize_pool_nhwc
 * reads. weights[7] / biases[7] (host arrays of device pointers) in the order conv1, layer1.conv1,
 * layer1.conv2, layer1.downsample, layer2.conv1, layer2.conv2, layer2.downsample: dense bf16
 * [32, kh * kw * cin] with columns (ky, kx, ci) (conv1's cin padded to 8) and f32 [32]. dtype must be
 * COMET_BF16, p == 31, c == 8, n < 2^31 / 256, tensors and weights 16-B aligned. */
int comet_shallow_front_nhwc(int dtype, const void* patches, const void* const* weights,
                             const float* const* biases, void* x, void* tmp1, void* tmp2, int64_t n,
                             int64_t p, int64_t c, float eps, void* stream);
/* NHWC resize into a channel slice of a wider NHWC tensor (output pixel pitch ldy elements):
 * BasicEncoder's four up-sampled maps land directly in their torch.cat(dim=1) positions
 * (blocks.py:97-107), so the 416-channel concat is never copied. c, ldy % 8 == 0. */
int comet_resize_bilinear_nhwc_into(int dtype_in, int dtype_out, const void* x, void* y, int64_t n,
                                    int64_t c, int64_t h, int64_t w, int64_t oh, int64_t ow,
                                    int64_t ldy, int add, void* stream);

/* ---------------------------------------------------------------------------------------
 * Camera head (camera_predictor10.py:329-484) and encoders.
 * ------------------------------------------------------------------------------------- */
/* y = act(x) elementwise (ReLU / GELU / sigmoid of the T_P gating MLPs) */
int comet_act_fwd(int act, int dtype_x, int dtype_y, const void* x, void* y, int64_t n, void* stream);
/* op 0: y = a + b; 1: y = relu(a + b); 2: y = a * b (same dtype, same shape) */
int comet_binary(int op, int dtype, const void* a, const void* b, void* y, int64_t n, void* stream);
/* y[r, c] = x[r, c] + table[r % period, c] (positional / time embeddings, table f32) */
int comet_add_rows(int dtype_x, int dtype_y, const void* x, const float* table, void* y, int64_t rows,
                   int64_t cols, int64_t period, int64_t ldx, int64_t ldy, void* stream);
/* T_P confidence gating traj * w (camera_predictor10.py:332-333): y[r, :] = x[r, :] * w[r];
 * backward dx = dy * w, dw[r] = <dy[r], x[r]> (dx / dw may be NULL) */
int comet_rowscale_fwd(int dtype, const void* x, const float* w, void* y, int64_t rows, int64_t cols,
                       void* stream);
int comet_rowscale_bwd(int dtype, const void* x, const float* w, const float* dy, float* dx, float* dw,
                       int64_t rows, int64_t cols, void* stream);
/* 1-D sin/cos table (utils.py:807-832, double math, f32 out): out[m*ld + col0 + d] */
int comet_sincos_table(const float* pos, float* out, int64_t m, int dim, int64_t ld, int64_t col0,
                       void* stream);
/* HarmonicEmbedding (minipytorch3d/harmonic_embedding.py:127-158): x [rows, dim], optional
 * diag_cov [rows, dim], freqs [n] -> y [rows, dim*(2n + append)]; backward gives dx, dcov. */
int comet_harmonic_fwd(const float* x, const float* diag_cov, const float* freqs, float* y, int64_t rows,
                       int dim, int n_freqs, int append_input, void* stream);
int comet_harmonic_bwd(const float* x, const float* diag_cov, const float* freqs, const float* dy,
                       float* dx, float* dcov, int64_t rows, int dim, int n_freqs, int append_input,
                       void* stream);
/* camera_to_pose_encoding2 per sequence (utils.py:631-688): R [B*S,4], T_uvz [B*S,3],
 * focal [B*S,2] -> enc [B*S,8]; ratio as in the reference (float64): the host value, or, when
 * ratio_dev is non-NULL, the float64 read from that device address (no host sync for a ratio that
 * already lives in HBM). */
int comet_pose_encode(const float* R, const float* T_uvz, const float* focal, double ratio,
                      const double* ratio_dev, float* enc, int64_t B, int S, void* stream);
/* pose_encoding_to_camera2 per sequence (utils.py:312-403): enc [B*S,7] -> R [B*S,4] (f32),
 * T [B*S,3] (f64, as the reference's float64 promotion), intrinsics fx, fy, cx, cy. */
int comet_pose_decode(const float* enc, const float* R_gt, const float* T_uvz_gt, double ratio,
                      const double* ratio_dev, double fx,
                      double fy, double cx, double cy, float* R_out, double* T_out, int64_t B, int S,
                      void* stream);
/* Single-head ablations (camera_predictor_abl_uvz.py / _abl_all.py): camera_to_pose_encoding3
 * (utils.py:591-627) per sequence: enc [B*S,8] = (T_i - T_0 in xyz, q_i * q_0^-1 standardised,
 * 0 padding; frame 0 = (0,0,0,1,0,0,0,0)) -- the GAPR kernels take it like encoding 2; and
 * pose_encoding_to_camera3 (utils.py:270-310): enc [B*S,7] -> R = dq * q_0, T = T_0 + dxyz (f32). */
int comet_pose_encode3(const float* R, const float* T, float* enc, int64_t B, int S, void* stream);
int comet_pose_decode3(const float* enc, const float* R_gt, const float* T_gt, float* R_out, float* T_out,
                       int64_t B, int S, void* stream);
/* GAPR head + pose loss (camera_predictor10.py:385-460): F.normalize(rot, eps 1e-8), loss =
 * w_trans*100*MSE(uvd[1:]) + w_rot*100*MSE(q[1:]) (mean over sequences), frame-0 reset.
 * gt_enc may be NULL (no loss). qn [B*S,4] is kept for the backward. */
int comet_gapr_fwd(const float* rot, int64_t ld_rot, const float* uv, int64_t ld_uv, const float* d,
                   int64_t ld_d, const float* gt_enc, float* qn, float* enc, float* losses, int B, int S,
                   float w_trans, float w_rot, void* stream);
/* dlosses[3] = upstream grads of (loss, loss_trans, loss_rot) (device) -> drot [B*S,4],
 * duv [B*S,2], dd [B*S,1] */
int comet_gapr_bwd(const float* rot, int64_t ld_rot, const float* uv, int64_t ld_uv, const float* d,
                   int64_t ld_d, const float* gt_enc, const float* qn, const float* dlosses, float* drot,
                   float* duv, float* dd, int B, int S, float w_trans, float w_rot, void* stream);

/* ---------------------------------------------------------------------------------------
 * Point tracker (base_track_predictor.py, blocks.py:351-429, refine_track.py) and DINOv2 input.
 * Feature maps are NHWC [n, H, W, C]; track state is [B, N, S, .] (row t = (b*N + n)*S + s).
 * ------------------------------------------------------------------------------------- */
/* sample_features4d / bilinear_sampler (utils.py:874-974): align_corners=True pixel coords,
 * border (1) or zeros (0) padding; out f32 [B, R, C] (element strides given). */
int comet_sample_bilinear(int dtype, const void* fmap, int64_t bstride, int H, int W, int C,
                          const float* coords, int64_t cstride_b, int64_t cstride_r, float* out,
                          int64_t ostride_b, int64_t ostride_r, int64_t B, int64_t R, int border,
                          void* stream);
/* CorrBlock.corr + .sample fused (blocks.py:376-429): pyramid[l] NHWC [B*S, H_l, W_l, C],
 * feats f32 [B*N*S, C], coords f32 [B*N*S, 2] (level-0 units) -> out[t*ldo + col0 + l*(2r+1)^2 + k] */
int comet_corr_sample(int dtype_fmap, int dtype_feat, const void* const* pyramid, const int* heights,
                      const int* widths, int levels, int radius, int C, const void* feats,
                      const float* coords, float* out, int64_t ldo, int64_t col0, int64_t B, int64_t N,
                      int S, void* stream);
/* transformer input (base_track_predictor.py:170-221): [flow emb | flows | corr | feats | pad] + pos,
 * tdim columns at row pitch ldx >= tdim; columns tdim..ldx-1 are written as zeros (rows padded to
 * the consuming GEMM's 64-deep k-tile; ldx > tdim needs tdim, ldx % 4 == 0 and 16-B aligned pos). */
int comet_tracker_tokens(int dtype_out, const float* coords, const float* feats, int latent,
                         const float* corr, int64_t ldcorr, int corrdim, const float* pos, int tdim,
                         void* x, int64_t ldx, int64_t rows, int S, void* stream);
/* coords += delta[:, :2] (frame 0 pinned); preds [B, S, N, 2] = coords * scale (may be NULL) */
int comet_coords_update(int dtype_delta, float* coords, const void* delta, int64_t ldd, float* preds,
                        float scale, int64_t B, int64_t N, int S, void* stream);
/* F.avg_pool2d(2, 2) on NHWC (CorrBlock pyramid, blocks.py:369-374) */
int comet_avgpool2_nhwc(int dtype, const void* x, void* y, int64_t n, int H, int W, int C, void* stream);
/* refine_track.py:74-131: patches NHWC [B*N*S, P, P, cpad] in (b, n, s) order (RGB in channels
 * 0..2, channels 3..cpad-1 zero: cpad 8 lets the first conv run as an implicit GEMM), topleft
 * [B,S,N,2] (int, unclamped), query [B*N,2] = frac(coarse[:, 0]) + pradius. Both patch origins
 * are clamped to [0, H - P] (the reference uses H for x as well), so the entry point requires
 * H >= P and W >= H and returns COMET_EINVAL otherwise (W < H would read past the row); track
 * coordinates must not be NaN. */
int comet_patch_gather(int dtype_out, const float* images, const float* coarse, void* patches,
                       int* topleft, float* query, int64_t B, int S, int64_t N, int H, int W,
                       int pradius, int cpad, void* stream);
/* track_predictor.py:117-143: RGB NCHW f32 [n,3,H,W] -> [n, oh, ow, cpad] (channels 3.. zero),
 * align_corners bilinear resize when (oh, ow) != (H, W) (the x1/down_ratio interpolate). */
int comet_images_nhwc(int dtype_out, const float* images, void* out, int64_t n, int H, int W, int oh,
                      int ow, int cpad, void* stream);
/* refined[b,s,n] = fine[(b*N+n), s] + topleft[b,s,n]; frame 0 = coarse query (refine_track.py:143-153) */
int comet_refine_combine(const float* fine, const int* topleft, const float* coarse, float* refined,
                         int64_t B, int S, int64_t N, void* stream);
/* compute_score_fn + score inversion (refine_track.py:174-278, E2Epose2.py:232-236):
 * qfeat [B*N, C], pfeat NHWC [B*N, S, P, P, C], fine [B*N, S, 2] -> score, inv_score [B, S, N] */
int comet_track_score(int dtype_feat, const float* qfeat, const void* pfeat, const float* fine,
                      float* score, float* inv_score, int64_t B, int S, int64_t N, int P, int C,
                      int sradius, void* stream);
/* camera_predictor10.py:624-634 + DINOv2 patch_embed im2col: images [BS,3,H,W] -> resize to
 * R (align_corners) -> (x-mean)/std -> cols [BS*(R/p)^2, ldc], column ci*p*p + ky*p + kx */
int comet_dino_prep(int dtype_out, const float* images, void* cols, int64_t BS, int H, int W, int R,
                    int patch, int64_t ldc, const float* mean3, const float* std3, void* stream);

/* ---------------------------------------------------------------------------------------
 * Evaluation metrics (comet/models/metric.py; called by the eval block of
 * train_eval_func_new_cp5.py:633-671). f32, one thread per pair / frame.
 * comet_pose_pair_errors: camera_to_rel_deg3's all-pairs part (metric.py:214-245): world-to-view
 *   matrices [batch*frames, 4, 4] (PyTorch3D layout [[R, 0], [T, 1]], get_matrix()), pairs i < j of
 *   each sequence in torch.combinations order -> rotation_angle / translation_angle in degrees,
 *   [batch * frames*(frames-1)/2] each (metric.py:561-570, 611-701).
 * comet_pose_frame_errors: camera_to_rel_deg2 (the definition bound last, metric.py:391-451) per
 *   frame: translation_angle(gt[:, :3], pred[:, :3]) in degrees, geodesic angle of Rp·Rgᵀ in radians
 *   (metric.py:326-347) and the Euler angles of Rp·Rgᵀ [n, 3] (metric.py:302-323), from pose
 *   encodings pred [n, ld_pred >= 7] (u, v, d, qw, qx, qy, qz) and gt [n, ld_gt >= 7].
 * ------------------------------------------------------------------------------------- */
int comet_pose_pair_errors(const float* pred_w2v, const float* gt_w2v, int64_t batch, int64_t frames,
                           float* rot_deg, float* trans_deg, void* stream);
int comet_pose_frame_errors(const float* pred_enc, int64_t ld_pred, const float* gt_enc, int64_t ld_gt,
                            int64_t n, float* trans_deg, float* geo_rad, float* euler, void* stream);

/* ---------------------------------------------------------------------------------------
 * Data path (YTDataset.load_images_from_folder, kubric_movif_SFM_dataset_YT.py:236-266):
 * PIL Image.crop (black outside the frame) + Image.resize(crop_size, LANCZOS) + ImageNet
 * normalisation, byte-exact with Pillow's Resample.c.
 * comet_resample_coeffs (host): Pillow's precompute_coeffs + normalize_coeffs_8bpc for LANCZOS
 *   over the source span [in0, in1) of in_size pixels -> bounds [out_size*2] (first source pixel,
 *   tap count), coeffs [out_size*max_ksize] int32 (22 fraction bits); coeffs == NULL: only the
 *   table width *ksize.
 * comet_lanczos_crop_resize (device): frames [n][h][w][3] uint8 (frame_stride bytes apart), crop
 *   box origin (x0, y0) size (cw, ch), output (ow, oh): horizontal pass over crop rows
 *   ybase .. ybase + rows - 1 (bx / kx, width ksx; skipped when ow == cw) into tmp
 *   [n][rows][ow][3] uint8, vertical pass (by rebased to ybase / ky, width ksy; skipped when
 *   oh == ch) -> out [n][3][oh][ow] f32 = (u / 255 - mean[c]) / std[c]. */
int comet_resample_coeffs(int in_size, float in0, float in1, int out_size, int32_t* bounds, int32_t* coeffs,
                          int max_ksize, int* ksize);
int comet_lanczos_crop_resize(const uint8_t* frames, int64_t n, int h, int w, int64_t frame_stride, int x0, int y0,
                              int cw, int ch, int ow, int oh, const int32_t* bx, const int32_t* kx, int ksx,
                              const int32_t* by, const int32_t* ky, int ksy, int ybase, int rows, uint8_t* tmp,
                              const float* mean, const float* stdv, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Keypoint initialisation (train_eval_func_new_cp5.py:527-595: lightglue SuperPoint.extract on
 * frame 0, then filter_and_pad): the SuperPoint encoder / detector convolutions run on
 * comet_conv2d_nhwc; these are its other dense stages.
 * comet_sp_preprocess: x [B,3,H,W] f32 -> bilinear (align_corners=False) resize to OH x OW
 *   (up-sampling only) + grayscale (0.299, 0.587, 0.114) -> y [B,OH,OW,cpad] (channel 0; rest 0).
 * comet_maxpool2_nhwc: nn.MaxPool2d(2, 2) on NHWC.
 * comet_sp_scores: detector logits [B,h,w,65] f32 -> softmax, dustbin dropped, depth-to-space
 *   -> scores [B, 8h, 8w].
 * comet_maxfilt2d: (2r+1)^2 stride-1 max filter of [B,H,W] f32 (max_pool2d with padding r),
 *   tmp = B*H*W floats of workspace (simple_nms; filter_and_pad's 3x3 mask dilation). */
int comet_sp_preprocess(int dtype_y, const float* x, void* y, int B, int H, int W, int OH, int OW, int cpad,
                        void* stream);
int comet_maxpool2_nhwc(int dtype, const void* x, void* y, int64_t n, int H, int W, int C, void* stream);
int comet_sp_scores(const float* logits, float* scores, int B, int h, int w, void* stream);
int comet_maxfilt2d(const float* x, float* y, float* tmp, int B, int H, int W, int r, void* stream);

/* ---------------------------------------------------------------------------------------
 * SIFT (difference-of-Gaussians) keypoint detector, the second detector of the keypoint
 * initialisation (train_eval_func_new_cp5.py:527-531: lightglue SIFT = OpenCV's detector; the
 * algorithm, not a bit copy: DESIGN.md §11). Images are contiguous [B, H, W]; one launch serves all B.
 * comet_sift_base: gray uint8 [B,H,W] -> octave-0 base image f32 [B,2H,2W]: 2x bilinear up-sample
 *   (src = (dst + 0.5) / 2 - 0.5, edge-clamped), then a blur of sigma = sqrt(1.6^2 - (2 * 0.5)^2).
 * comet_gauss_blur: separable Gaussian blur of f32 [B,H,W] (x != y): radius r = (round(8 sigma + 1) | 1) / 2,
 *   taps exp(-x^2 / 2 sigma^2) normalised to sum 1 (computed in double on the host), reflect-101
 *   border. COMET_EINVAL when r > 10 (sigma > ~2.56), the halo the kernel's LDS tile holds.
 * comet_downsample2: y [B,H/2,W/2] = every second pixel of every second row of x [B,H,W].
 * comet_sift_detect: one octave. gauss = its n_layers + 3 Gaussian images [B, n_layers + 3, h, w].
 *   Every DoG extremum inside the 5-px border that survives the sub-pixel refinement (at most 5
 *   Newton steps), the contrast test (|contr| * n_layers >= contrast_threshold) and the edge test is
 *   appended to cand [B, cap, 8] f32 (16-byte aligned) as (x, y, size, response, number of
 *   orientation-histogram peaks, octave, layer, 0), x / y / size in base-image pixels
 *   (x 2^octave). count [B] int32 (zeroed by the caller before the first octave) is advanced by
 *   one atomic add per keypoint -- the order of the records is not defined; when an image has
 *   more than cap keypoints, *overflow (int32, zeroed by the caller) is set and the surplus is
 *   not written. sigma: the scale of layer 0 (1.6). */
int comet_sift_base(const uint8_t* gray, float* base, int B, int H, int W, void* stream);
int comet_gauss_blur(const float* x, float* y, int B, int H, int W, float sigma, void* stream);
int comet_downsample2(const float* x, float* y, int B, int H, int W, void* stream);
int comet_sift_detect(const float* gauss, int B, int n_layers, int h, int w, int octave,
                      float contrast_threshold, float edge_threshold, float sigma, float* cand, int cap,
                      int* count, int* overflow, void* stream);

/* ---------------------------------------------------------------------------------------
 * Online inference (comet_amd/stream.py, DESIGN.md "Online / streaming inference"): the per-frame
 * tensors of the newest `capacity` frames are kept in device rings of equal-sized slots.
 * comet_ring_gather: for each of n_tensors (1..COMET_RING_MAX_TENSORS) rings,
 *   dst[j*slot_bytes : (j+1)*slot_bytes] = src[slots[j]*slot_bytes : ...] for j in [0, T), all rings
 *   in ONE launch (16-B vector loads, streaming stores, a grid-stride loop over 16 KiB tiles sized
 *   to the CU count). `slots` is the window's slot table on the device (int32 [T]); `slots_host`
 *   holds the same T values on the host and is range-checked against `capacity` before the launch
 *   (the kernel skips a slot outside [0, capacity) instead of reading it). slot_bytes must be a
 *   multiple of 16 and src / dst 16-B aligned. max_blocks: 0 = 4 workgroups per CU, > 0 caps the
 *   grid (tests: several grid passes at small sizes). */
#define COMET_RING_MAX_TENSORS 4
typedef struct CometRingTensor {
  const void* src;     /* ring: capacity slots of slot_bytes */
  void* dst;           /* window: T slots of slot_bytes, contiguous */
  int64_t slot_bytes;
} CometRingTensor;
int comet_ring_gather(const CometRingTensor* tensors, int n_tensors, const int32_t* slots,
                      const int32_t* slots_host, int T, int capacity, int max_blocks, void* stream);
/* comet_ring_scatter: the inverse, for the k new frames of a push (comet_amd.stream.StreamPool: one
 *   frame per stream). Here `src` is a contiguous block of k rows of slot_bytes and `dst` the ring:
 *   dst[slots[j]*slot_bytes : ...] = src[j*slot_bytes : (j+1)*slot_bytes] for j in [0, k), all rings
 *   in ONE launch (same tiling and grid; plain stores: the gather of the same push reads the slots
 *   again). slots / slots_host as above; besides the range check the k host values must be distinct
 *   (two rows for one slot would race). The kernel skips a slot outside [0, capacity) instead of
 *   writing it. */
int comet_ring_scatter(const CometRingTensor* tensors, int n_tensors, const int32_t* slots,
                       const int32_t* slots_host, int k, int capacity, int max_blocks, void* stream);

/* comet_pose_fuse (DESIGN.md "Pose fusion"): with stride < window a frame lies in several windows;
 *   this keeps one accumulator row per ring slot and returns, for every frame of the n hops of a
 *   push, ONE fused pose with a count and a spread, in one launch. acc [rows, COMET_FUSE_ROW] f64,
 *   row of frame f of stream s = s * capacity + f % capacity (the slot numbering of the frame
 *   rings, so `slots` / `slots_host` are the gather's tables, n * T entries). Row layout:
 *     0 W = sum w | 1..10 upper triangle of sum w q q^T (ww wx wy wz xx xy xz yy yz zz, q unit, in
 *     double) | 11..13 sum w (u, v, z) | 14..16 sum w (u^2, v^2, z^2) | 17 count | 18, 19 zero.
 *   enc [n * T, 7] f32, relative to each window's first frame. Per hop h: first[h] = 1 for a
 *   stream's first hop (the reference is anchors[h] = (q[4], u, v, z) f64, which also becomes row
 *   slots[h * T] as one hypothesis of weight 1), else 0 (the reference is the fused pose of row
 *   slots[h * T]; anchors[h] is not read); fresh_from[h] = 1 for a first hop, T - stride afterwards.
 *   One thread per (h, i): hypothesis q = normalise(enc[3:7] (x) q_ref), w >= 0; u = u_ref +
 *   e0 / ratio * 128, v likewise, z = z_ref * (e2 / ratio + 1), all double (the codec's composition,
 *   comet_pose_decode). For i >= 1 the row is overwritten by the hypothesis when i >= fresh_from[h],
 *   else the hypothesis is added; position 0 is written by a first hop only. weights [n * T] f32 > 0
 *   or NULL (= 1). ratio / ratio_dev as comet_pose_decode. Outputs per (h, i), from the row after
 *   the update: R [4] f32 = eigenvector of the largest eigenvalue of the 4 x 4 matrix (fixed-sweep
 *   cyclic Jacobi in double; lowest index among equal eigenvalues; w >= 0), uvz [3] f64 = sum w x / W,
 *   T [3] f64 = ((u - cx) z / fx, (v - cy) z / fy, z), count int32, rot_spread f32 =
 *   2 asin(sqrt(max(0, 1 - lambda_max / W))) rad, trans_spread [3] f32 = sqrt(max(0, E[x^2] - E[x]^2));
 *   and the window's own hypothesis hyp_R [4] f32, hyp_T [3] f64 (as T, from the hypothesis).
 *   COMET_EINVAL before anything is launched: a null pointer (weights and ratio_dev may be null),
 *   n <= 0, T < 2, rows <= 0, fresh_from outside [1, T], first not 0 / 1 or 1 with fresh_from != 1,
 *   a host slot outside [0, rows), two equal host slots (two positions for one row would race; a
 *   stream completes at most one hop per push), a host ratio that is not finite and positive. The
 *   kernel skips a slot outside [0, rows) and writes only inside acc and the outputs. */
#define COMET_FUSE_ROW 20
int comet_pose_fuse(const float* enc, const int32_t* slots, const int32_t* slots_host,
                    const int32_t* fresh_from, const int32_t* fresh_from_host, const int32_t* first,
                    const int32_t* first_host, const double* anchors, const float* weights, double ratio,
                    const double* ratio_dev, double fx, double fy, double cx, double cy, double* acc,
                    int rows, int n, int T, float* R_out, double* uvz_out, double* T_out,
                    int32_t* count_out, float* rot_spread, float* trans_spread, float* hyp_R,
                    double* hyp_T, void* stream);

/* comet_track_carry (DESIGN.md "Track carry"): the query points of the n hops of a push from the
 *   previous windows' tracks, one launch, one workgroup of 256 threads per hop (no communication
 *   between workgroups, no global atomics; every selection is order-independent, so the result is
 *   deterministic). Per hop b:
 *     tracks [n, T, N, 2] f32, score [n, T, N] f32: pred_tracks / pred_score of the previous window
 *       (score as the model returns it, larger is better); only row s (= stride) is read.
 *     ids, age [n, N] int32: the previous ids and ages; id < 0 marks a slot that holds no track.
 *     mask [n, H, W] uint8 or NULL: object mask of the new first frame.
 *     cand [n, M, 2] f32 (NULL only when M == 0): candidates in detector order, best first;
 *     cand_n [n] int32 on the device: valid candidates of the hop (clamped to [0, M]).
 *     next_id [n] int32: the hop's id counter, read and written.
 *     prev_valid [n] int32: 0 on a stream's first hop -- tracks and score are not read, every slot
 *       counts as dead.
 *   Rules:
 *   1. Alive: x and y finite; border <= x <= W - 1 - border and border <= y <= H - 1 - border; with
 *      a mask, mask[clamp(rint(y), 0, H - 1), clamp(rint(x), 0, W - 1)] != 0 (rint: round half to
 *      even, the indexing of filter_and_pad). A previous track also needs id >= 0 and
 *      score[b, s, j] >= min_score (a NaN score is dead).
 *   2. One track per cell: cell = (floor(x / cell), floor(y / cell)) in f32 on a grid of
 *      ceil(W / cell) x ceil(H / cell). Every alive point posts a 32-bit key with an LDS atomicMin:
 *      a previous track (2^19 - 1 - clamp(age, 0, 2^19 - 1)) << 12 | j (bit 31 clear), a candidate
 *      1 << 31 | c. A point is kept iff its key is its cell's minimum: a track beats any candidate,
 *      among tracks the older wins, then the lower slot; among candidates the lower index.
 *   3. A kept track stays in slot j with its id; age_out = age + 1 (saturating at INT32_MAX, a
 *      negative age counts as 0); query[b, j] = tracks[b, s, j] bit for bit; src = j.
 *   4. Births: the r-th free slot (ascending j) takes the r-th kept candidate (ascending c), ranks
 *      by exclusive prefix sums over the workgroup in chunks of 256 with a carry: query = cand[b, c],
 *      id = next_id + r, age = 0, src = -1 - c. next_id grows by the number born.
 *   5. Pads: with the live slots (kept and born) l_0 < ... < l_{L-1}, the r-th slot still free
 *      (ascending j) copies the query of l_{r mod L}: id = -1, age = 0, src = INT32_MIN + l. If
 *      L == 0 it is a lattice point, g = ceil(sqrt(N)), in f32 evaluated left to right
 *        x = ((float)(r % g) + 0.5f) * (float)W / (float)g,  y = ((float)(r / g) + 0.5f) * (float)H / (float)g,
 *      id = -1, src = INT32_MIN. A pad has id < 0, so the next hop treats its slot as free.
 *   Outputs: query [n, N, 2] f32; ids_out, age_out, src [n, N] int32; stats [n, 4] int32 =
 *   (survivors, born, padded, alive tracks dropped by rule 2). ids_out == ids and age_out == age
 *   (in place) is allowed: a slot is read and written by one thread, reads first.
 *   LDS: 32 KiB of keys (8192 cells) + 16 KiB rank list + 4 KiB slot states, static.
 *   COMET_EINVAL before anything is launched: a null pointer (mask may be null; cand only when
 *   M == 0), n < 1, N outside [1, 4096], M outside [0, 65536], s outside [1, T - 1], H or W < 1,
 *   cell < 1, border < 0, more than 8192 grid cells, tracks / cand / query not 8-B aligned. Slot and
 *   candidate indices are range-checked in the kernel before they address memory. */
#define COMET_CARRY_MAX_TRACKS 4096
#define COMET_CARRY_MAX_CANDIDATES 65536
#define COMET_CARRY_MAX_CELLS 8192
int comet_track_carry(const float* tracks, const float* score, const int32_t* ids, const int32_t* age,
                      const uint8_t* mask, const float* cand, const int32_t* cand_n, int32_t* next_id,
                      const int32_t* prev_valid, int n, int T, int N, int M, int s, int H, int W, int cell,
                      int border, float min_score, float* query, int32_t* ids_out, int32_t* age_out,
                      int32_t* src, int32_t* stats, void* stream);

/* comet_track_warm (DESIGN.md "Warm start"): the coarse tracker's starting coordinates for the n
 *   hops of a push, one launch, one thread per slot (grid-stride, 256 threads per workgroup, no
 *   LDS, no atomics, no communication between threads). With stride s < T the previous window has
 *   already tracked T - s of the new window's T frames; a slot that comet_track_carry carried starts
 *   on those positions instead of on its query point in every frame.
 *     prev [n, T, N, 2] f32 pixels: pred_tracks of the previous windows (the `tracks` argument of the
 *       comet_track_carry call of this push).
 *     src [n, N] int32, query [n, N, 2] f32 pixels: the outputs of that comet_track_carry call.
 *     prev_valid [n] int32: as for comet_track_carry; 0 -- prev is not read, every slot is cold.
 *     s: the stride, 1 <= s <= T - 1. mode: 0 hold, 1 constant velocity.
 *     div0, div1: the predictor's two divisions (down_ratio, then stride); 1 and 1 when it divides
 *       by nothing.
 *   Per hop b and slot j:
 *   Donor. prev_valid[b] == 0: none. 0 <= src[j] < N: k = src[j] (a carried slot). src[j] =
 *     INT32_MIN + l with 0 <= l < N (a pad copy): l iff src[l] == l; the lattice pad (src = INT32_MIN
 *     itself) falls under this with l = 0 and stays cold, since slot 0 is then not carried. Anything
 *     else (births -M <= src < 0, values outside every range): none. Every index is range-checked
 *     before it addresses memory.
 *   Warm row of donor k, in pixels: frame 0 = query[b, j] bit for bit; frame i in [1, T - 1 - s] =
 *     prev[b, i + s, k]; frame i > T - 1 - s, with e = i - (T - 1 - s), last = prev[b, T - 1, k] and
 *     before = prev[b, T - 2, k]: hold -- last; velocity -- last + (float)e * (last - before) in f32,
 *     one rounding per operation (no contraction), then clamped by v < 0 ? 0 : (v > hi ? hi : v) with
 *     hi = W - 1 for x and H - 1 for y. If any of the row's 2 T values is not finite before the clamp,
 *     the slot falls back to a cold row (a value of prev that the row does not use may be anything).
 *   Cold row: query[b, j] in every frame, what the predictor starts from without this kernel.
 *   Units: every value is divided by div0 and then by div1 in f32 (IEEE division). For divisors that
 *     are powers of two (the model's 2 and 4) a cold row is bit-identical to torch's q / down_ratio /
 *     stride; torch multiplies by the reciprocal of a scalar divisor, which can differ in the last bit
 *     for other divisors.
 *   Outputs: coords [n, N, T, 2] f32 (the layout the predictor iterates on); warm [n, N] int32: 0 cold,
 *     1 carried, 2 pad copy of a carried slot, -1 fallen back (a non-finite value).
 *   COMET_EINVAL before anything is launched, checked in this order: a null pointer, n < 1, N outside
 *   [1, COMET_CARRY_MAX_TRACKS], T < 2, s outside [1, T - 1], H or W < 1, mode not 0 or 1, div0 or
 *   div1 not finite or <= 0, prev / query / coords not 8-B aligned. */
int comet_track_warm(const float* prev, const int32_t* src, const float* query,
                     const int32_t* prev_valid, int n, int T, int N, int s, int H, int W, int mode,
                     float div0, float div1, float* coords, int32_t* warm, void* stream);

/* comet_landmark_update (DESIGN.md "Landmarks"): a carried track, seen over the frames whose fused
 *   pose is final, is a multi-view triangulation problem; this keeps its normal equations and returns
 *   a 3-D point in the body frame for every query slot of the n hops of a push, one launch, one thread
 *   per (hop h, slot j), grid (ceil(N / 256), n), no LDS, no atomics, no communication between threads.
 *   Everything is IEEE double evaluated as written (no contraction).
 *   State: acc [rows, COMET_LM_ROW] f64 and acc_id [rows] int32, rows = streams * N; the row of slot j
 *   of the stream of hop h is stream_idx[h] * N + j. Row layout:
 *     0..5 upper triangle of M = sum w a a^T (xx xy xz yy yz zz) | 6..8 g = sum w a c | 9 sum w c^2 |
 *     10 frames added | 11 zero.
 *   Inputs per hop: tracks [n, T, N, 2] f32 pixels (pred_tracks); weights [n, T, N] f32 or NULL (= 1);
 *     R [n, T, 4] f32 quaternions (w first) and T [n, T, 3] f64, the fused_R / fused_T of
 *     comet_pose_fuse; ids, src [n, N] int32 as comet_track_carry returned them for this hop;
 *     intr [n, 4] f64 = (fx, fy, cx, cy) of the pixels the tracks live in.
 *   Observation of the frame at window position i: Rm = the matrix of R[h, i] (the formula of
 *     minipytorch3d.quaternion_to_matrix; its transpose when inverse_rotation = 1), rows r1 r2 r3,
 *     x_cam = Rm X + T. With xn = (x - cx) / fx, yn = (y - cy) / fy the two equations a . X = c are
 *     a = r1 - xn r3, c = xn tz - tx and a = r2 - yn r3, c = yn tz - ty, each added with weight w. A frame
 *     whose x, y or w is not finite, or whose w <= 0, adds nothing.
 *   Frames: a hop commits the positions [0, s), s = stride: the frames that leave the window after this
 *     hop, whose fused pose is final; every frame of a stream is committed exactly once.
 *   Reset rule: ids[j] < 0 (a pad): the row is zeroed, acc_id = -1, state 0. src[j] != j (born) or
 *     acc_id[row] != ids[j]: the row is overwritten by this hop's observations, acc_id = ids[j]. Otherwise
 *     the observations are added.
 *   Solve, after the update: M X = g by an unpivoted LDL^T. Outputs per (h, j): X [3] f64; n_obs int32;
 *     err_px f32, the pixel distance between tracks[h, s, j] and the projection of X with the pose of
 *     position s (the frame that becomes the next window's first); state int32: 1 valid | 0 no landmark
 *     (a pad, or n_obs < min_obs) | 2 ill-conditioned (a pivot <= min_pivot * max(diag M)) | 3 behind the
 *     camera (r3 . X + tz <= 0 at position s) | -1 a non-finite X or err_px. For every state other than 1,
 *     X is 0 and err_px is +inf.
 *   COMET_EINVAL before anything is launched, checked in this order: a null pointer (weights may be
 *   null), n < 1, N outside [1, 4096], T < 2, s outside [1, T - 1], rows < n * N, a host stream index
 *   outside [0, rows / N) or two equal ones (two hops on one row would race; a stream completes at most
 *   one hop per push), host intrinsics whose fx or fy is not finite and positive, inverse_rotation not 0
 *   or 1, min_obs < 2, min_pivot outside [0, 1), tracks / T / intr / X not 8-B aligned or R / acc not
 *   16-B aligned. The kernel range-checks every row index before it addresses memory. */
#define COMET_LM_ROW 12
int comet_landmark_update(const float* tracks, const float* weights, const float* R, const double* T,
                          const int32_t* ids, const int32_t* src, const int32_t* stream_idx,
                          const int32_t* stream_idx_host, const double* intr, const double* intr_host,
                          double* acc, int32_t* acc_id, int rows, int n, int Tw, int N, int s,
                          int inverse_rotation, int min_obs, double min_pivot, double* X, int32_t* n_obs,
                          float* err_px, int32_t* state, void* stream);

/* comet_landmark_reid (DESIGN.md "Landmark archive"): comet_landmark_update forgets a landmark when its
 *   track dies. This keeps the row of a dying track in a per-stream archive and hands it back, with its
 *   identity, to a track born on its projection. One launch per push for the n hops due, after that push's
 *   comet_pose_fuse and before its comet_landmark_update, on the same stream: grid (n), one workgroup of 256
 *   threads per hop, no communication between workgroups, no global atomics; the result does not depend on
 *   the order threads arrive in. Everything is IEEE double evaluated as written (no contraction), and only
 *   + - * / and sqrt; the solve and the rotation are the text comet_landmark_update uses (csrc/lm_solve.hpp).
 *   State, next to acc [rows, COMET_LM_ROW] / acc_id [rows] of comet_landmark_update (rows >= S N):
 *     arch [entries, COMET_LM_ARCH_ROW] f64, entries >= S C, entry e of stream s at s * C + e: 0..11 the
 *       accumulator row as it was when the track died | 12..14 its solution X | 15..17 the unit view direction
 *       d = (c - X) / |c - X|, c the camera centre in the body frame when it retired | 18..19 zero.
 *     arch_id [entries] int32: the landmark's identity, -1 a free entry. arch_cursor [S] int32: the entry the
 *       next retirement of the stream goes to (a value outside [0, C) is folded into it).
 *     alias [rows] int32: the archived identity the row was restored from, -1 none.
 *     S = min(rows / N, entries / C) streams; C = the archive capacity per stream.
 *   Inputs per hop: tracks [n, T, N, 2] f32, R [n, T, 4] f32, T [n, T, 3] f64, ids / src [n, N] int32,
 *     stream_idx [n] / intr [n, 4] with their host copies: all as comet_landmark_update takes them. Only window
 *     position 0 is read: the frame that was position s of the stream's previous window, whose pose is final;
 *     the last frame a dead track was alive on and the frame a born track's query sits on. Pose: Rm, t as
 *     comet_landmark_update forms them, x_cam = Rm X + t, c_k = 0 - (Rm_0k t_0 + Rm_1k t_1 + Rm_2k t_2).
 *     ws [n, N, COMET_LM_ROW] f64: a workspace (the dying rows, so that every read precedes every write).
 *   Semantics: as if every read of arch, arch_id, acc, acc_id and alias happened before any write.
 *   1. Dying: acc_id[row] >= 0 and (ids[j] != acc_id[row] or src[j] != j): the rows comet_landmark_update is
 *      about to overwrite or clear. A dying row is retirable when the shared solve finds no pivot <=
 *      min_pivot * max(diag M), X is finite, acc[row, 10] >= arch_min_obs and (Rm X + t).z > 0.
 *   2. Match. A born slot has ids[j] >= 0 and src[j] < 0; its pixel is p = tracks[h, 0, j]. An entry of the
 *      hop's stream is a candidate when arch_id >= 0, z = (Rm X_e + t).z > 0, d . d' >= reid_min_cos with
 *      d' = (c - X_e) / |c - X_e| (the sum left to right), and its projection (fx (x / z) + cx, fy (y / z) + cy)
 *      is finite. dist2 = du du + dv dv, (du, dv) = projection - p widened to double. The pick of a born slot
 *      with a finite pixel: the candidate of least dist2 among those with dist2 <= reid_px reid_px, ties to
 *      the lower entry. An entry accepts, of the slots that picked it, the one of least dist2, ties to the
 *      lower slot. A slot is matched iff its pick accepted it. Entries retired in this launch are no
 *      candidates in it (a track the score test or the reprojection gate killed is not resurrected in the
 *      same hop).
 *   3. Writes. Matched slot j <- entry e: acc[row] = arch[e, 0..11], acc_id[row] = ids[j], alias[row] =
 *      arch_id[e], arch_id[e] = -1. A carried row (ids[j] >= 0, src[j] == j, acc_id[row] == ids[j]) keeps its
 *      alias; every other unmatched row: alias[row] = -1. Retirable rows in ascending slot order, r their rank
 *      (an exclusive prefix sum over the workgroup in chunks of 256 with a carry, as comet_track_carry ranks):
 *      entry (cursor + r) mod C takes (row, X, d, 0, 0) and the id alias[row] if that is >= 0, else
 *      acc_id[row]; cursor <- (cursor + count) mod C. Retirements follow the matches: one that lands on an entry
 *      consumed in this launch reuses it, one that lands on an entry in use overwrites it and is counted, and
 *      so is one that lands on an entry an earlier retirement of this launch filled (count > C: the last C
 *      stay).
 *   Outputs, [n, N]: src_lm int32 = src with src_lm[j] = j for matched slots, which comet_landmark_update takes
 *     in place of src, so that it adds to the restored row; lm_id int32, the landmark's identity: the row's
 *     alias after this launch if >= 0, else ids[j] (-1 for a pad); reid_state int32: 0 not a born slot | 1
 *     matched | 2 no candidate within the gate, or a pixel that is not finite | 3 the pick accepted another
 *     slot; reid_dist f32 = sqrt(dist2) of a match, +inf otherwise. stats [n, 4] int32 = (retired, matched,
 *     entries in use afterwards, retirements counted as overwriting).
 *   LDS: 21 C + 12 N bytes, dynamic (132 KiB at C = N = 4096; a gfx950 workgroup may hold 160 KiB) + 656 B
 *   static (the pose, the arguments, the scan and the counters).
 *   COMET_EINVAL before anything is launched, checked in this order: a null pointer, n < 1, N outside
 *   [1, 4096], C outside [1, COMET_LM_ARCH_MAX], T < 2, rows < n * N, entries < n * C, a host stream index
 *   outside [0, S) or two equal ones, host intrinsics whose fx or fy is not finite and positive,
 *   inverse_rotation not 0 or 1, arch_min_obs < 2, min_pivot outside [0, 1), reid_px not finite and positive,
 *   reid_min_cos outside [-1, 1], tracks / T / intr not 8-B aligned or R / acc / arch / ws not 16-B aligned.
 *   The kernel range-checks every row and entry index before it addresses memory. */
#define COMET_LM_ARCH_ROW 20
#define COMET_LM_ARCH_MAX 4096
int comet_landmark_reid(const float* tracks, const float* R, const double* T, const int32_t* ids,
                        const int32_t* src, const int32_t* stream_idx, const int32_t* stream_idx_host,
                        const double* intr, const double* intr_host, double* acc, int32_t* acc_id,
                        int32_t* alias, int rows, double* arch, int32_t* arch_id, int32_t* arch_cursor,
                        int entries, double* ws, int n, int Tw, int N, int C, int inverse_rotation,
                        int arch_min_obs, double min_pivot, double reid_px, double reid_min_cos,
                        int32_t* src_lm, int32_t* lm_id, int32_t* reid_state, float* reid_dist,
                        int32_t* stats, void* stream);

/* comet_landmark_pnp (DESIGN.md "PnP refinement"): the landmarks are 3-D points in the body frame and the
 *   window's tracks their 2-D observations, so every frame of a window has a perspective-n-point problem.
 *   This solves it for every (hop h, window position i) of a push by `iters` Gauss-Newton steps with a
 *   Huber weight, starting from the fused pose, in one launch after that push's comet_pose_fuse and
 *   comet_landmark_update launches: grid (T, n), one workgroup of 256 threads per (i, h), no atomics, no
 *   communication between workgroups. Everything is IEEE double evaluated as written (no contraction), and
 *   only + - * / and sqrt.
 *   Inputs: tracks [n, T, N, 2] f32 pixels; weights [n, T, N] f32 or NULL (= 1); X [n, N, 3] f64 and
 *     state [n, N] int32 as comet_landmark_update wrote them in this push; R0 [n, T, 4] f32 (w first) and
 *     T0 [n, T, 3] f64, the fused pose, the starting point; intr [n, 4] f64 = (fx, fy, cx, cy) of the pixels
 *     the tracks live in, intr_host the same values on the host.
 *   Pose: Rm = the matrix of R0[h, i] by the formula of comet_landmark_update (its transpose when
 *     inverse_rotation = 1), t = T0[h, i], q = R0[h, i] widened to double. Not all finite: state -1.
 *   Usable point j at a pose: state[h, j] == 1; x, y and w finite; w > 0; Xc = Rm X + t has Xc.z > 0.
 *   Residual r = (fx (Xc.x / Xc.z) + cx - x, fy (Xc.y / Xc.z) + cy - y), |r| = sqrt(r0^2 + r1^2); Huber
 *     weight wh = 1 if |r| <= huber_px else huber_px / |r|. Perturbation on the left, in the camera frame:
 *     Xc' = Xc + omega x Xc + upsilon, J = Jproj [ -[Xc]x | I ] (2 x 6); with a0 = fx / z, a1 = fy / z,
 *     c0 = a0 (x / z), c1 = a1 (y / z) its rows are
 *       J0 = (-(c0 y), a0 z + c0 x, -(a0 y), a0, 0, -c0),  J1 = (-(a1 z) - c1 y, c1 x, a1 x, 0, a1, -c1).
 *   Per iteration: a point adds (w wh) (J0_r J0_c + J1_r J1_c) to the upper triangle of H (21 values, row
 *     by row), (w wh) (J0_r r0 + J1_r r1) to b (6 values) and 1 to the usable count. Thread t sums its
 *     slots j = t, t + 256, ... in ascending order from +0; the 256 partials are combined by the fixed
 *     tree p[t] += p[t + d], d = 128, 64, ..., 1 (LDS for d >= 64, wave shuffles below).
 *     A count below min_pts: state 0. A sum that is not finite: state -1.
 *   Solve H delta = -b by an unpivoted LDL^T: column j: c_i = H_ij - sum_{k < j} L_jk U_ik (k ascending),
 *     d_j = c_j, U_ij = c_i, L_ij = c_i / d_j; y_i = -b_i - sum_{k < i} L_ik y_k; delta_i = y_i / d_i -
 *     sum_{k > i} L_ki delta_k (k ascending). A pivot d_j <= min_pivot * max(diag H): state 2.
 *   Update with delta = (omega, upsilon): dq = (1, omega / 2) / sqrt(1 + |omega / 2|^2); Rm <- R(dq) Rm;
 *     t <- R(dq) t + upsilon; q <- dq (x) q (inverse_rotation = 0) or q (x) conj(dq) (1), divided by its
 *     norm with w >= 0. A value of the new pose that is not finite: state -1.
 *   Final pass at the last pose: n_in = usable points with |r| <= huber_px; rms_px = sqrt(sum w (r0^2 +
 *     r1^2) / sum w) over the usable points, summed by the same tree. A usable count below min_pts here:
 *     state 0; rms_px not finite: state -1.
 *   Outputs per (h, i): q [4] f64 (unit, w >= 0), R [4] f32 (q rounded), t [3] f64, n_in int32, rms_px f32,
 *     state int32: 1 solved | 0 fewer than min_pts usable points | 2 degenerate pivot | -1 not finite. For
 *     every state other than 1: R = R0 and t = T0 bit for bit, q = R0 widened, n_in = 0, rms_px = +inf.
 *   Injection (optional): fuse_acc [rows, COMET_FUSE_ROW] f64, the accumulator of comet_pose_fuse, or NULL;
 *     slots [n * T] int32 / slots_host, the tables of that push's comet_pose_fuse call (read only with
 *     fuse_acc); inject_w; (fuse_fx, fuse_fy, fuse_cx, fuse_cy) the fuser's intrinsics. With fuse_acc and
 *     inject_w > 0, thread 0 of a position i in [s, T) with state 1 adds one hypothesis of weight inject_w
 *     to row slots[h * T + i], as comet_pose_fuse adds one: q as returned, (u, v, z) = (cx + fx tx / tz,
 *     cy + fy ty / tz, tz) left to right, every sum of the row layout, count + 1. Nothing is added when
 *     (u, v, z) is not finite. Positions [0, s) are final and never touched; nothing else is written.
 *   COMET_EINVAL before anything is launched, checked in this order: a null pointer (weights may be null;
 *   fuse_acc may be null, and then slots and slots_host may be too), n < 1, N outside [1, 4096], T < 2,
 *   s outside [1, T - 1], iters outside [1, COMET_PNP_MAX_ITERS], huber_px not finite and positive,
 *   min_pts < 4, min_pivot outside [0, 1), inverse_rotation not 0 or 1, host intrinsics whose fx or fy is
 *   not finite and positive; with fuse_acc: inject_w not finite or negative, a host slot outside [0, rows),
 *   two equal host slots; then tracks / X / T0 / intr / q / t not 8-B aligned or R0 / fuse_acc not 16-B
 *   aligned. The kernel range-checks every index before it addresses memory.
 *   LDS: 42 KiB of partial sums + 100 B, static. */
#define COMET_PNP_MAX_ITERS 16
int comet_landmark_pnp(const float* tracks, const float* weights, const double* X, const int32_t* state,
                       const float* R0, const double* T0, const double* intr, const double* intr_host, int n,
                       int Tw, int N, int s, int inverse_rotation, int iters, double huber_px, int min_pts,
                       double min_pivot, double* fuse_acc, int rows, const int32_t* slots,
                       const int32_t* slots_host, double inject_w, double fuse_fx, double fuse_fy, double fuse_cx,
                       double fuse_cy, double* q_out, float* R_out, double* t_out, int32_t* n_in, float* rms_px,
                       int32_t* state_out, void* stream);

/* comet_motion_fit (DESIGN.md "Motion estimate"): the frames at the positions [0, s) of a hop leave the
 *   window with a final fused pose and are committed exactly once (the rule of comet_landmark_update), so
 *   the committed poses of a stream are a time series in frames. This keeps a short history of them per
 *   stream and fits a constant angular velocity and a constant linear velocity to its newest frames, in one
 *   launch per push after that push's comet_pose_fuse: grid (n), one wave of 64 threads per hop, no LDS, no
 *   atomics, no communication between workgroups. Everything is IEEE double evaluated as written (no
 *   contraction); atan2, sin and cos are the device library's. It reports only: nothing is written but the
 *   state and the outputs.
 *   State: hist [S, cap, COMET_MOTION_ROW] f64, rows (q[4] w first, t[3], w), cap <= 64; hist_n [S] int32,
 *     the frames committed. Frame number f of a stream (from 0) lives in row f % cap. The row of the stream of
 *     hop h is stream_idx[h] (stream_idx_host: the same values on the host). hist_n saturates without losing
 *     the row: a count c >= COMET_MOTION_COUNT_FOLD is stored as cap + c % cap; a negative count reads as 0.
 *   Inputs per hop: R [n, T, 4] f32 quaternions (w first) and T [n, T, 3] f64, the fused_R / fused_T of that
 *     push; weights [n, T] f32 or NULL (= 1); first [n] int32.
 *   Per hop h, with c = first[h] ? 0 : hist_n:
 *   1. Append: position i = 0 .. s - 1 becomes frame number c + i: q = R[h, i] widened to double, conjugated
 *      when inverse_rotation = 1 (the convention of comet_landmark_update); t = T[h, i]; w = weights[h, i]. A
 *      frame is always stored, so a row's age is its time offset; if q, t or w is not finite or w <= 0 it is
 *      stored with w = 0 (q and t as they came). hist_n = c + s. Of more than cap frames the newest cap stay.
 *   2. Fit over the newest m = min(hist_n, fit_len) rows: lane k holds the row of age k (k = 0: the newest
 *      committed frame), tau_k = -k. A row is usable when k < m and w != 0 (this function stores w >= 0 only; a
 *      NaN or negative w can only come from the caller's hist and is summed as it is). n_used = usable rows.
 *   Sums: every lane contributes its term, or +0 when its row is not usable; the 64 values are combined by the
 *     fixed tree p[l] += p[l + d], d = 32, 16, .., 1 (__shfl_down), and lane 0's value is used. With wt = w tau:
 *     Sw = sum w, St = sum wt, Stt = sum wt tau, and for a component x: Sp = sum w x, Stp = sum wt x. Line:
 *     D = Sw Stt - St St, slope = (Sw Stp - St Sp) / D, offset = (Sp - slope St) / Sw.
 *   Rotation: q_ref = the newest usable row. `iters` passes: d_k = q_k (x) conj(q_ref) (Hamilton product),
 *     negated when its w < 0; with nv = |v| = sqrt(x^2 + y^2 + z^2): theta = 2 atan2(nv, w), phi_k =
 *     (theta / nv) v, and theta = 0, phi_k = 0 when nv == 0. A usable row with theta > max_angle: state 3. The
 *     line through each component of phi gives omega (slope) and a (offset); q_ref <- Exp(a) (x) q_ref,
 *     Exp(p) = (cos(|p| / 2), (sin(|p| / 2) / |p|) p), the identity when |p| == 0; then divided by its norm,
 *     negated when its w < 0 (the fuser's sign rule). q0 = q_ref after the last pass. One more pass takes
 *     phi_k against q0 (theta > max_angle: state 3 again) and the residual r_k = phi_k - omega tau_k (the offset
 *     is in q0): rot_rms = sqrt(sum w |r_k|^2 / Sw).
 *   Translation: the same line through each component of t gives vel (slope) and t0 (offset);
 *     trans_rms[j] = sqrt(sum w ((t_j - t0_j) - vel_j tau)^2 / Sw).
 *   Prediction at tau = 1 .. P, P = T - s + horizon, counted from the newest committed frame: pred_q =
 *     Exp(omega tau) (x) q0, conjugated back when inverse_rotation = 1; pred_t = t0 + vel tau. The first T - s
 *     of them are the window positions i = s .. T - 1 (tau = i - s + 1), for which the innovation against that
 *     push's fused pose is reported too: innov_rot = theta of R[h, i] (x) conj(pred_q) as above, innov_trans =
 *     |T[h, i] - pred_t|.
 *   State int32, in this order: 0 n_used < min_frames | -1 Sw, St, Stt or D not finite | 2 D <= 0 | 3 a relative
 *     rotation beyond max_angle | -1 an omega, a, q_ref, rms, vel or t0 that is not finite | 1 fitted. For every
 *     state other than 1: omega = vel = 0, q0 / t0 = the newest committed row bit for bit, rot_rms, trans_rms
 *     and the innovations are +inf, every prediction repeats the newest committed pose (R[h, s - 1] widened,
 *     T[h, s - 1]). The history is updated in every state.
 *   Outputs per hop: omega [3] f64 rad / frame with R(tau) = Exp(omega tau) R0 for the rotation as stored
 *     (after the conjugation on load); q0 [4] f64 in that same convention; vel [3], t0 [3] f64; rot_rms f32;
 *     trans_rms [3] f32; n_used, state int32; pred_q [P, 4], pred_t [P, 3] f64; innov_rot, innov_trans
 *     [T - s] f32.
 *   COMET_EINVAL before anything is launched, checked in this order: a null pointer (weights may be null),
 *   n < 1, T < 2, s outside [1, T - 1], cap outside [2, 64], fit_len outside [2, cap], min_frames outside
 *   [2, fit_len], iters outside [1, COMET_MOTION_MAX_ITERS], horizon outside [0, COMET_MOTION_MAX_HORIZON],
 *   max_angle not in (0, pi), inverse_rotation not 0 or 1, a host stream index outside [0, S) or two equal
 *   ones (two hops on one ring would race; a stream completes at most one hop per push), R / hist not 16-B
 *   aligned or T / omega / q0 / vel / t0 / pred_q / pred_t not 8-B aligned. The kernel range-checks every row
 *   index before it addresses memory. */
#define COMET_MOTION_ROW 8
#define COMET_MOTION_COUNT_FOLD (1 << 30)
#define COMET_MOTION_MAX_ITERS 8
#define COMET_MOTION_MAX_HORIZON 64
int comet_motion_fit(const float* R, const double* T, const float* weights, const int32_t* first,
                     const int32_t* stream_idx, const int32_t* stream_idx_host, double* hist, int32_t* hist_n,
                     int S, int cap, int n, int Tw, int s, int fit_len, int min_frames, int iters, int horizon,
                     double max_angle, int inverse_rotation, double* omega, double* q0, double* vel, double* t0,
                     float* rot_rms, float* trans_rms, int32_t* n_used, int32_t* state, double* pred_q,
                     double* pred_t, float* innov_rot, float* innov_trans, void* stream);

/* ---------------------------------------------------------------------------------------
 * Debug support (bounds asserts and a NaN / Inf check mode).
 * comet_count_nonfinite: adds the number of NaN / Inf elements of x (n elements, dtype) to
 *   *count (an int32 on the device; no host sync). Used by comet_amd.debug's finite-check hooks.
 * comet_debug_flags: the build's debug state. In a `make DEBUG=1` library (libcomet_hip_debug.so,
 *   compiled with COMET_DEBUG) every launch is followed by a device synchronise and a read of the
 *   device-side assertion word (index checks inside the kernels record a failed check there instead
 *   of trapping); the call returns that word and clears it (clear != 0). A release library returns
 *   -1. */
int comet_count_nonfinite(int dtype, const void* x, int64_t n, int32_t* count, void* stream);
int comet_debug_flags(int clear);
/* comet_lds_probe: LDS integrity probe for concurrency tests (tools/lds_race.py,
 *   tests/test_ops_gpu.py). `groups` workgroups each own the CU's whole LDS (160 KiB): per round
 *   they fill it with a pattern keyed by (workgroup, round), sleep about `spin` x 8k cycles and
 *   count the words that changed, adding the count to *bad (a uint32 on the device). A workgroup's
 *   LDS is its own, so any change is a write that landed after the CU handed the LDS over -- e.g.
 *   LDS-DMA of a kernel that ended with pieces in flight. */
int comet_lds_probe(int groups, int rounds, int spin, uint32_t* bad, void* stream);
/* comet_shfl_probe: cross-lane exchange probe for concurrency tests (tools/op_repeat.py). Each wave
 *   sums known integers over its 64 lanes `iters` times -- mode 0 by ds_bpermute (__shfl_xor), 1 by
 *   DPP + v_permlane swaps, 2 through its own LDS words -- and adds the number of wrong lane results
 *   to *bad (uint32 on the device). */
int comet_shfl_probe(int groups, int iters, int mode, uint32_t* bad, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COMET_HIP_H_ */
