// Elementwise, reduction and optimizer kernels: dtype cast, activation backward, axpby,
// column sums (bias grads), multi-tensor squared norm (clip_grad_norm_) and fused AdamW.
//
// Reference sites: train_eval_func_new_cp5.py:790-801 (backward, clip_grad_norm_(1.0),
// optimizer.step), train_util.py:311-332 (AdamW over camera_predictor.parameters()).
#include <cstdlib>

#include "common.hpp"

namespace comet {
namespace {

template <typename TI, typename TO>
__global__ void cast_kernel(const TI* __restrict__ x, TO* __restrict__ y, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    y[i] = from_f32<TO>(to_f32(x[i]));
}

template <typename TP, typename TD, typename TX>
__global__ void act_bwd_kernel(int act, const TP* __restrict__ pre, const TD* __restrict__ dy,
                               TX* __restrict__ dx, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float p = to_f32(pre[i]), d = to_f32(dy[i]);
    float g;
    switch (act) {
      case COMET_ACT_GELU: g = gelu_erf_grad(p); break;
      case COMET_ACT_RELU: g = p > 0.f ? 1.f : 0.f; break;
      case COMET_ACT_SIGMOID: { const float s = 1.f / (1.f + __expf(-p)); g = s * (1.f - s); break; }
      default: g = 1.f;
    }
    dx[i] = from_f32<TX>(d * g);
  }
}

__device__ __forceinline__ float act_grad(int act, float p) {
  switch (act) {
    case COMET_ACT_GELU: return gelu_erf_grad(p);
    case COMET_ACT_RELU: return p > 0.f ? 1.f : 0.f;
    case COMET_ACT_SIGMOID: { const float s = 1.f / (1.f + __expf(-p)); return s * (1.f - s); }
    default: return 1.f;
  }
}

template <int ACT>
__device__ __forceinline__ float act_grad_t(float p) {
  if constexpr (ACT == COMET_ACT_GELU) return gelu_grad_fast(p);
  else if constexpr (ACT == COMET_ACT_RELU) return p > 0.f ? 1.f : 0.f;
  else if constexpr (ACT == COMET_ACT_SIGMOID) { const float s = 1.f / (1.f + __expf(-p)); return s * (1.f - s); }
  else return 1.f;
}

// Linear-layer backward prologue in one pass over dY [rows, cols] (cols % 8 == 0):
// g = dY * act'(pre) (or dY), optionally stored (out, any dtype), and dbias[c] += sum_r g.
// Block = 32 column groups of 8 x 8 row lanes; partial column sums meet in LDS, one atomic per
// column per block. The activation and the presence of `out` are template parameters so the
// row loop is branch-free: four rows per trip with all their loads issued first.
template <typename TP, typename TD, typename TO, int ACT, bool HO>
__global__ void __launch_bounds__(256)
act_bwd_colsum_kernel(const TP* __restrict__ pre, const TD* __restrict__ dy, TO* __restrict__ out,
                      float* __restrict__ dbias, int64_t rows, int cols, int64_t chunk) {
  constexpr bool HP = ACT != COMET_ACT_NONE;
  __shared__ float red[8][256];
  const int t = threadIdx.x, cl = t & 31, rl = t >> 5;
  const int c0 = blockIdx.x * 256 + cl * 8;
  const int64_t r0 = (int64_t)blockIdx.y * chunk;
  const int64_t r1 = r0 + chunk < rows ? r0 + chunk : rows;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  auto row_step = [&](int64_t r, float (&g)[8], const float (&x)[8]) {
    if constexpr (HP) {
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] *= act_grad_t<ACT>(x[e]);
    }
    if constexpr (HO) {
      // round first so the bias gradient sums exactly the values the GEMMs consume
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = to_f32(from_f32<TO>(g[e]));
      store8(out + r * cols + c0, g);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += g[e];
  };
  if (c0 < cols) {
    int64_t r = r0 + rl;
    for (; r + 24 < r1; r += 32) {
      float g[4][8], x[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        load8(dy + (r + 8 * u) * cols + c0, g[u]);
        if constexpr (HP) load8(pre + (r + 8 * u) * cols + c0, x[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) row_step(r + 8 * u, g[u], x[u]);
    }
    for (; r < r1; r += 8) {
      float g[8], x[8];
      load8(dy + r * cols + c0, g);
      if constexpr (HP) load8(pre + r * cols + c0, x);
      row_step(r, g, x);
    }
  }
  if (!dbias) return;
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cl * 8 + e] = acc[e];
  __syncthreads();
  const int col = blockIdx.x * 256 + t;
  if (col < cols) {
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) sum += red[q][t];
    atomicAdd(dbias + col, sum);
  }
}

__global__ void axpby_kernel(const float* __restrict__ x, float* __restrict__ y, float a, float b,
                             int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    y[i] = a * x[i] + b * y[i];
}

// out[c] (+)= sum_r x[r*ld + c]; block = 256 columns x ROWCHUNK rows, atomics per block.
constexpr int COLSUM_ROWS = 1024;
template <typename T>
__global__ void colsum_kernel(const T* __restrict__ x, float* __restrict__ out, int64_t rows,
                              int64_t cols, int64_t ld) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const int64_t r0 = (int64_t)blockIdx.y * COLSUM_ROWS;
  const int64_t r1 = r0 + COLSUM_ROWS < rows ? r0 + COLSUM_ROWS : rows;
  float s = 0.f;
  for (int64_t r = r0; r < r1; ++r) s += to_f32(x[r * ld + c]);
  atomicAdd(out + c, s);
}

// Few rows (rows <= COLSUM_FEW: the f32 camera trunk's 128-token bias gradients): one workgroup per
// 64 columns, its 4 waves take every 4th row with 8 loads in flight per lane, the 4 partial sums meet
// in LDS and the workgroup writes (or adds to) out directly -- no memset launch, no atomics. The
// round-4 path (3 workgroups of serial 128-row sums behind a memset) took 34 us per 768 columns.
constexpr int COLSUM_FEW = 4096;
template <typename T>
__global__ void __launch_bounds__(256) colsum_few_kernel(const T* __restrict__ x, float* __restrict__ out,
                                                        int rows, int64_t cols, int64_t ld, int accumulate) {
  __shared__ float part[4][64];
  const int cl = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cl;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < cols) {
    int r = w;
    for (; r + 28 < rows; r += 32) {
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += to_f32(x[(int64_t)(r + 4 * u) * ld + c]);
    }
    for (; r < rows; r += 4) s[0] += to_f32(x[(int64_t)r * ld + c]);
  }
  part[w][cl] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (w == 0 && c < cols) {
    const float t = (part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl]);
    out[c] = accumulate ? out[c] + t : t;
  }
}

constexpr int MT_MAX = 24;
struct MultiPtr {
  float* p[MT_MAX];
  const float* g[MT_MAX];
  float* m[MT_MAX];
  float* v[MT_MAX];
  int64_t n[MT_MAX];
  int count;
};

// Squared L2 norm of many tensors in a fixed summation order (the clip coefficient every data-
// parallel replica derives from it must be bit-identical, or the replicas' weights drift apart):
// pass 1, at most SQ_NORM_BLOCKS workgroups with 16-B loads, writes one partial per workgroup (each
// thread's elements are fixed by its index and the grid, the grid by the sizes); pass 2, one
// workgroup, folds the partials in index order into out[0]. Round 5 ended pass 1 with one f32
// atomicAdd per workgroup on out[0]: an arrival-order sum that differed by ulps from launch to launch.
constexpr int SQ_NORM_BLOCKS = COMET_SQ_NORM_PARTIALS;
__global__ void __launch_bounds__(256) sq_norm_part_kernel(MultiPtr mp, float* __restrict__ part) {
  __shared__ float scratch[4];
  float s = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int t = 0; t < mp.count; ++t) {
    const float* x = mp.g[t];
    const int64_t n = mp.n[t];
    int64_t head = ((16 - ((uintptr_t)x & 15)) & 15) / 4;  // scalars before the first 16-B boundary
    if (head > n) head = n;
    const int64_t nv = (n - head) / 4;
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    for (int64_t i = tid; i < nv; i += stride) {
      const float4 v = xv[i];
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    for (int64_t i = tid; i < head; i += stride) s += x[i] * x[i];
    for (int64_t i = head + nv * 4 + tid; i < n; i += stride) s += x[i] * x[i];
  }
  s = block_sum<4>(s, scratch);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) sq_norm_fold_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
  __shared__ float scratch[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = block_sum<4>(s, scratch);
  if (threadIdx.x == 0) out[0] += s;
}

// torch.optim.AdamW (foreach=False semantics): p *= 1 - lr*wd; m.lerp_(g, 1-b1);
// v = b2*v + (1-b2)*g^2; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps).
__global__ void adamw_kernel(MultiPtr mp, float lr, float b1, float b2, float eps, float wd,
                             float bc1, float bc2_sqrt, const float* __restrict__ sqnorm,
                             float max_norm) {
  float clip = 1.f;
  if (sqnorm) {
    const float total = sqrtf(*sqnorm);
    const float coef = max_norm / (total + 1e-6f);
    clip = coef < 1.f ? coef : 1.f;
  }
  const float step_size = lr / bc1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int t = 0; t < mp.count; ++t) {
    float* p = mp.p[t]; const float* g = mp.g[t]; float* m = mp.m[t]; float* v = mp.v[t];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < mp.n[t]; i += stride) {
      const float gi = g[i] * clip;
      float pi = p[i] * (1.f - lr * wd);
      float mi = m[i];
      mi = mi + (1.f - b1) * (gi - mi);
      const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
      const float denom = sqrtf(vi) / bc2_sqrt + eps;
      pi = pi - step_size * (mi / denom);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
  }
}

// f32 -> bf16 for many tensors in one launch (the bf16 copies of the trainable weights, refreshed
// after every optimizer step instead of ~125 per-tensor casts at first use in the next forward)
constexpr int CAST_MAX = 48;
struct CastPtrs {
  const float* s[CAST_MAX];
  __bf16* d[CAST_MAX];
  int64_t n[CAST_MAX];
  int count;
};

__global__ void __launch_bounds__(256) cast_multi_kernel(CastPtrs cp) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int t = 0; t < cp.count; ++t) {
    const float* x = cp.s[t];
    __bf16* y = cp.d[t];
    const int64_t n = cp.n[t];
    if ((((uintptr_t)x & 15) | ((uintptr_t)y & 7)) == 0) {
      const int64_t nv = n / 4;
      for (int64_t i = tid; i < nv; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        reinterpret_cast<uint2*>(y)[i] = uint2{pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
      }
      for (int64_t i = nv * 4 + tid; i < n; i += stride) y[i] = static_cast<__bf16>(x[i]);
    } else {
      for (int64_t i = tid; i < n; i += stride) y[i] = static_cast<__bf16>(x[i]);
    }
  }
}

inline unsigned grid_for(int64_t n, int bs = 256) {
  int64_t g = cdiv(n, bs);
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (unsigned)g;
}

}  // namespace
}  // namespace comet

using namespace comet;

extern "C" int comet_cast(int dtype_in, int dtype_out, const void* x, void* y, int64_t n,
                          void* stream) {
  COMET_CHECK_ARG(x && y, "comet_cast: null pointer");
  if (n == 0) return COMET_OK;
  hipStream_t s = as_stream(stream);
  const unsigned g = grid_for(n);
  if (dtype_in == COMET_F32 && dtype_out == COMET_BF16)
    hipLaunchKernelGGL((cast_kernel<float, __bf16>), dim3(g), dim3(256), 0, s, (const float*)x, (__bf16*)y, n);
  else if (dtype_in == COMET_BF16 && dtype_out == COMET_F32)
    hipLaunchKernelGGL((cast_kernel<__bf16, float>), dim3(g), dim3(256), 0, s, (const __bf16*)x, (float*)y, n);
  else if (dtype_in == COMET_F32 && dtype_out == COMET_F32)
    hipLaunchKernelGGL((cast_kernel<float, float>), dim3(g), dim3(256), 0, s, (const float*)x, (float*)y, n);
  else
    hipLaunchKernelGGL((cast_kernel<__bf16, __bf16>), dim3(g), dim3(256), 0, s, (const __bf16*)x, (__bf16*)y, n);
  COMET_CHECK_LAUNCH("comet_cast");
  return COMET_OK;
}

extern "C" int comet_cast_multi_f32_bf16(const float* const* src, void* const* dst, const int64_t* sizes,
                                         int n_tensors, void* stream) {
  COMET_CHECK_ARG(n_tensors >= 0 && (n_tensors == 0 || (src && dst && sizes)), "comet_cast_multi_f32_bf16: bad args");
  hipStream_t s = as_stream(stream);
  for (int base = 0; base < n_tensors; base += CAST_MAX) {
    CastPtrs cp{};
    cp.count = n_tensors - base < CAST_MAX ? n_tensors - base : CAST_MAX;
    int64_t total = 0;
    for (int i = 0; i < cp.count; ++i) {
      COMET_CHECK_ARG(src[base + i] && dst[base + i] && sizes[base + i] >= 0, "comet_cast_multi_f32_bf16: null tensor");
      cp.s[i] = src[base + i];
      cp.d[i] = reinterpret_cast<__bf16*>(dst[base + i]);
      cp.n[i] = sizes[base + i];
      total += cp.n[i];
    }
    hipLaunchKernelGGL(cast_multi_kernel, dim3(grid_for(total / 4 + 1)), dim3(256), 0, s, cp);
    COMET_CHECK_LAUNCH("comet_cast_multi_f32_bf16");
  }
  return COMET_OK;
}

extern "C" int comet_act_bwd(int act, int dtype_pre, int dtype_dy, const void* pre, const void* dy,
                             void* dx, int dtype_dx, int64_t n, void* stream) {
  COMET_CHECK_ARG(pre && dy && dx, "comet_act_bwd: null pointer");
  if (n == 0) return COMET_OK;
  hipStream_t s = as_stream(stream);
  const unsigned g = grid_for(n);
#define AB(TP, TD, TX) \
  hipLaunchKernelGGL((act_bwd_kernel<TP, TD, TX>), dim3(g), dim3(256), 0, s, act, (const TP*)pre, (const TD*)dy, (TX*)dx, n)
#define AB_X(TP, TD) \
  do { if (dtype_dx == COMET_F32) AB(TP, TD, float); else AB(TP, TD, __bf16); } while (0)
#define AB_D(TP) \
  do { if (dtype_dy == COMET_F32) AB_X(TP, float); else AB_X(TP, __bf16); } while (0)
  if (dtype_pre == COMET_F32) AB_D(float); else AB_D(__bf16);
#undef AB_D
#undef AB_X
#undef AB
  COMET_CHECK_LAUNCH("comet_act_bwd");
  return COMET_OK;
}

extern "C" int comet_axpby(const float* x, float* y, float a, float b, int64_t n, void* stream) {
  COMET_CHECK_ARG(x && y, "comet_axpby: null pointer");
  if (n == 0) return COMET_OK;
  hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), x, y, a, b, n);
  COMET_CHECK_LAUNCH("comet_axpby");
  return COMET_OK;
}

extern "C" int comet_act_bwd_colsum(int act, int dtype_pre, const void* pre, int dtype_dy, const void* dy,
                                    int dtype_out, void* out, float* dbias, int64_t rows, int64_t cols,
                                    int accumulate, void* stream) {
  COMET_CHECK_ARG(dy && rows >= 0 && cols > 0 && cols % 8 == 0 && cols < (1ll << 31),
                  "comet_act_bwd_colsum: dy required, cols a positive multiple of 8");
  COMET_CHECK_ARG(act == COMET_ACT_NONE || pre != nullptr, "comet_act_bwd_colsum: activation needs pre");
  COMET_CHECK_ARG(((uintptr_t)pre | (uintptr_t)dy | (uintptr_t)out) % 32 == 0, "comet_act_bwd_colsum: 32-B alignment");
  hipStream_t s = as_stream(stream);
  if (dbias && !accumulate) {
    hipError_t e = hipMemsetAsync(dbias, 0, cols * sizeof(float), s);
    if (e != hipSuccess) { set_error("comet_act_bwd_colsum: memset failed"); return COMET_ELAUNCH; }
  }
  if (rows == 0) return COMET_OK;
  const int64_t cblocks = cdiv(cols, 256);
  // ~4096 workgroups (2-3 % faster than 2048 on the 73856-row f32 and bf16 shapes, tools/tail_ab.py,
  // profiles/r06_tail/tail_ab.txt; 1024: 2-7 % slower); COMET_COLSUM_WGS overrides (measurement)
  const char* cw = getenv("COMET_COLSUM_WGS");
  int64_t rblocks = cdiv(cw != nullptr && atoll(cw) > 0 ? atoll(cw) : 4096, cblocks);
  int64_t chunk = cdiv(rows, rblocks);
  if (chunk < 64) chunk = 64;
  rblocks = cdiv(rows, chunk);
  COMET_CHECK_ARG(rblocks <= 65535, "comet_act_bwd_colsum: too many rows");
  dim3 grid((unsigned)cblocks, (unsigned)rblocks);
  const void* P = act == COMET_ACT_NONE ? nullptr : pre;
  const bool ho = out != nullptr;
#define ABC(TP, TD, TO, A, H) \
  hipLaunchKernelGGL((act_bwd_colsum_kernel<TP, TD, TO, A, H>), grid, dim3(256), 0, s, (const TP*)P, (const TD*)dy, (TO*)out, dbias, rows, (int)cols, chunk)
#define ABC_H(TP, TD, TO, A) do { if (ho) ABC(TP, TD, TO, A, true); else ABC(TP, TD, TO, A, false); } while (0)
#define ABC_A(TP, TD, TO)                                                                   \
  do {                                                                                      \
    switch (act) {                                                                          \
      case COMET_ACT_GELU: ABC_H(TP, TD, TO, COMET_ACT_GELU); break;                        \
      case COMET_ACT_RELU: ABC_H(TP, TD, TO, COMET_ACT_RELU); break;                        \
      case COMET_ACT_SIGMOID: ABC_H(TP, TD, TO, COMET_ACT_SIGMOID); break;                  \
      default: ABC_H(TP, TD, TO, COMET_ACT_NONE); break;                                    \
    }                                                                                       \
  } while (0)
#define ABC_O(TP, TD) do { if (dtype_out == COMET_F32) ABC_A(TP, TD, float); else ABC_A(TP, TD, __bf16); } while (0)
#define ABC_D(TP) do { if (dtype_dy == COMET_F32) ABC_O(TP, float); else ABC_O(TP, __bf16); } while (0)
  if (dtype_pre == COMET_F32) ABC_D(float); else ABC_D(__bf16);
#undef ABC_D
#undef ABC_O
#undef ABC_A
#undef ABC_H
#undef ABC
  COMET_CHECK_LAUNCH("comet_act_bwd_colsum");
  return COMET_OK;
}

extern "C" int comet_colsum(int dtype, const void* x, float* out, int64_t rows, int64_t cols,
                            int64_t ld, int accumulate, void* stream) {
  COMET_CHECK_ARG(out && cols > 0 && rows >= 0 && (x || rows == 0), "comet_colsum: bad args");
  hipStream_t s = as_stream(stream);
  if (rows <= COLSUM_FEW) {
    const dim3 grid((unsigned)cdiv(cols, 64));
    if (dtype == COMET_F32)
      hipLaunchKernelGGL((colsum_few_kernel<float>), grid, dim3(256), 0, s, (const float*)x, out, (int)rows, cols, ld, accumulate);
    else
      hipLaunchKernelGGL((colsum_few_kernel<__bf16>), grid, dim3(256), 0, s, (const __bf16*)x, out, (int)rows, cols, ld, accumulate);
    COMET_CHECK_LAUNCH("comet_colsum (few rows)");
    return COMET_OK;
  }
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(out, 0, cols * sizeof(float), s);
    if (e != hipSuccess) { set_error("comet_colsum: memset failed"); return COMET_ELAUNCH; }
  }
  if (rows == 0) return COMET_OK;
  COMET_CHECK_ARG(cdiv(rows, COLSUM_ROWS) <= 65535, "comet_colsum: too many rows");
  dim3 grid((unsigned)cdiv(cols, 256), (unsigned)cdiv(rows, COLSUM_ROWS));
  if (dtype == COMET_F32)
    hipLaunchKernelGGL((colsum_kernel<float>), grid, dim3(256), 0, s, (const float*)x, out, rows, cols, ld);
  else
    hipLaunchKernelGGL((colsum_kernel<__bf16>), grid, dim3(256), 0, s, (const __bf16*)x, out, rows, cols, ld);
  COMET_CHECK_LAUNCH("comet_colsum");
  return COMET_OK;
}

extern "C" int comet_sq_norm_multi(const float* const* ptrs, const int64_t* sizes, int n_tensors,
                                   float* out, float* partials, void* stream) {
  COMET_CHECK_ARG(out && partials && n_tensors >= 0, "comet_sq_norm_multi: bad args");
  hipStream_t s = as_stream(stream);
  for (int base = 0; base < n_tensors; base += MT_MAX) {
    MultiPtr mp{};
    mp.count = n_tensors - base < MT_MAX ? n_tensors - base : MT_MAX;
    int64_t total = 0;
    for (int i = 0; i < mp.count; ++i) {
      mp.g[i] = ptrs[base + i];
      mp.n[i] = sizes[base + i];
      total += mp.n[i];
    }
    int64_t g = cdiv(total / 4 + 1, 256);
    if (g > SQ_NORM_BLOCKS) g = SQ_NORM_BLOCKS;
    hipLaunchKernelGGL(sq_norm_part_kernel, dim3((unsigned)g), dim3(256), 0, s, mp, partials);
    COMET_CHECK_LAUNCH("comet_sq_norm_multi (partials)");
    hipLaunchKernelGGL(sq_norm_fold_kernel, dim3(1), dim3(256), 0, s, (const float*)partials, (int)g, out);
    COMET_CHECK_LAUNCH("comet_sq_norm_multi (fold)");
  }
  return COMET_OK;
}

extern "C" int comet_adamw_multi(float* const* params, const float* const* grads,
                                 float* const* exp_avg, float* const* exp_avg_sq,
                                 const int64_t* sizes, int n_tensors, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int step,
                                 const float* sqnorm, float max_norm, void* stream) {
  COMET_CHECK_ARG(step >= 1, "comet_adamw_multi: step must be >= 1");
  hipStream_t s = as_stream(stream);
  // bias corrections in double, as torch computes them on the host: 1 - powf(beta2, step) in f32
  // cancels (beta2 = 0.999, step 2: half an ulp of 0.998 is 1.5e-5 of the 0.002 left), which moved
  // the step size of the early steps by up to 7e-6 relative
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  for (int base = 0; base < n_tensors; base += MT_MAX) {
    MultiPtr mp{};
    mp.count = n_tensors - base < MT_MAX ? n_tensors - base : MT_MAX;
    int64_t total = 0;
    for (int i = 0; i < mp.count; ++i) {
      mp.p[i] = params[base + i]; mp.g[i] = grads[base + i];
      mp.m[i] = exp_avg[base + i]; mp.v[i] = exp_avg_sq[base + i];
      mp.n[i] = sizes[base + i];
      total += mp.n[i];
    }
    hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(total / 4 + 1)), dim3(256), 0, s, mp, lr, beta1,
                       beta2, eps, weight_decay, bc1, bc2_sqrt, sqnorm, max_norm);
    COMET_CHECK_LAUNCH("comet_adamw_multi");
  }
  return COMET_OK;
}

// ---- NaN / Inf census (debug support, comet_amd.debug) --------------------------------------
namespace comet {
namespace {
template <typename T>
__global__ void __launch_bounds__(256) nonfinite_kernel(const T* __restrict__ x, int64_t n, int32_t* __restrict__ count) {
  int c = 0;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    c += !isfinite(to_f32(x[i]));
  c = (int)wave_sum((float)c);
  if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(count, c);
}

// LDS integrity probe (comet_lds_probe): the whole 160 KiB, one workgroup per CU. The pattern of
// word i in round r of workgroup b is a hash of (b, r, i), so a word written by anything else --
// or left over from another round -- is counted.
constexpr int PROBE_WORDS = 160 * 1024 / 4;
__device__ __forceinline__ unsigned probe_word(unsigned b, unsigned r, unsigned i) {
  unsigned h = (b * 0x9E3779B1u) ^ (r * 0x85EBCA77u) ^ (i * 0xC2B2AE3Du);
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  return h ^ (h >> 12);
}
__global__ void __launch_bounds__(256) lds_probe_kernel(int rounds, int spin, uint32_t* __restrict__ bad) {
  __shared__ unsigned lds[PROBE_WORDS];
  unsigned miss = 0;
  for (int r = 0; r < rounds; ++r) {
    for (int i = threadIdx.x; i < PROBE_WORDS; i += 256) lds[i] = probe_word(blockIdx.x, r, i);
    __syncthreads();
    for (int k = 0; k < spin; ++k) __builtin_amdgcn_s_sleep(127);
    for (int i = threadIdx.x; i < PROBE_WORDS; i += 256) miss += lds[i] != probe_word(blockIdx.x, r, i);
    __syncthreads();
  }
  miss = (unsigned)wave_sum((float)miss);
  if ((threadIdx.x & 63) == 0 && miss != 0) atomicAdd(bad, miss);
}

// Cross-lane exchange probe (comet_shfl_probe): every wave reduces known integers over its 64 lanes
// `iters` times and counts lanes whose result is wrong. mode 0: xor butterfly by __shfl_xor
// (ds_bpermute_b32, through the LDS crossbar); mode 1: the same sums by DPP row_mirror /
// row_half_mirror / quad_perm steps and v_permlane16_swap / v_permlane32_swap (VALU only);
// mode 2: through the wave's own LDS words (ds_write_b32, ds_read_b32 of the xor-16 partner).
__global__ void __launch_bounds__(256) shfl_probe_kernel(int iters, int mode, uint32_t* __restrict__ bad) {
  __shared__ int ex[256];
  const int lane = threadIdx.x & 63;
  unsigned miss = 0;
  for (int it = 0; it < iters; ++it) {
    const int v = lane * 7 + it + (int)blockIdx.x;
    const int want = 7 * 2016 + 64 * (it + (int)blockIdx.x);
    int x = v;
    if (mode == 0) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    } else if (mode == 1) {
      x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, false);  // row_mirror
      x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, false);  // row_half_mirror
      x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
      x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
      const auto w16 = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
      x = (int)(w16[0] + w16[1]);
      const auto w32 = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
      x = (int)(w32[0] + w32[1]);
    } else if (mode == 3 || mode == 4) {
      // two sums reduced together (the row-LN statistics' shape): small integers as f32, so every
      // order of the adds gives the same exact value; mode 3 lets hipcc pair the adds into
      // v_pk_add_f32, mode 4 keeps them scalar (an empty asm between the two)
      typedef float f2 __attribute__((ext_vector_type(2)));
      float a = (float)v, b = (float)(2 * v + 1);
      if (mode == 3) {
        f2 p = {a, b};
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          const f2 q = {__shfl_xor(p.x, m, 64), __shfl_xor(p.y, m, 64)};
          p += q;  // v_pk_add_f32
        }
        a = p.x;
        b = p.y;
      } else {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          const float pa = __shfl_xor(a, m, 64), pb = __shfl_xor(b, m, 64);
          a += pa;
          asm volatile("" : "+v"(a));
          b += pb;
        }
      }
      const bool ok = a == (float)want && b == (float)(2 * want + 64);
      x = ok ? want : want + 1;
    } else if (mode == 5 || mode == 6) {
      // one VOP3P instruction, 32 times: mode 5 the row-LN reduce's centring form (op_sel: the low
      // result reads the high half of the second pair; op_sel_hi: the high result its low half;
      // both negated), mode 6 the plain form; small integers, so the results are exact
      typedef float f2 __attribute__((ext_vector_type(2)));
      const f2 a = {(float)v, (float)(v + 3)};
      int okc = 0;
#pragma unroll 4
      for (int u = 0; u < 32; ++u) {
        const f2 b = {(float)(u + lane), (float)(2 * u - lane)};
        f2 r;
        if (mode == 5) {
          asm volatile("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]"
                       : "=v"(r) : "v"(a), "v"(b));
          okc += r.x == a.x - b.y && r.y == a.y - b.x;
        } else {
          asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
          okc += r.x == a.x - b.x && r.y == a.y - b.y;
        }
      }
      x = okc == 32 ? want : want + 1;
    } else if (mode >= 7 && mode <= 11) {
      // which VOP3P form: 7 op_sel:[0,1] alone, 8 op_sel_hi:[1,0] alone, 9 v_pk_mul_f32 op_sel:[0,1],
      // 10 v_pk_fma_f32 op_sel:[0,1,0], 11 v_pk_add_f32 op_sel:[1,0] (the first source's high half)
      typedef float f2 __attribute__((ext_vector_type(2)));
      const f2 a = {(float)v, (float)(v + 3)};
      int okc = 0;
#pragma unroll 4
      for (int u = 0; u < 32; ++u) {
        const f2 b = {(float)(u + lane), (float)(2 * u - lane)};
        f2 r;
        bool ok;
        if (mode == 7) {
          asm volatile("v_pk_add_f32 %0, %1, %2 op_sel:[0,1]" : "=v"(r) : "v"(a), "v"(b));
          ok = r.x == a.x + b.y && r.y == a.y + b.y;
        } else if (mode == 8) {
          asm volatile("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
          ok = r.x == a.x + b.x && r.y == a.y + b.x;
        } else if (mode == 9) {
          asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1]" : "=v"(r) : "v"(a), "v"(b));
          ok = r.x == a.x * b.y && r.y == a.y * b.y;
        } else if (mode == 10) {
          asm volatile("v_pk_fma_f32 %0, %1, %2, %1 op_sel:[0,1,0]" : "=v"(r) : "v"(a), "v"(b));
          ok = r.x == fmaf(a.x, b.y, a.x) && r.y == fmaf(a.y, b.y, a.y);
        } else {
          asm volatile("v_pk_add_f32 %0, %1, %2 op_sel:[1,0]" : "=v"(r) : "v"(a), "v"(b));
          ok = r.x == a.y + b.x && r.y == a.y + b.y;
        }
        okc += ok;
      }
      x = okc == 32 ? want : want + 1;
    } else if (mode >= 13 && mode <= 16) {
      // 13-15: v_pk_mov_b32 op_sel:[1,0] / [0,1] / [1,1] (dst.lo = src0[op_sel0], dst.hi =
      // src1[op_sel1]); 16: v_pk_fma_f32 op_sel:[0,0,1] (the addend's high half into the low result)
      typedef float f2 __attribute__((ext_vector_type(2)));
      const f2 a = {(float)v, (float)(v + 3)};
      int okc = 0;
#pragma unroll 4
      for (int u = 0; u < 32; ++u) {
        const f2 b = {(float)(u + lane), (float)(2 * u - lane)};
        f2 r;
        bool ok;
        if (mode == 13) {
          asm volatile("v_pk_mov_b32 %0, %1, %2 op_sel:[1,0]" : "=v"(r) : "v"(a), "v"(b));
          ok = r.x == a.y && r.y == b.x;
        } else if (mode == 14) {
          asm volatile("v_pk_mov_b32 %0, %1, %2 op_sel:[0,1]" : "=v"(r) : "v"(a), "v"(b));
          ok = r.x == a.x && r.y == b.y;
        } else if (mode == 15) {
          asm volatile("v_pk_mov_b32 %0, %1, %2 op_sel:[1,1]" : "=v"(r) : "v"(a), "v"(b));
          ok = r.x == a.y && r.y == b.y;
        } else {
          asm volatile("v_pk_fma_f32 %0, %1, %1, %2 op_sel:[0,0,1]" : "=v"(r) : "v"(a), "v"(b));
          ok = r.x == fmaf(a.x, a.x, b.y) && r.y == fmaf(a.y, a.y, b.y);
        }
        okc += ok;
      }
      x = okc == 32 ? want : want + 1;
    } else if (mode == 12) {
      // aggressor: a back-to-back MFMA stream (16x16x32 bf16), nothing checked
      typedef __bf16 b8 __attribute__((ext_vector_type(8)));
      typedef float f4 __attribute__((ext_vector_type(4)));
      const b8 fa = __builtin_bit_cast(b8, uint4{(unsigned)v, 2u, 3u, 4u});
      f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
#pragma unroll 4
      for (int u = 0; u < 64; ++u) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fa, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fa, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fa, acc2, 0, 0, 0);
        acc3 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fa, acc3, 0, 0, 0);
      }
      x = (acc0[0] + acc1[1] + acc2[2] + acc3[3]) == 12345.f ? want + 1 : want;
    } else {
      ex[threadIdx.x] = v;
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's write is in LDS
      const int p = ex[threadIdx.x ^ 16];
      x = (v + p == 2 * v + ((lane ^ 16) - lane) * 7) ? want : want + 1;
      __builtin_amdgcn_s_waitcnt(0xC07F);
    }
    miss += x != want;
  }
  miss = (unsigned)wave_sum((float)miss);
  if (lane == 0 && miss != 0) atomicAdd(bad, miss);
}
}  // namespace
}  // namespace comet

extern "C" int comet_shfl_probe(int groups, int iters, int mode, uint32_t* bad, void* stream) {
  using namespace comet;
  COMET_CHECK_ARG(bad != nullptr && groups > 0 && iters > 0 && mode >= 0 && mode <= 16, "comet_shfl_probe: bad args");
  hipLaunchKernelGGL(shfl_probe_kernel, dim3((unsigned)groups), dim3(256), 0, as_stream(stream), iters, mode, bad);
  COMET_CHECK_LAUNCH("comet_shfl_probe");
  return COMET_OK;
}

extern "C" int comet_lds_probe(int groups, int rounds, int spin, uint32_t* bad, void* stream) {
  using namespace comet;
  COMET_CHECK_ARG(bad != nullptr && groups > 0 && rounds > 0 && spin >= 0 && spin <= 1024, "comet_lds_probe: bad args");
  hipLaunchKernelGGL(lds_probe_kernel, dim3((unsigned)groups), dim3(256), 0, as_stream(stream), rounds, spin, bad);
  COMET_CHECK_LAUNCH("comet_lds_probe");
  return COMET_OK;
}

extern "C" int comet_count_nonfinite(int dtype, const void* x, int64_t n, int32_t* count, void* stream) {
  using namespace comet;
  COMET_CHECK_ARG(x != nullptr && count != nullptr && n >= 0, "comet_count_nonfinite: bad args");
  if (n == 0) return COMET_OK;
  const unsigned g = (unsigned)(cdiv(n, 256) < 4096 ? cdiv(n, 256) : 4096);
  if (dtype == COMET_BF16)
    hipLaunchKernelGGL(nonfinite_kernel<__bf16>, dim3(g), dim3(256), 0, as_stream(stream), (const __bf16*)x, n, count);
  else if (dtype == COMET_F32)
    hipLaunchKernelGGL(nonfinite_kernel<float>, dim3(g), dim3(256), 0, as_stream(stream), (const float*)x, n, count);
  else {
    set_error("comet_count_nonfinite: bad dtype");
    return COMET_EINVAL;
  }
  COMET_CHECK_LAUNCH("comet_count_nonfinite");
  return COMET_OK;
}
