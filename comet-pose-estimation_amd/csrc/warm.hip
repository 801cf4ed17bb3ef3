// Warm start of the coarse tracker in carried streams (comet_amd/stream.py TrackCarry, DESIGN.md
// "Warm start"): a slot that comet_track_carry carried over starts the new window's iterations where
// its track already was one hop ago, shifted by the stride, not on its query point in every frame.
// comet_track_warm builds the predictor's starting coordinates [n, N, T, 2] for all n hops of a push
// in one launch, one thread per slot. The contract is in include/comet_hip.h; tests/warm_numpy.py
// restates it with sequential loops.
#include <climits>
#include <cmath>

#include "common.hpp"

namespace comet {
namespace {

constexpr int WARM_THREADS = 256;
constexpr int WARM_MAX_BLOCKS = 2048;
constexpr int WARM_MAX_N = COMET_CARRY_MAX_TRACKS;

// the extrapolation is plain f32 evaluated as written (tests/warm_numpy.py uses the same expression)
#pragma clang fp contract(off)

struct WarmArgs {  // by value in the kernel arguments
  const float2* prev;     // [n, T, N]
  const int* src;         // [n, N]
  const float2* query;    // [n, N]
  const int* prev_valid;  // [n]
  float2* coords;         // [n, N, T]
  int* warm;              // [n, N]
  int64_t total;          // n * N
  int T, N, s, mode;
  float xmax, ymax, div0, div1;
};

__device__ __forceinline__ float warm_clamp(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

// Frame i >= 1 of the warm row of donor k, in pixels, before the clamp. pv: the hop's prev [T, N].
__device__ __forceinline__ float2 warm_frame(const WarmArgs& a, const float2* pv, int k, int i, float2 last,
                                             float2 before) {
  const int overlap = a.T - 1 - a.s;
  if (i <= overlap) return pv[(size_t)(i + a.s) * a.N + k];
  if (a.mode == 0) return last;
  const float e = (float)(i - overlap);
  return float2{last.x + e * (last.x - before.x), last.y + e * (last.y - before.y)};
}

__global__ __launch_bounds__(WARM_THREADS) void track_warm_kernel(WarmArgs a) {
  const int T = a.T, N = a.N;
  for (int64_t t = (int64_t)blockIdx.x * WARM_THREADS + threadIdx.x; t < a.total;
       t += (int64_t)gridDim.x * WARM_THREADS) {
    const int64_t b = t / N;
    const int j = (int)(t - b * N);
    const int* src = a.src + b * N;
    const float2* pv = a.prev + b * T * N;
    const float2 q = a.query[t];
    // the donor: a carried slot, or for a pad copy the slot it copies when that one is carried
    int k = -1, code = 0;
    if (a.prev_valid[b] != 0) {
      const int v = src[j];
      if (v >= 0 && v < N) {
        k = v;
        code = 1;
      } else if (v < 0) {
        const int64_t l = (int64_t)v - (int64_t)INT_MIN;
        if (l < N && src[l] == (int)l) {
          k = (int)l;
          code = 2;
        }
      }
    }
    float2 last = q, before = q;
    if (k >= 0) {  // (0 <= k < N was checked above; T >= 2 on the host)
      last = pv[(size_t)(T - 1) * N + k];
      before = pv[(size_t)(T - 2) * N + k];
      bool ok = isfinite(q.x) && isfinite(q.y);
      for (int i = 1; i < T; ++i) {
        const float2 p = warm_frame(a, pv, k, i, last, before);
        ok = ok && isfinite(p.x) && isfinite(p.y);
      }
      if (!ok) {
        k = -1;
        code = -1;
      }
    }
    float2* out = a.coords + t * T;
    const float2 q0{q.x / a.div0 / a.div1, q.y / a.div0 / a.div1};
    out[0] = q0;
    const int overlap = T - 1 - a.s;
    for (int i = 1; i < T; ++i) {
      float2 p = q0;
      if (k >= 0) {
        p = warm_frame(a, pv, k, i, last, before);
        if (i > overlap && a.mode == 1) {
          p.x = warm_clamp(p.x, a.xmax);
          p.y = warm_clamp(p.y, a.ymax);
        }
        p.x = p.x / a.div0 / a.div1;
        p.y = p.y / a.div0 / a.div1;
      }
      out[i] = p;
    }
    a.warm[t] = code;
  }
}

}  // namespace
}  // namespace comet

using namespace comet;

extern "C" int comet_track_warm(const float* prev, const int32_t* src, const float* query, const int32_t* prev_valid,
                                int n, int T, int N, int s, int H, int W, int mode, float div0, float div1,
                                float* coords, int32_t* warm, void* stream) {
  COMET_CHECK_ARG(prev && src && query && prev_valid && coords && warm, "comet_track_warm: null pointer");
  COMET_CHECK_ARG(n >= 1, "comet_track_warm: n must be positive");
  COMET_CHECK_ARG(N >= 1 && N <= WARM_MAX_N, "comet_track_warm: N outside [1, 4096]");
  COMET_CHECK_ARG(T >= 2, "comet_track_warm: T must be at least 2");
  COMET_CHECK_ARG(s >= 1 && s <= T - 1, "comet_track_warm: s outside [1, T - 1]");
  COMET_CHECK_ARG(H >= 1 && W >= 1, "comet_track_warm: H and W must be positive");
  COMET_CHECK_ARG(mode == 0 || mode == 1, "comet_track_warm: mode must be 0 (hold) or 1 (constant velocity)");
  COMET_CHECK_ARG(std::isfinite(div0) && std::isfinite(div1) && div0 > 0.f && div1 > 0.f,
                  "comet_track_warm: div0 and div1 must be finite and positive");
  COMET_CHECK_ARG((((uintptr_t)prev | (uintptr_t)query | (uintptr_t)coords) & 7) == 0,
                  "comet_track_warm: prev, query and coords must be 8-B aligned");
  WarmArgs a{};
  a.prev = reinterpret_cast<const float2*>(prev);
  a.src = src;
  a.query = reinterpret_cast<const float2*>(query);
  a.prev_valid = prev_valid;
  a.coords = reinterpret_cast<float2*>(coords);
  a.warm = warm;
  a.total = (int64_t)n * N;
  a.T = T; a.N = N; a.s = s; a.mode = mode;
  a.xmax = (float)(W - 1); a.ymax = (float)(H - 1);
  a.div0 = div0; a.div1 = div1;
  const int64_t blocks = cdiv(a.total, WARM_THREADS);
  const unsigned grid = (unsigned)(blocks < WARM_MAX_BLOCKS ? blocks : WARM_MAX_BLOCKS);
  hipLaunchKernelGGL(track_warm_kernel, dim3(grid), dim3(WARM_THREADS), 0, as_stream(stream), a);
  COMET_CHECK_LAUNCH("comet_track_warm");
  return COMET_OK;
}
