// Landmark map of the online path (comet_amd/stream.py LandmarkMap, DESIGN.md "Landmarks"): a carried
// track (comet_track_carry) observed over the frames whose fused pose is final (comet_pose_fuse) is a
// multi-view triangulation problem. comet_landmark_update keeps one row of normal equations per
// query slot and returns, for every slot of the n hops of a push, the 3-D point in the body frame,
// its observation count, its reprojection error on the frame that becomes the next window's first,
// and a state, all in one launch. One thread per (hop, slot); no LDS, no atomics, no communication
// between threads. The contract is in include/comet_hip.h; tests/landmark_numpy.py restates it.
#include <cmath>

#include "common.hpp"
#include "lm_solve.hpp"

namespace comet {
namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_MAX_N = COMET_CARRY_MAX_TRACKS;

// Everything below is plain IEEE double evaluated as written (no contraction into fma):
// tests/landmark_numpy.py restates it operation by operation.
#pragma clang fp contract(off)

struct LandmarkArgs {  // by value in the kernel arguments
  const float* tracks;    // [n, T, N, 2]
  const float* weights;   // [n, T, N] or NULL
  const float* R;         // [n, T, 4]
  const double* Tx;       // [n, T, 3]
  const int* ids;         // [n, N]
  const int* src;         // [n, N]
  const int* stream_idx;  // [n]
  const double* intr;     // [n, 4]
  double* acc;            // [rows, LM_ROW]
  int* acc_id;            // [rows]
  double* X;              // [n, N, 3]
  int* n_obs;             // [n, N]
  float* err_px;          // [n, N]
  int* state;             // [n, N]
  int T, N, s, rows, inverse, min_obs;
  double min_pivot;
};

// row += w (a a^T, a c, c^2) of one equation a . X = c
__device__ __forceinline__ void lm_add_equation(double (&r)[LM_ROW], double w, const double (&a)[3], double c) {
  r[0] += w * (a[0] * a[0]);
  r[1] += w * (a[0] * a[1]);
  r[2] += w * (a[0] * a[2]);
  r[3] += w * (a[1] * a[1]);
  r[4] += w * (a[1] * a[2]);
  r[5] += w * (a[2] * a[2]);
  r[6] += w * (a[0] * c);
  r[7] += w * (a[1] * c);
  r[8] += w * (a[2] * c);
  r[9] += w * (c * c);
}

__global__ __launch_bounds__(LM_THREADS) void landmark_update_kernel(LandmarkArgs a) {
  const int j = blockIdx.x * LM_THREADS + threadIdx.x, h = blockIdx.y;
  const int N = a.N, T = a.T, s = a.s;
  if (j >= N) return;
  const int sidx = a.stream_idx[h];
  const long long row = (long long)sidx * N + j;
  COMET_DASSERT(sidx >= 0 && row < a.rows);
  // (the stream indices are checked on the host too: never touch memory outside the state)
  if (sidx < 0 || row >= a.rows) return;
  const size_t o = (size_t)h * N + j;
  double* accp = a.acc + (size_t)row * LM_ROW;
  const int id = a.ids[o];
  double r[LM_ROW];
  int st = 0, nobs = 0;
  double X[3] = {0.0, 0.0, 0.0};
  float err = INFINITY;

  if (id < 0) {  // a pad: no landmark lives here
#pragma unroll
    for (int k = 0; k < LM_ROW; ++k) r[k] = 0.0;
#pragma unroll
    for (int k = 0; k < LM_ROW; k += 2) *reinterpret_cast<double2*>(accp + k) = double2{0.0, 0.0};
    a.acc_id[row] = -1;
  } else {
    const bool fresh = a.src[o] != j || a.acc_id[row] != id;
    if (fresh) {
#pragma unroll
      for (int k = 0; k < LM_ROW; ++k) r[k] = 0.0;
    } else {
#pragma unroll
      for (int k = 0; k < LM_ROW; k += 2) {
        const double2 d = *reinterpret_cast<const double2*>(accp + k);
        r[k] = d.x;
        r[k + 1] = d.y;
      }
    }
    const double* in = a.intr + (size_t)h * 4;
    const double fx = in[0], fy = in[1], cx = in[2], cy = in[3];
    // the committed frames: positions [0, s) leave the window after this hop, their pose is final
    for (int i = 0; i < s; ++i) {
      const size_t f = (size_t)h * T + i;
      const float2 p = *reinterpret_cast<const float2*>(a.tracks + (f * N + j) * 2);
      const double w = a.weights ? (double)a.weights[f * N + j] : 1.0;
      if (!(isfinite(p.x) && isfinite(p.y) && isfinite(w) && w > 0.0)) continue;
      double m[3][3];
      lm_rotation(a.R + f * 4, a.inverse != 0, m);
      const double* t = a.Tx + f * 3;
      const double tx = t[0], ty = t[1], tz = t[2];
      const double xn = ((double)p.x - cx) / fx, yn = ((double)p.y - cy) / fy;
      const double a1[3] = {m[0][0] - xn * m[2][0], m[0][1] - xn * m[2][1], m[0][2] - xn * m[2][2]};
      const double a2[3] = {m[1][0] - yn * m[2][0], m[1][1] - yn * m[2][1], m[1][2] - yn * m[2][2]};
      lm_add_equation(r, w, a1, xn * tz - tx);
      lm_add_equation(r, w, a2, yn * tz - ty);
      r[10] += 1.0;
    }
    r[11] = 0.0;
#pragma unroll
    for (int k = 0; k < LM_ROW; k += 2) *reinterpret_cast<double2*>(accp + k) = double2{r[k], r[k + 1]};
    a.acc_id[row] = id;
    nobs = (int)r[10];

    if (nobs >= a.min_obs) {
      // M X = g by the shared solve (lm_solve.hpp); a pivot at or below min_pivot * max(diag M) is ill-conditioned
      double sol[3];
      if (!lm_solve(r, a.min_pivot, sol)) {
        st = 2;
      } else {
        const double x0 = sol[0], x1 = sol[1], x2 = sol[2];
        // the reprojection on position s, the frame that becomes the next window's first
        const size_t f = (size_t)h * T + s;
        double m[3][3];
        lm_rotation(a.R + f * 4, a.inverse != 0, m);
        const double* t = a.Tx + f * 3;
        const double xc = m[0][0] * x0 + m[0][1] * x1 + m[0][2] * x2 + t[0];
        const double yc = m[1][0] * x0 + m[1][1] * x1 + m[1][2] * x2 + t[1];
        const double zc = m[2][0] * x0 + m[2][1] * x1 + m[2][2] * x2 + t[2];
        const float2 p = *reinterpret_cast<const float2*>(a.tracks + (f * N + j) * 2);
        const double du = fx * (xc / zc) + cx - (double)p.x, dv = fy * (yc / zc) + cy - (double)p.y;
        const double e = sqrt(du * du + dv * dv);
        if (!(isfinite(x0) && isfinite(x1) && isfinite(x2))) {
          st = -1;
        } else if (zc <= 0.0) {
          st = 3;
        } else if (!isfinite(e)) {
          st = -1;
        } else {
          st = 1;
          X[0] = x0; X[1] = x1; X[2] = x2;
          err = (float)e;
        }
      }
    }
  }
  a.X[o * 3 + 0] = X[0];
  a.X[o * 3 + 1] = X[1];
  a.X[o * 3 + 2] = X[2];
  a.n_obs[o] = nobs;
  a.err_px[o] = err;
  a.state[o] = st;
}

}  // namespace
}  // namespace comet

using namespace comet;

extern "C" int comet_landmark_update(const float* tracks, const float* weights, const float* R, const double* T,
                                     const int32_t* ids, const int32_t* src, const int32_t* stream_idx,
                                     const int32_t* stream_idx_host, const double* intr, const double* intr_host,
                                     double* acc, int32_t* acc_id, int rows, int n, int Tw, int N, int s,
                                     int inverse_rotation, int min_obs, double min_pivot, double* X, int32_t* n_obs,
                                     float* err_px, int32_t* state, void* stream) {
  COMET_CHECK_ARG(tracks && R && T && ids && src && stream_idx && stream_idx_host && intr && intr_host && acc &&
                      acc_id && X && n_obs && err_px && state,
                  "comet_landmark_update: null pointer");
  COMET_CHECK_ARG(n >= 1, "comet_landmark_update: n must be positive");
  COMET_CHECK_ARG(N >= 1 && N <= LM_MAX_N, "comet_landmark_update: N outside [1, 4096]");
  COMET_CHECK_ARG(Tw >= 2, "comet_landmark_update: T must be at least 2");
  COMET_CHECK_ARG(s >= 1 && s <= Tw - 1, "comet_landmark_update: s outside [1, T - 1]");
  COMET_CHECK_ARG((int64_t)rows >= (int64_t)n * N, "comet_landmark_update: rows below n * N");
  for (int h = 0; h < n; ++h) {  // two hops on one stream's rows would race (n is a handful: compared pairwise)
    COMET_CHECK_ARG(stream_idx_host[h] >= 0 && stream_idx_host[h] < rows / N,
                    "comet_landmark_update: stream index outside the state");
    for (int g = 0; g < h; ++g)
      COMET_CHECK_ARG(stream_idx_host[g] != stream_idx_host[h], "comet_landmark_update: duplicate stream index");
  }
  for (int h = 0; h < n; ++h)
    COMET_CHECK_ARG(std::isfinite(intr_host[4 * h]) && intr_host[4 * h] > 0.0 && std::isfinite(intr_host[4 * h + 1]) &&
                        intr_host[4 * h + 1] > 0.0,
                    "comet_landmark_update: fx and fy must be finite and positive");
  COMET_CHECK_ARG(inverse_rotation == 0 || inverse_rotation == 1, "comet_landmark_update: inverse_rotation must be 0 or 1");
  COMET_CHECK_ARG(min_obs >= 2, "comet_landmark_update: min_obs must be at least 2");
  COMET_CHECK_ARG(min_pivot >= 0.0 && min_pivot < 1.0, "comet_landmark_update: min_pivot outside [0, 1)");
  COMET_CHECK_ARG((((uintptr_t)tracks) & 7) == 0 && (((uintptr_t)R | (uintptr_t)acc) & 15) == 0 &&
                      (((uintptr_t)T | (uintptr_t)intr | (uintptr_t)X) & 7) == 0,
                  "comet_landmark_update: tracks, T, intr and X must be 8-B aligned, R and acc 16-B aligned");
  LandmarkArgs a{};
  a.tracks = tracks; a.weights = weights; a.R = R; a.Tx = T; a.ids = ids; a.src = src; a.stream_idx = stream_idx;
  a.intr = intr; a.acc = acc; a.acc_id = acc_id; a.X = X; a.n_obs = n_obs; a.err_px = err_px; a.state = state;
  a.T = Tw; a.N = N; a.s = s; a.rows = rows; a.inverse = inverse_rotation; a.min_obs = min_obs;
  a.min_pivot = min_pivot;
  hipLaunchKernelGGL(landmark_update_kernel, dim3((unsigned)cdiv(N, LM_THREADS), (unsigned)n), dim3(LM_THREADS), 0,
                     as_stream(stream), a);
  COMET_CHECK_LAUNCH("comet_landmark_update");
  return COMET_OK;
}
