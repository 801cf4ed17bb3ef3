// Map-based pose refinement of the online path (comet_amd/stream.py LandmarkMap.pnp, DESIGN.md "PnP
// refinement"): the landmarks of comet_landmark_update are 3-D points in the body frame and the window's
// tracks are their 2-D observations, so every frame of a window has a perspective-n-point problem of its
// own. comet_landmark_pnp solves it by K Gauss-Newton steps with a Huber weight, starting from the fused
// pose, and can add the result to the fusion accumulator as one more hypothesis. One workgroup of 256
// threads per (hop, window position); the normal equations are summed by a fixed tree (strided sums per
// thread, then p[t] += p[t + d] for d = 128 .. 1), so the result does not depend on the launch. No
// atomics, no communication between workgroups. The contract is in include/comet_hip.h;
// tests/pnp_numpy.py restates it.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "fuse_row.hpp"

namespace comet {
namespace {

constexpr int PNP_THREADS = 256;
constexpr int PNP_WAVES = PNP_THREADS / 64;
constexpr int PNP_MAX_N = COMET_CARRY_MAX_TRACKS;
constexpr int PNP_MAX_ITERS = COMET_PNP_MAX_ITERS;
constexpr int PNP_NV = 28;  // 21 values of the upper triangle of H, 6 of b, the usable count
constexpr int PNP_NF = 4;   // the final pass: usable count, inliers, sum w |r|^2, sum w

// Everything below is plain IEEE double evaluated as written (no contraction into fma), and only
// + - * / and sqrt: tests/pnp_numpy.py restates it operation by operation.
#pragma clang fp contract(off)

struct PnpArgs {  // by value in the kernel arguments
  const float* tracks;   // [n, T, N, 2]
  const float* weights;  // [n, T, N] or NULL
  const double* X;       // [n, N, 3]
  const int* state;      // [n, N]
  const float* R0;       // [n, T, 4]
  const double* T0;      // [n, T, 3]
  const double* intr;    // [n, 4]
  double* fuse_acc;      // [rows, FUSE_ROW] or NULL
  const int* slots;      // [n * T] or NULL
  double* q_out;         // [n, T, 4]
  float* R_out;          // [n, T, 4]
  double* t_out;         // [n, T, 3]
  int* n_in;             // [n, T]
  float* rms_px;         // [n, T]
  int* state_out;        // [n, T]
  double huber, min_pivot, inject_w, ffx, ffy, fcx, fcy;
  int n, T, N, s, inverse, iters, min_pts, rows;
};

// rows of the matrix of the quaternion (r, i, j, k) (minipytorch3d.quaternion_to_matrix, the formula of
// landmark.hip lm_rotation), or of its transpose
__device__ __forceinline__ void pnp_rotation(double r, double i, double j, double k, bool inverse, double (&m)[3][3]) {
  const double two_s = 2.0 / (r * r + i * i + j * j + k * k);
  const double m00 = 1.0 - two_s * (j * j + k * k), m01 = two_s * (i * j - k * r), m02 = two_s * (i * k + j * r);
  const double m10 = two_s * (i * j + k * r), m11 = 1.0 - two_s * (i * i + k * k), m12 = two_s * (j * k - i * r);
  const double m20 = two_s * (i * k - j * r), m21 = two_s * (j * k + i * r), m22 = 1.0 - two_s * (i * i + j * j);
  m[0][0] = m00; m[1][1] = m11; m[2][2] = m22;
  m[0][1] = inverse ? m10 : m01; m[1][0] = inverse ? m01 : m10;
  m[0][2] = inverse ? m20 : m02; m[2][0] = inverse ? m02 : m20;
  m[1][2] = inverse ? m21 : m12; m[2][1] = inverse ? m12 : m21;
}

struct PnpPoint {
  double w, xc[3], r0, r1, rn;
};

// The observation of slot j on the frame f = h * T + i at the pose (m, t); false: not usable.
__device__ __forceinline__ bool pnp_point(const PnpArgs& a, int h, size_t f, int j, const double (&m)[3][3],
                                          const double (&t)[3], const double (&in)[4], PnpPoint& p) {
  const size_t o = (size_t)h * a.N + j;
  if (a.state[o] != 1) return false;
  const float2 px = *reinterpret_cast<const float2*>(a.tracks + (f * a.N + j) * 2);
  p.w = a.weights ? (double)a.weights[f * a.N + j] : 1.0;
  if (!(isfinite(px.x) && isfinite(px.y) && isfinite(p.w) && p.w > 0.0)) return false;
  const double* X = a.X + o * 3;
  const double x0 = X[0], x1 = X[1], x2 = X[2];
  p.xc[0] = m[0][0] * x0 + m[0][1] * x1 + m[0][2] * x2 + t[0];
  p.xc[1] = m[1][0] * x0 + m[1][1] * x1 + m[1][2] * x2 + t[1];
  p.xc[2] = m[2][0] * x0 + m[2][1] * x1 + m[2][2] * x2 + t[2];
  if (!(p.xc[2] > 0.0)) return false;
  p.r0 = in[0] * (p.xc[0] / p.xc[2]) + in[2] - (double)px.x;
  p.r1 = in[1] * (p.xc[1] / p.xc[2]) + in[3] - (double)px.y;
  p.rn = sqrt(p.r0 * p.r0 + p.r1 * p.r1);
  return true;
}

// The workgroup's sum of v, valid in thread 0: p[t] += p[t + d] for d = 128, 64 through LDS (waves 1..3
// hand their values to wave 0), then d = 32 .. 1 by wave shuffles. At step d only the threads t < d
// matter, and those read lane t + d < 64, so the additions are exactly the tree's. The caller
// synchronises the workgroup before the next call (it does, to broadcast the new pose).
template <int NV>
__device__ __forceinline__ void pnp_reduce(double (&v)[NV], double* lds) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[((wave - 1) * NV + k) * 64 + lane] = v[k];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const double p0 = v[k] + lds[(1 * NV + k) * 64 + lane];                               // p[t] += p[t + 128]
      const double p1 = lds[(0 * NV + k) * 64 + lane] + lds[(2 * NV + k) * 64 + lane];      // p[t + 64] += p[t + 192]
      double s = p0 + p1;                                                                   // p[t] += p[t + 64]
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
      v[k] = s;
    }
  }
}

// One Gauss-Newton step from the reduced sums v (thread 0 only): H delta = -b by an unpivoted LDL^T, then
// the retraction on (m, t, q). -> 1 solved, 2 a pivot at or below min_pivot * max(diag H), -1 not finite.
__device__ __forceinline__ int pnp_step(const double (&v)[PNP_NV], double min_pivot, bool inverse, double (&m)[3][3],
                                        double (&t)[3], double (&q)[4]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < PNP_NV - 1; ++k) ok = ok && isfinite(v[k]);
  if (!ok) return -1;
  double A[6][6];  // the lower triangle of H; v holds the upper one row by row
  {
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) A[c][r] = v[k++];
  }
  double thr = A[0][0];
#pragma unroll
  for (int r = 1; r < 6; ++r) thr = fmax(thr, A[r][r]);
  thr = min_pivot * thr;
  // column j: c_i = A_ij - sum_{k < j} L_jk U_ik (k ascending), d_j = c_j, U_ij = c_i, L_ij = c_i / d_j
  double Lm[6][6], U[6][6], d[6];
  bool ill = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
#pragma unroll
    for (int i = j; i < 6; ++i) {
      double c = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) c = c - Lm[j][k] * U[i][k];
      if (i == j) {
        d[j] = c;
      } else {
        U[i][j] = c;
        Lm[i][j] = c / d[j];
      }
    }
    ill = ill || d[j] <= thr;
  }
  if (ill) return 2;
  double y[6], x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double c = -v[21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) c = c - Lm[i][k] * y[k];
    y[i] = c;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double c = y[i] / d[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) c = c - Lm[k][i] * x[k];
    x[i] = c;
  }
  // delta = (omega, upsilon): dq = normalise(1, omega / 2); Rm <- R(dq) Rm; t <- R(dq) t + upsilon
  const double hx = 0.5 * x[0], hy = 0.5 * x[1], hz = 0.5 * x[2];
  const double nrm = sqrt(1.0 + hx * hx + hy * hy + hz * hz);
  const double dq[4] = {1.0 / nrm, hx / nrm, hy / nrm, hz / nrm};
  double D[3][3];
  pnp_rotation(dq[0], dq[1], dq[2], dq[3], false, D);
  double m2[3][3], t2[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) m2[r][c] = D[r][0] * m[0][c] + D[r][1] * m[1][c] + D[r][2] * m[2][c];
    t2[r] = D[r][0] * t[0] + D[r][1] * t[1] + D[r][2] * t[2] + x[3 + r];
  }
  // on the quaternion: q <- dq (x) q, or q (x) conj(dq) when the matrix is the transpose of q's
  double a4[4], b4[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a4[k] = inverse ? q[k] : dq[k];
    b4[k] = inverse ? (k == 0 ? dq[0] : -dq[k]) : q[k];
  }
  double q2[4];
  q2[0] = a4[0] * b4[0] - a4[1] * b4[1] - a4[2] * b4[2] - a4[3] * b4[3];
  q2[1] = a4[0] * b4[1] + a4[1] * b4[0] + a4[2] * b4[3] - a4[3] * b4[2];
  q2[2] = a4[0] * b4[2] - a4[1] * b4[3] + a4[2] * b4[0] + a4[3] * b4[1];
  q2[3] = a4[0] * b4[3] + a4[1] * b4[2] - a4[2] * b4[1] + a4[3] * b4[0];
  const double qn = sqrt(q2[0] * q2[0] + q2[1] * q2[1] + q2[2] * q2[2] + q2[3] * q2[3]);
  const double sg = (q2[0] < 0.0 ? -1.0 : 1.0) / qn;
#pragma unroll
  for (int k = 0; k < 4; ++k) q2[k] *= sg;
  ok = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) ok = ok && isfinite(m2[r][c]);
    ok = ok && isfinite(t2[r]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) ok = ok && isfinite(q2[k]);
  if (!ok) return -1;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) m[r][c] = m2[r][c];
    t[r] = t2[r];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = q2[k];
  return 1;
}

// One workgroup per (window position i, hop h).
__global__ __launch_bounds__(PNP_THREADS) void landmark_pnp_kernel(PnpArgs a) {
  __shared__ double lds[(PNP_WAVES - 1) * PNP_NV * 64];
  __shared__ double bc[12];
  __shared__ int bst;
  const int i = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
  const int N = a.N, T = a.T;
  if (i >= T || h >= a.n) return;
  const size_t f = (size_t)h * T + i;
  const float4 q0 = *reinterpret_cast<const float4*>(a.R0 + f * 4);
  double in[4], t[3], m[3][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) in[k] = a.intr[(size_t)h * 4 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = a.T0[f * 3 + k];
  double q[4] = {q0.x, q0.y, q0.z, q0.w};  // (followed by thread 0 only)
  pnp_rotation(q[0], q[1], q[2], q[3], a.inverse != 0, m);
  int st = 1;  // uniform over the workgroup
#pragma unroll
  for (int r = 0; r < 3; ++r)
    if (!(isfinite(m[r][0]) && isfinite(m[r][1]) && isfinite(m[r][2]) && isfinite(t[r]))) st = -1;

#pragma unroll 1
  for (int it = 0; it < a.iters && st == 1; ++it) {
    double v[PNP_NV];
#pragma unroll
    for (int k = 0; k < PNP_NV; ++k) v[k] = 0.0;
    for (int j = tid; j < N; j += PNP_THREADS) {
      PnpPoint p;
      if (!pnp_point(a, h, f, j, m, t, in, p)) continue;
      const double wh = p.rn <= a.huber ? 1.0 : a.huber / p.rn;
      const double ww = p.w * wh;
      // J = Jproj [ -[Xc]x | I ], Jproj = [[a0, 0, -c0], [0, a1, -c1]]
      const double x = p.xc[0], y = p.xc[1], z = p.xc[2];
      const double a0 = in[0] / z, a1 = in[1] / z;
      const double c0 = a0 * (x / z), c1 = a1 * (y / z);
      const double J0[6] = {-(c0 * y), a0 * z + c0 * x, -(a0 * y), a0, 0.0, -c0};
      const double J1[6] = {-(a1 * z) - c1 * y, c1 * x, a1 * x, 0.0, a1, -c1};
      int k = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) v[k++] += ww * (J0[r] * J0[c] + J1[r] * J1[c]);
#pragma unroll
      for (int r = 0; r < 6; ++r) v[21 + r] += ww * (J0[r] * p.r0 + J1[r] * p.r1);
      v[27] += 1.0;
    }
    pnp_reduce<PNP_NV>(v, lds);
    if (tid == 0) {
      const int s2 = v[27] < (double)a.min_pts ? 0 : pnp_step(v, a.min_pivot, a.inverse != 0, m, t, q);
      if (s2 == 1) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) bc[r * 3 + c] = m[r][c];
          bc[9 + r] = t[r];
        }
      }
      bst = s2;
    }
    __syncthreads();
    st = bst;
    if (st == 1) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[r][c] = bc[r * 3 + c];
        t[r] = bc[9 + r];
      }
    }
  }

  // the final pass at the refined pose: the inliers and the weighted rms residual
  double rms = 0.0;
  int nin = 0;
  if (st == 1) {
    double v[PNP_NF] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < N; j += PNP_THREADS) {
      PnpPoint p;
      if (!pnp_point(a, h, f, j, m, t, in, p)) continue;
      v[0] += 1.0;
      v[1] += p.rn <= a.huber ? 1.0 : 0.0;
      v[2] += p.w * (p.r0 * p.r0 + p.r1 * p.r1);
      v[3] += p.w;
    }
    pnp_reduce<PNP_NF>(v, lds);
    if (tid == 0) {
      rms = sqrt(v[2] / v[3]);  // (0 / 0 with no usable point: the count check below comes first, state 0)
      nin = (int)v[1];
      if (v[0] < (double)a.min_pts) st = 0;
      else if (!isfinite(rms)) st = -1;
    }
  }
  if (tid != 0) return;

  // outputs; every state other than 1 returns the input pose bit for bit
  const bool ok = st == 1;
  const float Rf[4] = {ok ? (float)q[0] : q0.x, ok ? (float)q[1] : q0.y, ok ? (float)q[2] : q0.z, ok ? (float)q[3] : q0.w};
  const double qd[4] = {ok ? q[0] : (double)q0.x, ok ? q[1] : (double)q0.y, ok ? q[2] : (double)q0.z,
                        ok ? q[3] : (double)q0.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a.q_out[f * 4 + k] = qd[k];
    a.R_out[f * 4 + k] = Rf[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) a.t_out[f * 3 + k] = ok ? t[k] : a.T0[f * 3 + k];
  a.n_in[f] = ok ? nin : 0;
  a.rms_px[f] = ok ? (float)rms : INFINITY;
  a.state_out[f] = st;

  // the feedback: one more hypothesis on the frame's fusion row, added as comet_pose_fuse adds one.
  // Positions [0, s) are final and stay as they are.
  if (ok && a.fuse_acc && a.inject_w > 0.0 && i >= a.s) {
    const int slot = a.slots[f];
    COMET_DASSERT(slot >= 0 && slot < a.rows);
    // (checked on the host too: never touch memory outside the accumulator ring)
    if ((unsigned)slot >= (unsigned)a.rows) return;
    const double x[3] = {a.fcx + a.ffx * t[0] / t[2], a.fcy + a.ffy * t[1] / t[2], t[2]};
    if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) return;
    double row[FUSE_ROW];
    load_row(a.fuse_acc + (size_t)slot * FUSE_ROW, row);
    add_hypothesis(row, a.inject_w, q, x);
    store_row(a.fuse_acc + (size_t)slot * FUSE_ROW, row);
  }
}

}  // namespace
}  // namespace comet

using namespace comet;

extern "C" int comet_landmark_pnp(const float* tracks, const float* weights, const double* X, const int32_t* state,
                                  const float* R0, const double* T0, const double* intr, const double* intr_host,
                                  int n, int Tw, int N, int s, int inverse_rotation, int iters, double huber_px,
                                  int min_pts, double min_pivot, double* fuse_acc, int rows, const int32_t* slots,
                                  const int32_t* slots_host, double inject_w, double fuse_fx, double fuse_fy,
                                  double fuse_cx, double fuse_cy, double* q_out, float* R_out, double* t_out,
                                  int32_t* n_in, float* rms_px, int32_t* state_out, void* stream) {
  COMET_CHECK_ARG(tracks && X && state && R0 && T0 && intr && intr_host && q_out && R_out && t_out && n_in && rms_px &&
                      state_out && (!fuse_acc || (slots && slots_host)),
                  "comet_landmark_pnp: null pointer");
  COMET_CHECK_ARG(n >= 1, "comet_landmark_pnp: n must be positive");
  COMET_CHECK_ARG(N >= 1 && N <= PNP_MAX_N, "comet_landmark_pnp: N outside [1, 4096]");
  COMET_CHECK_ARG(Tw >= 2, "comet_landmark_pnp: T must be at least 2");
  COMET_CHECK_ARG(s >= 1 && s <= Tw - 1, "comet_landmark_pnp: s outside [1, T - 1]");
  COMET_CHECK_ARG(iters >= 1 && iters <= PNP_MAX_ITERS, "comet_landmark_pnp: iters outside [1, 16]");
  COMET_CHECK_ARG(std::isfinite(huber_px) && huber_px > 0.0, "comet_landmark_pnp: huber_px must be finite and positive");
  COMET_CHECK_ARG(min_pts >= 4, "comet_landmark_pnp: min_pts must be at least 4");
  COMET_CHECK_ARG(min_pivot >= 0.0 && min_pivot < 1.0, "comet_landmark_pnp: min_pivot outside [0, 1)");
  COMET_CHECK_ARG(inverse_rotation == 0 || inverse_rotation == 1, "comet_landmark_pnp: inverse_rotation must be 0 or 1");
  for (int h = 0; h < n; ++h)
    COMET_CHECK_ARG(std::isfinite(intr_host[4 * h]) && intr_host[4 * h] > 0.0 && std::isfinite(intr_host[4 * h + 1]) &&
                        intr_host[4 * h + 1] > 0.0,
                    "comet_landmark_pnp: fx and fy must be finite and positive");
  if (fuse_acc) {
    COMET_CHECK_ARG(std::isfinite(inject_w) && inject_w >= 0.0, "comet_landmark_pnp: inject_w must be finite and >= 0");
    const int64_t count = (int64_t)n * Tw;
    for (int64_t j = 0; j < count; ++j)
      COMET_CHECK_ARG(slots_host[j] >= 0 && slots_host[j] < rows, "comet_landmark_pnp: slot index outside the ring");
    {  // two positions on one row would race
      std::vector<char> taken((size_t)rows, 0);
      for (int64_t j = 0; j < count; ++j) {
        COMET_CHECK_ARG(!taken[slots_host[j]], "comet_landmark_pnp: duplicate slot index");
        taken[slots_host[j]] = 1;
      }
    }
  }
  COMET_CHECK_ARG((((uintptr_t)tracks) & 7) == 0 && (((uintptr_t)R0 | (uintptr_t)fuse_acc) & 15) == 0 &&
                      (((uintptr_t)T0 | (uintptr_t)intr | (uintptr_t)X | (uintptr_t)q_out | (uintptr_t)t_out) & 7) == 0,
                  "comet_landmark_pnp: tracks, X, T0, intr, q and t must be 8-B aligned, R0 and fuse_acc 16-B aligned");
  PnpArgs a{};
  a.tracks = tracks; a.weights = weights; a.X = X; a.state = state; a.R0 = R0; a.T0 = T0; a.intr = intr;
  a.fuse_acc = fuse_acc; a.slots = fuse_acc ? slots : nullptr; a.q_out = q_out; a.R_out = R_out; a.t_out = t_out;
  a.n_in = n_in; a.rms_px = rms_px; a.state_out = state_out;
  a.huber = huber_px; a.min_pivot = min_pivot; a.inject_w = fuse_acc ? inject_w : 0.0;
  a.ffx = fuse_fx; a.ffy = fuse_fy; a.fcx = fuse_cx; a.fcy = fuse_cy;
  a.n = n; a.T = Tw; a.N = N; a.s = s; a.inverse = inverse_rotation; a.iters = iters; a.min_pts = min_pts;
  a.rows = fuse_acc ? rows : 0;
  hipLaunchKernelGGL(landmark_pnp_kernel, dim3((unsigned)Tw, (unsigned)n), dim3(PNP_THREADS), 0, as_stream(stream), a);
  COMET_CHECK_LAUNCH("comet_landmark_pnp");
  return COMET_OK;
}
