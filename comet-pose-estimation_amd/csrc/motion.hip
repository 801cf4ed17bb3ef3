// Motion estimate of the online path (comet_amd/stream.py MotionTracker, DESIGN.md "Motion estimate"):
// the fused poses of the frames that leave the window (comet_pose_fuse, positions [0, s)) are final and
// committed exactly once, so a short history of them is a time series. comet_motion_fit keeps that
// history per stream and fits a constant angular and linear velocity to its newest frames: a weighted
// line through the rotation vectors about a reference that the fit itself re-centres, and a weighted
// line through the translations. One wave of 64 threads per hop, lane k holds the frame of age k; the
// sums are a fixed shuffle tree. No LDS, no atomics, no communication between workgroups. The contract
// is in include/comet_hip.h; tests/motion_numpy.py restates it.
#include <cmath>

#include "common.hpp"

namespace comet {
namespace {

constexpr int MO_LANES = 64;
constexpr int MO_ROW = COMET_MOTION_ROW;  // doubles per history row
constexpr long long MO_FOLD = COMET_MOTION_COUNT_FOLD;

// Everything below is plain IEEE double evaluated as written (no contraction into fma):
// tests/motion_numpy.py restates it operation by operation.
#pragma clang fp contract(off)

struct MotionArgs {  // by value in the kernel arguments
  const float* R;          // [n, T, 4]
  const double* Tx;        // [n, T, 3]
  const float* weights;    // [n, T] or NULL
  const int* first;        // [n]
  const int* stream_idx;   // [n]
  double* hist;            // [S, cap, MO_ROW]
  int* hist_n;             // [S]
  double* omega;           // [n, 3]
  double* q0;              // [n, 4]
  double* vel;             // [n, 3]
  double* t0;              // [n, 3]
  float* rot_rms;          // [n]
  float* trans_rms;        // [n, 3]
  int* n_used;             // [n]
  int* state;              // [n]
  double* pred_q;          // [n, P, 4]
  double* pred_t;          // [n, P, 3]
  float* innov_rot;        // [n, T - s]
  float* innov_trans;      // [n, T - s]
  int S, cap, T, s, fit_len, min_frames, iters, horizon, inverse;
  double max_angle;
};

struct Quat {
  double w, x, y, z;
};

__device__ __forceinline__ Quat qmul(const Quat& a, const Quat& b) {  // Hamilton product, w first
  Quat r;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
  r.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
  return r;
}
__device__ __forceinline__ Quat qconj(const Quat& a) { return Quat{a.w, -a.x, -a.y, -a.z}; }

// phi = Log(d), d negated when its w < 0 -> theta in [0, pi]
__device__ __forceinline__ double qlog(Quat d, double (&phi)[3]) {
  if (d.w < 0.0) d = Quat{-d.w, -d.x, -d.y, -d.z};
  const double nv = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
  if (nv == 0.0) {
    phi[0] = phi[1] = phi[2] = 0.0;
    return 0.0;
  }
  const double theta = 2.0 * atan2(nv, d.w);
  const double f = theta / nv;
  phi[0] = f * d.x;
  phi[1] = f * d.y;
  phi[2] = f * d.z;
  return theta;
}

__device__ __forceinline__ Quat qexp(double px, double py, double pz) {
  const double theta = sqrt(px * px + py * py + pz * pz);
  if (theta == 0.0) return Quat{1.0, 0.0, 0.0, 0.0};
  const double half = 0.5 * theta;
  const double f = sin(half) / theta;
  return Quat{cos(half), f * px, f * py, f * pz};
}

// p[l] += p[l + d], d = 32 .. 1; lane 0's value to every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, MO_LANES);
  return __shfl(v, 0, MO_LANES);
}

__device__ __forceinline__ bool finite3(const double (&v)[3]) {
  return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
}

struct Frame {
  Quat q;
  double t[3];
  double w;
};

// the frame at window position i of hop h as the history stores it
__device__ __forceinline__ Frame load_frame(const MotionArgs& a, int h, int i) {
  const size_t f = (size_t)h * a.T + i;
  const float4 qf = *reinterpret_cast<const float4*>(a.R + f * 4);
  Frame r;
  r.q = Quat{(double)qf.x, (double)qf.y, (double)qf.z, (double)qf.w};
  if (a.inverse) r.q = qconj(r.q);
  r.t[0] = a.Tx[f * 3 + 0];
  r.t[1] = a.Tx[f * 3 + 1];
  r.t[2] = a.Tx[f * 3 + 2];
  const double w = a.weights ? (double)a.weights[f] : 1.0;
  const bool ok = isfinite(r.q.w) && isfinite(r.q.x) && isfinite(r.q.y) && isfinite(r.q.z) && isfinite(r.t[0]) &&
                  isfinite(r.t[1]) && isfinite(r.t[2]) && isfinite(w) && w > 0.0;
  r.w = ok ? w : 0.0;
  return r;
}

// weighted line x ~ x0 + slope tau through one component
__device__ __forceinline__ void line_fit(bool usable, double wk, double wt, double x, double Sw, double St, double D,
                                         double& slope, double& x0) {
  const double Sp = wave_sum(usable ? wk * x : 0.0);
  const double Stp = wave_sum(usable ? wt * x : 0.0);
  slope = (Sw * Stp - St * Sp) / D;
  x0 = (Sp - slope * St) / Sw;
}

__global__ __launch_bounds__(MO_LANES) void motion_fit_kernel(MotionArgs a) {
  const int h = blockIdx.x, k = threadIdx.x;
  const int T = a.T, s = a.s, cap = a.cap;
  const int sidx = a.stream_idx[h];
  COMET_DASSERT(sidx >= 0 && sidx < a.S);
  // (the stream indices are checked on the host too: never touch memory outside the state)
  if (sidx < 0 || sidx >= a.S) return;
  double* hist = a.hist + (size_t)sidx * cap * MO_ROW;
  long long c = a.first[h] ? 0 : a.hist_n[sidx];
  if (c < 0) c = 0;
  const long long c1 = c + s;  // frames committed after this hop; frame number f lives in row f % cap

  // append the positions [0, s); of more than cap frames only the newest cap reach the ring
  for (int i = k; i < s; i += MO_LANES) {
    if (s - i > cap) continue;
    const Frame fr = load_frame(a, h, i);
    const int row = (int)((c + i) % cap);
    COMET_DASSERT(row >= 0 && row < cap);
    double2* p = reinterpret_cast<double2*>(hist + (size_t)row * MO_ROW);
    p[0] = double2{fr.q.w, fr.q.x};
    p[1] = double2{fr.q.y, fr.q.z};
    p[2] = double2{fr.t[0], fr.t[1]};
    p[3] = double2{fr.t[2], fr.w};
  }
  if (k == 0) a.hist_n[sidx] = (int)(c1 < MO_FOLD ? c1 : cap + c1 % cap);

  // lane k: the frame of age k. The frames this hop appended come from its inputs, the older ones from
  // rows that the append above does not write (their ages are below cap), so no lane waits for another.
  const int m = (int)(c1 < a.fit_len ? c1 : a.fit_len);
  Frame fr;
  fr.q = Quat{1.0, 0.0, 0.0, 0.0};
  fr.t[0] = fr.t[1] = fr.t[2] = 0.0;
  fr.w = 0.0;
  if (k < m) {
    if (k < s) {
      fr = load_frame(a, h, s - 1 - k);
    } else {
      const int row = (int)((c1 - 1 - k) % cap);
      COMET_DASSERT(row >= 0 && row < cap);
      const double2* p = reinterpret_cast<const double2*>(hist + (size_t)row * MO_ROW);
      const double2 p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
      fr.q = Quat{p0.x, p0.y, p1.x, p1.y};
      fr.t[0] = p2.x; fr.t[1] = p2.y; fr.t[2] = p3.x;
      fr.w = p3.y;
    }
  }
  const bool usable = k < m && !(fr.w == 0.0);
  const unsigned long long mask = __ballot(usable);
  const int n_used = __popcll(mask);
  const double tau = -(double)k;
  const double wk = usable ? fr.w : 0.0;
  const double wt = wk * tau;

  // the newest committed pose: what every state other than 1 reports
  Quat qn;
  qn.w = __shfl(fr.q.w, 0, MO_LANES); qn.x = __shfl(fr.q.x, 0, MO_LANES);
  qn.y = __shfl(fr.q.y, 0, MO_LANES); qn.z = __shfl(fr.q.z, 0, MO_LANES);
  double tn[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) tn[j] = __shfl(fr.t[j], 0, MO_LANES);

  int st = 1;  // (every value a branch below tests is the same in all lanes)
  double om[3] = {0.0, 0.0, 0.0}, vel[3] = {0.0, 0.0, 0.0}, t0[3] = {tn[0], tn[1], tn[2]};
  Quat qr = qn;
  float rot_rms = INFINITY, trans_rms[3] = {INFINITY, INFINITY, INFINITY};
  double Sw = 0.0, St = 0.0, D = 0.0;
  if (n_used < a.min_frames) {
    st = 0;
  } else {
    Sw = wave_sum(usable ? wk : 0.0);
    St = wave_sum(usable ? wt : 0.0);
    const double Stt = wave_sum(usable ? wt * tau : 0.0);
    D = Sw * Stt - St * St;
    if (!(isfinite(Sw) && isfinite(St) && isfinite(Stt) && isfinite(D))) st = -1;
    else if (D <= 0.0) st = 2;
  }
  if (st == 1) {
    const int ref = __ffsll((long long)mask) - 1;  // the newest usable row
    qr.w = __shfl(fr.q.w, ref, MO_LANES); qr.x = __shfl(fr.q.x, ref, MO_LANES);
    qr.y = __shfl(fr.q.y, ref, MO_LANES); qr.z = __shfl(fr.q.z, ref, MO_LANES);
    double phi[3];
    for (int pass = 0; pass < a.iters && st == 1; ++pass) {
      const double theta = qlog(qmul(fr.q, qconj(qr)), phi);
      if (__any(usable && theta > a.max_angle)) {
        st = 3;
        break;
      }
      double off[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) line_fit(usable, wk, wt, phi[j], Sw, St, D, om[j], off[j]);
      if (!(finite3(om) && finite3(off))) {
        st = -1;
        break;
      }
      const Quat q = qmul(qexp(off[0], off[1], off[2]), qr);
      const double nrm = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
      const double sg = (q.w < 0.0 ? -1.0 : 1.0) / nrm;  // unit length, w >= 0: the fuser's sign rule
      qr = Quat{q.w * sg, q.x * sg, q.y * sg, q.z * sg};
      if (!(isfinite(qr.w) && isfinite(qr.x) && isfinite(qr.y) && isfinite(qr.z))) st = -1;
    }
    if (st == 1) {  // the residual against the final q0, which has absorbed the offset
      const double theta = qlog(qmul(fr.q, qconj(qr)), phi);
      if (__any(usable && theta > a.max_angle)) {
        st = 3;
      } else {
        const double r0 = phi[0] - om[0] * tau, r1 = phi[1] - om[1] * tau, r2 = phi[2] - om[2] * tau;
        const double rss = wave_sum(usable ? wk * (r0 * r0 + r1 * r1 + r2 * r2) : 0.0);
        const double rms = sqrt(rss / Sw);
        if (!isfinite(rms)) st = -1;
        rot_rms = (float)rms;
      }
    }
    if (st == 1) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        line_fit(usable, wk, wt, fr.t[j], Sw, St, D, vel[j], t0[j]);
        const double r = (fr.t[j] - t0[j]) - vel[j] * tau;
        const double rms = sqrt(wave_sum(usable ? wk * (r * r) : 0.0) / Sw);
        if (!(isfinite(vel[j]) && isfinite(t0[j]) && isfinite(rms))) st = -1;
        trans_rms[j] = (float)rms;
      }
    }
    if (st != 1) {
      qr = qn;
      rot_rms = INFINITY;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        om[j] = vel[j] = 0.0;
        t0[j] = tn[j];
        trans_rms[j] = INFINITY;
      }
    }
  }

  if (k == 0) {
    a.q0[h * 4 + 0] = qr.w; a.q0[h * 4 + 1] = qr.x; a.q0[h * 4 + 2] = qr.y; a.q0[h * 4 + 3] = qr.z;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      a.omega[h * 3 + j] = om[j];
      a.vel[h * 3 + j] = vel[j];
      a.t0[h * 3 + j] = t0[j];
      a.trans_rms[h * 3 + j] = trans_rms[j];
    }
    a.rot_rms[h] = rot_rms;
    a.n_used[h] = n_used;
    a.state[h] = st;
  }

  // predictions at tau = 1 .. P after the newest committed frame; the first T - s of them are the window
  // positions [s, T), whose fused pose of this push gives the innovation
  const int P = T - s + a.horizon;
  for (int j = k; j < P; j += MO_LANES) {
    const double tp = (double)(j + 1);
    Quat pq = st == 1 ? qmul(qexp(om[0] * tp, om[1] * tp, om[2] * tp), qr) : qr;
    if (a.inverse) pq = qconj(pq);
    double pt[3] = {t0[0], t0[1], t0[2]};
    if (st == 1) {
#pragma unroll
      for (int c3 = 0; c3 < 3; ++c3) pt[c3] = t0[c3] + vel[c3] * tp;
    }
    const size_t o = (size_t)h * P + j;
    a.pred_q[o * 4 + 0] = pq.w; a.pred_q[o * 4 + 1] = pq.x; a.pred_q[o * 4 + 2] = pq.y; a.pred_q[o * 4 + 3] = pq.z;
    a.pred_t[o * 3 + 0] = pt[0]; a.pred_t[o * 3 + 1] = pt[1]; a.pred_t[o * 3 + 2] = pt[2];
    if (j < T - s) {
      float ir = INFINITY, it = INFINITY;
      if (st == 1) {
        const size_t f = (size_t)h * T + s + j;
        const float4 qf = *reinterpret_cast<const float4*>(a.R + f * 4);
        double phi[3];
        ir = (float)qlog(qmul(Quat{(double)qf.x, (double)qf.y, (double)qf.z, (double)qf.w}, qconj(pq)), phi);
        const double dx = a.Tx[f * 3 + 0] - pt[0], dy = a.Tx[f * 3 + 1] - pt[1], dz = a.Tx[f * 3 + 2] - pt[2];
        it = (float)sqrt(dx * dx + dy * dy + dz * dz);
      }
      a.innov_rot[(size_t)h * (T - s) + j] = ir;
      a.innov_trans[(size_t)h * (T - s) + j] = it;
    }
  }
}

}  // namespace
}  // namespace comet

using namespace comet;

extern "C" int comet_motion_fit(const float* R, const double* T, const float* weights, const int32_t* first,
                                const int32_t* stream_idx, const int32_t* stream_idx_host, double* hist,
                                int32_t* hist_n, int S, int cap, int n, int Tw, int s, int fit_len, int min_frames,
                                int iters, int horizon, double max_angle, int inverse_rotation, double* omega,
                                double* q0, double* vel, double* t0, float* rot_rms, float* trans_rms, int32_t* n_used,
                                int32_t* state, double* pred_q, double* pred_t, float* innov_rot, float* innov_trans,
                                void* stream) {
  COMET_CHECK_ARG(R && T && first && stream_idx && stream_idx_host && hist && hist_n && omega && q0 && vel && t0 &&
                      rot_rms && trans_rms && n_used && state && pred_q && pred_t && innov_rot && innov_trans,
                  "comet_motion_fit: null pointer");
  COMET_CHECK_ARG(n >= 1, "comet_motion_fit: n must be positive");
  COMET_CHECK_ARG(Tw >= 2, "comet_motion_fit: T must be at least 2");
  COMET_CHECK_ARG(s >= 1 && s <= Tw - 1, "comet_motion_fit: s outside [1, T - 1]");
  COMET_CHECK_ARG(cap >= 2 && cap <= MO_LANES, "comet_motion_fit: cap outside [2, 64]");
  COMET_CHECK_ARG(fit_len >= 2 && fit_len <= cap, "comet_motion_fit: fit_len outside [2, cap]");
  COMET_CHECK_ARG(min_frames >= 2 && min_frames <= fit_len, "comet_motion_fit: min_frames outside [2, fit_len]");
  COMET_CHECK_ARG(iters >= 1 && iters <= COMET_MOTION_MAX_ITERS, "comet_motion_fit: iters outside [1, 8]");
  COMET_CHECK_ARG(horizon >= 0 && horizon <= COMET_MOTION_MAX_HORIZON, "comet_motion_fit: horizon outside [0, 64]");
  COMET_CHECK_ARG(max_angle > 0.0 && max_angle < 3.14159265358979323846, "comet_motion_fit: max_angle outside (0, pi)");
  COMET_CHECK_ARG(inverse_rotation == 0 || inverse_rotation == 1, "comet_motion_fit: inverse_rotation must be 0 or 1");
  for (int h = 0; h < n; ++h) {  // two hops on one stream's ring would race (n is a handful: compared pairwise)
    COMET_CHECK_ARG(stream_idx_host[h] >= 0 && stream_idx_host[h] < S, "comet_motion_fit: stream index outside the state");
    for (int g = 0; g < h; ++g)
      COMET_CHECK_ARG(stream_idx_host[g] != stream_idx_host[h], "comet_motion_fit: duplicate stream index");
  }
  COMET_CHECK_ARG((((uintptr_t)R | (uintptr_t)hist) & 15) == 0 &&
                      (((uintptr_t)T | (uintptr_t)omega | (uintptr_t)q0 | (uintptr_t)vel | (uintptr_t)t0 |
                        (uintptr_t)pred_q | (uintptr_t)pred_t) & 7) == 0,
                  "comet_motion_fit: R and hist must be 16-B aligned, T and the f64 outputs 8-B aligned");
  MotionArgs a{};
  a.R = R; a.Tx = T; a.weights = weights; a.first = first; a.stream_idx = stream_idx; a.hist = hist; a.hist_n = hist_n;
  a.omega = omega; a.q0 = q0; a.vel = vel; a.t0 = t0; a.rot_rms = rot_rms; a.trans_rms = trans_rms; a.n_used = n_used;
  a.state = state; a.pred_q = pred_q; a.pred_t = pred_t; a.innov_rot = innov_rot; a.innov_trans = innov_trans;
  a.S = S; a.cap = cap; a.T = Tw; a.s = s; a.fit_len = fit_len; a.min_frames = min_frames; a.iters = iters;
  a.horizon = horizon; a.inverse = inverse_rotation; a.max_angle = max_angle;
  hipLaunchKernelGGL(motion_fit_kernel, dim3((unsigned)n), dim3(MO_LANES), 0, as_stream(stream), a);
  COMET_CHECK_LAUNCH("comet_motion_fit");
  return COMET_OK;
}
