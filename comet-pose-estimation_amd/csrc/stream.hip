// Frame ring of the online path (comet_amd/stream.py, DESIGN.md "Online / streaming inference"):
// the per-frame tensors of the last `capacity` frames live in device rings; a hop needs the T
// slots of its window contiguous. comet_ring_gather copies them for up to 4 rings in one launch.
// comet_ring_scatter is its inverse: the k new frames of a push (StreamPool: one per stream) go
// from contiguous rows into their ring slots, for up to 4 rings in one launch.
// comet_pose_fuse (DESIGN.md "Pose fusion") keeps one accumulator row per ring slot and turns the
// overlapping windows' poses into one fused pose per frame, all hops of a push in one launch.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "fuse_row.hpp"

namespace comet {
namespace {

constexpr int RING_MAX = COMET_RING_MAX_TENSORS;
constexpr int RING_THREADS = 256;
constexpr int RING_UNROLL = 4;                             // 16-B vectors per thread and tile
constexpr unsigned RING_TILE = RING_THREADS * RING_UNROLL;  // vectors per tile (16 KiB)

struct RingArgs {  // by value in the kernel arguments
  const u32x4* src[RING_MAX];
  u32x4* dst[RING_MAX];
  unsigned nv[RING_MAX];   // 16-B vectors per slot
  unsigned tps[RING_MAX];  // tiles per slot
  const int* slots;        // [T] device
  int count, T, capacity;
};

// Work = tiles of RING_TILE vectors, numbered tensor-major, then window position, then offset in
// the slot. A workgroup takes tiles blockIdx.x, + gridDim.x, ... and keeps (tensor, position,
// tile in slot) up to date by subtraction (no division: every quantity here is wave-uniform).
__global__ __launch_bounds__(RING_THREADS) void ring_gather_kernel(RingArgs a) {
  int t = 0, j = 0;
  unsigned c = blockIdx.x;
  for (;;) {
    while (t < a.count && c >= a.tps[t]) {
      c -= a.tps[t];
      if (++j == a.T) {
        j = 0;
        ++t;
      }
    }
    if (t >= a.count) return;
    const int slot = a.slots[j];
    COMET_DASSERT(slot >= 0 && slot < a.capacity);
    if ((unsigned)slot < (unsigned)a.capacity) {  // (checked on the host too: never read outside the ring)
      const unsigned nv = a.nv[t];
      const u32x4* s = a.src[t] + (size_t)slot * nv;
      u32x4* d = a.dst[t] + (size_t)j * nv;
      const unsigned i0 = c * RING_TILE + threadIdx.x;
      u32x4 v[RING_UNROLL];
#pragma unroll
      for (int u = 0; u < RING_UNROLL; ++u) {
        const unsigned i = i0 + u * RING_THREADS;
        if (i < nv) v[u] = s[i];
      }
#pragma unroll
      for (int u = 0; u < RING_UNROLL; ++u) {
        const unsigned i = i0 + u * RING_THREADS;
        if (i < nv) __builtin_nontemporal_store(v[u], d + i);
      }
    }
    c += gridDim.x;
  }
}

// The inverse: row j of the contiguous src [k, slot] block goes to ring slot slots[j]; a.T holds k.
// Same tiling and tile numbering (tensor-major, then row, then offset in the row). The stores are
// plain: the gather of the same push reads these slots again, and a plain store leaves the line in
// the XCD's L2. The host has checked that the k slots are distinct, so no two rows share a target.
__global__ __launch_bounds__(RING_THREADS) void ring_scatter_kernel(RingArgs a) {
  int t = 0, j = 0;
  unsigned c = blockIdx.x;
  for (;;) {
    while (t < a.count && c >= a.tps[t]) {
      c -= a.tps[t];
      if (++j == a.T) {
        j = 0;
        ++t;
      }
    }
    if (t >= a.count) return;
    const int slot = a.slots[j];
    COMET_DASSERT(slot >= 0 && slot < a.capacity);
    if ((unsigned)slot < (unsigned)a.capacity) {  // (checked on the host too: never write outside the ring)
      const unsigned nv = a.nv[t];
      const u32x4* s = a.src[t] + (size_t)j * nv;
      u32x4* d = a.dst[t] + (size_t)slot * nv;
      const unsigned i0 = c * RING_TILE + threadIdx.x;
      u32x4 v[RING_UNROLL];
#pragma unroll
      for (int u = 0; u < RING_UNROLL; ++u) {
        const unsigned i = i0 + u * RING_THREADS;
        if (i < nv) v[u] = s[i];
      }
#pragma unroll
      for (int u = 0; u < RING_UNROLL; ++u) {
        const unsigned i = i0 + u * RING_THREADS;
        if (i < nv) d[i] = v[u];
      }
    }
    c += gridDim.x;
  }
}

// ---- pose fusion --------------------------------------------------------------------------------
constexpr int FUSE_THREADS = 64;
constexpr int FUSE_SWEEPS = 8;            // cyclic Jacobi sweeps of the 4 x 4 problem

// Everything from here to the end of the file is plain IEEE double evaluated as written (no
// contraction into fma): tests/fuse_numpy.py restates the accumulation operation by operation.
#pragma clang fp contract(off)

struct FuseArgs {  // by value in the kernel arguments
  const float* enc;          // [n * T, 7]
  const int* slots;          // [n * T]
  const int* fresh;          // [n]
  const int* first;          // [n]
  const double* anchors;     // [n, 7] (q[4], u, v, z)
  const float* weights;      // [n * T] or NULL
  const double* ratio_dev;   // or NULL
  double ratio, fx, fy, cx, cy;
  double* acc;               // [rows, FUSE_ROW]
  float* R;                  // [n * T, 4]
  double* uvz;               // [n * T, 3]
  double* Tx;                // [n * T, 3]
  int* count;                // [n * T]
  float* rot_spread;         // [n * T]
  float* trans_spread;       // [n * T, 3]
  float* hyp_R;              // [n * T, 4]
  double* hyp_T;             // [n * T, 3]
  int n, T, rows;
};

struct FusedPose {
  double q[4], uvz[3], lam, W;
};

// One Jacobi rotation of the symmetric a (both triangles kept) in the (P, Q) plane; v collects the
// eigenvectors as columns. P, Q are template constants so that every index is one.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (apq == 0.0 || !(fabs(theta) < 1e150)) t = (apq == 0.0) ? 0.0 : 0.5 / theta;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k != P && k != Q) {
      const double akp = a[k][P], akq = a[k][Q];
      a[k][P] = a[P][k] = c * akp - s * akq;
      a[k][Q] = a[Q][k] = s * akp + c * akq;
    }
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq;
    v[k][Q] = s * vkp + c * vkq;
  }
}

// The fused pose of one accumulator row r (FUSE_ROW doubles, in registers): the eigenvector of the
// largest eigenvalue of sum w q q^T (lowest index among equal ones), w >= 0 as qmul_std leaves its
// product, and the weighted mean of (u, v, z).
__device__ __forceinline__ FusedPose fuse_row(const double (&r)[FUSE_ROW]) {
  double a[4][4] = {{r[1], r[2], r[3], r[4]}, {r[2], r[5], r[6], r[7]}, {r[3], r[6], r[8], r[9]}, {r[4], r[7], r[9], r[10]}};
  double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  // the six rotations of a sweep are unrolled with constant indices, so a and v stay in registers;
  // the sweep loop itself stays rolled (unrolled: 256 VGPRs + 34 AGPRs instead of 134 VGPRs)
#pragma unroll 1
  for (int sweep = 0; sweep < FUSE_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<0, 3>(a, v);
    jacobi_rotate<1, 2>(a, v);
    jacobi_rotate<1, 3>(a, v);
    jacobi_rotate<2, 3>(a, v);
  }
  FusedPose f;
  f.lam = a[0][0];
#pragma unroll
  for (int k = 0; k < 4; ++k) f.q[k] = v[k][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const bool up = a[j][j] > f.lam;  // strict: the lowest index wins a tie
    f.lam = up ? a[j][j] : f.lam;
#pragma unroll
    for (int k = 0; k < 4; ++k) f.q[k] = up ? v[k][j] : f.q[k];
  }
  const double nrm = sqrt(f.q[0] * f.q[0] + f.q[1] * f.q[1] + f.q[2] * f.q[2] + f.q[3] * f.q[3]);
  const double sg = (f.q[0] < 0.0 ? -1.0 : 1.0) / nrm;
#pragma unroll
  for (int k = 0; k < 4; ++k) f.q[k] *= sg;
  f.W = r[0];
#pragma unroll
  for (int k = 0; k < 3; ++k) f.uvz[k] = r[11 + k] / f.W;
  return f;
}

__device__ __forceinline__ void zero_row(double (&r)[FUSE_ROW]) {
#pragma unroll
  for (int k = 0; k < FUSE_ROW; ++k) r[k] = 0.0;
}

// One thread per (hop, window position).
__global__ __launch_bounds__(FUSE_THREADS) void pose_fuse_kernel(FuseArgs a) {
  const int t = blockIdx.x * FUSE_THREADS + threadIdx.x;
  if (t >= a.n * a.T) return;
  const int hop = t / a.T, i = t - hop * a.T;
  const int slot0 = a.slots[hop * a.T], slot = a.slots[t];
  COMET_DASSERT(slot0 >= 0 && slot0 < a.rows && slot >= 0 && slot < a.rows);
  // (checked on the host too: never touch memory outside the accumulator ring)
  if ((unsigned)slot0 >= (unsigned)a.rows || (unsigned)slot >= (unsigned)a.rows) return;
  const double ratio = a.ratio_dev ? *a.ratio_dev : a.ratio;
  const bool first = a.first[hop] != 0;
  const int fresh = a.fresh[hop];
  double row[FUSE_ROW];

  // 1. the reference: the anchor (first hop), else the fused pose of position 0's row, which no
  //    thread of this launch writes
  double qr[4], xr[3];
  FusedPose f;
  if (first) {
    const double* an = a.anchors + (size_t)hop * 7;
#pragma unroll
    for (int k = 0; k < 4; ++k) qr[k] = an[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) xr[k] = an[4 + k];
  } else {
    load_row(a.acc + (size_t)slot0 * FUSE_ROW, row);
    f = fuse_row(row);
#pragma unroll
    for (int k = 0; k < 4; ++k) qr[k] = f.q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) xr[k] = f.uvz[k];
  }

  // 2. this window's hypothesis for the frame, by the codec's composition (pose_decode_kernel)
  double q[4], x[3];
  if (i == 0) {  // the reference itself
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = qr[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = xr[k];
  } else {
    const float* e = a.enc + (size_t)t * 7;
    const double ew = e[3], ex = e[4], ey = e[5], ez = e[6];
    q[0] = ew * qr[0] - ex * qr[1] - ey * qr[2] - ez * qr[3];
    q[1] = ew * qr[1] + ex * qr[0] + ey * qr[3] - ez * qr[2];
    q[2] = ew * qr[2] - ex * qr[3] + ey * qr[0] + ez * qr[1];
    q[3] = ew * qr[3] + ex * qr[2] - ey * qr[1] + ez * qr[0];
    x[0] = xr[0] + (double)e[0] / ratio * 128.0;
    x[1] = xr[1] + (double)e[1] / ratio * 128.0;
    x[2] = xr[2] * ((double)e[2] / ratio + 1.0);
  }
  {  // unit length (the product of the normalised factors, up to rounding), w >= 0
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sg = (q[0] < 0.0 ? -1.0 : 1.0) / nrm;
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] *= sg;
  }

  // 3. accumulate. Position 0 is written by a first hop only (the anchor, weight 1).
  if (i == 0) {
    if (first) {
      zero_row(row);
      add_hypothesis(row, 1.0, q, x);
      store_row(a.acc + (size_t)slot * FUSE_ROW, row);
      f = fuse_row(row);
    }
  } else {
    const double w = a.weights ? (double)a.weights[t] : 1.0;
    if (i >= fresh)  // a new frame, or a slot that held an older one
      zero_row(row);
    else
      load_row(a.acc + (size_t)slot * FUSE_ROW, row);
    add_hypothesis(row, w, q, x);
    store_row(a.acc + (size_t)slot * FUSE_ROW, row);
    f = fuse_row(row);
  }

  // 4. outputs: the row's fused pose and this window's own hypothesis
  const double W = f.W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a.R[(size_t)t * 4 + k] = (float)f.q[k];
    a.hyp_R[(size_t)t * 4 + k] = (float)q[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.uvz[(size_t)t * 3 + k] = f.uvz[k];
    const double var = row[14 + k] / W - f.uvz[k] * f.uvz[k];
    a.trans_spread[(size_t)t * 3 + k] = (float)sqrt(fmax(0.0, var));
  }
  a.Tx[(size_t)t * 3 + 0] = (f.uvz[0] - a.cx) * f.uvz[2] / a.fx;
  a.Tx[(size_t)t * 3 + 1] = (f.uvz[1] - a.cy) * f.uvz[2] / a.fy;
  a.Tx[(size_t)t * 3 + 2] = f.uvz[2];
  a.hyp_T[(size_t)t * 3 + 0] = (x[0] - a.cx) * x[2] / a.fx;
  a.hyp_T[(size_t)t * 3 + 1] = (x[1] - a.cy) * x[2] / a.fy;
  a.hyp_T[(size_t)t * 3 + 2] = x[2];
  a.count[t] = (int)row[17];
  a.rot_spread[t] = (float)(2.0 * asin(sqrt(fmin(1.0, fmax(0.0, 1.0 - f.lam / W)))));
}

int ring_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      cus = n;
    else
      cus = 256;
  }
  return cus;
}

}  // namespace
}  // namespace comet

using namespace comet;

extern "C" int comet_ring_gather(const CometRingTensor* tensors, int n_tensors, const int32_t* slots,
                                 const int32_t* slots_host, int T, int capacity, int max_blocks, void* stream) {
  COMET_CHECK_ARG(tensors && slots && slots_host, "comet_ring_gather: null pointer");
  COMET_CHECK_ARG(n_tensors >= 1 && n_tensors <= RING_MAX, "comet_ring_gather: 1 to 4 tensors per launch");
  COMET_CHECK_ARG(T > 0, "comet_ring_gather: T must be positive");
  COMET_CHECK_ARG(capacity >= T, "comet_ring_gather: capacity below T");
  COMET_CHECK_ARG(max_blocks >= 0, "comet_ring_gather: negative max_blocks");
  for (int j = 0; j < T; ++j)
    COMET_CHECK_ARG(slots_host[j] >= 0 && slots_host[j] < capacity, "comet_ring_gather: slot index outside the ring");
  RingArgs a{};
  a.slots = slots;
  a.count = n_tensors;
  a.T = T;
  a.capacity = capacity;
  int64_t tiles = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const CometRingTensor& r = tensors[i];
    COMET_CHECK_ARG(r.src && r.dst, "comet_ring_gather: null tensor");
    COMET_CHECK_ARG(r.slot_bytes > 0 && r.slot_bytes % 16 == 0,
                    "comet_ring_gather: slot_bytes must be a positive multiple of 16");
    COMET_CHECK_ARG((((uintptr_t)r.src | (uintptr_t)r.dst) & 15) == 0, "comet_ring_gather: pointers must be 16-B aligned");
    const int64_t nv = r.slot_bytes / 16;
    COMET_CHECK_ARG(nv < (int64_t(1) << 31), "comet_ring_gather: slot too large");
    a.src[i] = reinterpret_cast<const u32x4*>(r.src);
    a.dst[i] = reinterpret_cast<u32x4*>(r.dst);
    a.nv[i] = (unsigned)nv;
    a.tps[i] = (unsigned)cdiv(nv, RING_TILE);
    tiles += (int64_t)a.tps[i] * T;
  }
  COMET_CHECK_ARG(tiles < (int64_t(1) << 31), "comet_ring_gather: window too large");
  // memory-bound: 4 workgroups (16 waves, 64 KiB of loads in flight) per CU, grid-stride over the rest
  int64_t grid = max_blocks > 0 ? max_blocks : 4 * (int64_t)ring_cus();
  if (grid > tiles) grid = tiles;
  hipLaunchKernelGGL(ring_gather_kernel, dim3((unsigned)grid), dim3(RING_THREADS), 0, as_stream(stream), a);
  COMET_CHECK_LAUNCH("comet_ring_gather");
  return COMET_OK;
}

extern "C" int comet_ring_scatter(const CometRingTensor* tensors, int n_tensors, const int32_t* slots,
                                  const int32_t* slots_host, int k, int capacity, int max_blocks, void* stream) {
  COMET_CHECK_ARG(tensors && slots && slots_host, "comet_ring_scatter: null pointer");
  COMET_CHECK_ARG(n_tensors >= 1 && n_tensors <= RING_MAX, "comet_ring_scatter: 1 to 4 tensors per launch");
  COMET_CHECK_ARG(k > 0, "comet_ring_scatter: k must be positive");
  COMET_CHECK_ARG(capacity >= k, "comet_ring_scatter: capacity below k");
  COMET_CHECK_ARG(max_blocks >= 0, "comet_ring_scatter: negative max_blocks");
  for (int j = 0; j < k; ++j)
    COMET_CHECK_ARG(slots_host[j] >= 0 && slots_host[j] < capacity, "comet_ring_scatter: slot index outside the ring");
  {  // two rows for one slot would race
    std::vector<char> taken((size_t)capacity, 0);
    for (int j = 0; j < k; ++j) {
      COMET_CHECK_ARG(!taken[slots_host[j]], "comet_ring_scatter: duplicate slot index");
      taken[slots_host[j]] = 1;
    }
  }
  RingArgs a{};
  a.slots = slots;
  a.count = n_tensors;
  a.T = k;
  a.capacity = capacity;
  int64_t tiles = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const CometRingTensor& r = tensors[i];
    COMET_CHECK_ARG(r.src && r.dst, "comet_ring_scatter: null tensor");
    COMET_CHECK_ARG(r.slot_bytes > 0 && r.slot_bytes % 16 == 0,
                    "comet_ring_scatter: slot_bytes must be a positive multiple of 16");
    COMET_CHECK_ARG((((uintptr_t)r.src | (uintptr_t)r.dst) & 15) == 0, "comet_ring_scatter: pointers must be 16-B aligned");
    const int64_t nv = r.slot_bytes / 16;
    COMET_CHECK_ARG(nv < (int64_t(1) << 31), "comet_ring_scatter: slot too large");
    a.src[i] = reinterpret_cast<const u32x4*>(r.src);
    a.dst[i] = reinterpret_cast<u32x4*>(r.dst);
    a.nv[i] = (unsigned)nv;
    a.tps[i] = (unsigned)cdiv(nv, RING_TILE);
    tiles += (int64_t)a.tps[i] * k;
  }
  COMET_CHECK_ARG(tiles < (int64_t(1) << 31), "comet_ring_scatter: block too large");
  int64_t grid = max_blocks > 0 ? max_blocks : 4 * (int64_t)ring_cus();
  if (grid > tiles) grid = tiles;
  hipLaunchKernelGGL(ring_scatter_kernel, dim3((unsigned)grid), dim3(RING_THREADS), 0, as_stream(stream), a);
  COMET_CHECK_LAUNCH("comet_ring_scatter");
  return COMET_OK;
}

extern "C" int comet_pose_fuse(const float* enc, const int32_t* slots, const int32_t* slots_host,
                               const int32_t* fresh_from, const int32_t* fresh_from_host, const int32_t* first,
                               const int32_t* first_host, const double* anchors, const float* weights, double ratio,
                               const double* ratio_dev, double fx, double fy, double cx, double cy, double* acc,
                               int rows, int n, int T, float* R_out, double* uvz_out, double* T_out,
                               int32_t* count_out, float* rot_spread, float* trans_spread, float* hyp_R,
                               double* hyp_T, void* stream) {
  COMET_CHECK_ARG(enc && slots && slots_host && fresh_from && fresh_from_host && first && first_host && anchors &&
                      acc && R_out && uvz_out && T_out && count_out && rot_spread && trans_spread && hyp_R && hyp_T,
                  "comet_pose_fuse: null pointer");
  COMET_CHECK_ARG(n > 0, "comet_pose_fuse: n must be positive");
  COMET_CHECK_ARG(T >= 2, "comet_pose_fuse: T must be at least 2");
  COMET_CHECK_ARG(rows > 0, "comet_pose_fuse: rows must be positive");
  for (int h = 0; h < n; ++h) {
    COMET_CHECK_ARG(fresh_from_host[h] >= 1 && fresh_from_host[h] <= T, "comet_pose_fuse: fresh_from outside [1, T]");
    COMET_CHECK_ARG(first_host[h] == 0 || (first_host[h] == 1 && fresh_from_host[h] == 1),
                    "comet_pose_fuse: first must be 0 or 1, and a first hop has fresh_from 1");
  }
  for (int64_t j = 0; j < (int64_t)n * T; ++j)
    COMET_CHECK_ARG(slots_host[j] >= 0 && slots_host[j] < rows, "comet_pose_fuse: slot index outside the ring");
  {  // two positions for one row would race
    std::vector<char> taken((size_t)rows, 0);
    for (int64_t j = 0; j < (int64_t)n * T; ++j) {
      COMET_CHECK_ARG(!taken[slots_host[j]], "comet_pose_fuse: duplicate slot index");
      taken[slots_host[j]] = 1;
    }
  }
  if (!ratio_dev) COMET_CHECK_ARG(std::isfinite(ratio) && ratio > 0.0, "comet_pose_fuse: ratio must be finite and positive");
  COMET_CHECK_ARG((((uintptr_t)acc) & 15) == 0, "comet_pose_fuse: acc must be 16-B aligned");
  FuseArgs a{};
  a.enc = enc;
  a.slots = slots;
  a.fresh = fresh_from;
  a.first = first;
  a.anchors = anchors;
  a.weights = weights;
  a.ratio_dev = ratio_dev;
  a.ratio = ratio;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
  a.acc = acc;
  a.R = R_out; a.uvz = uvz_out; a.Tx = T_out; a.count = count_out;
  a.rot_spread = rot_spread; a.trans_spread = trans_spread; a.hyp_R = hyp_R; a.hyp_T = hyp_T;
  a.n = n; a.T = T; a.rows = rows;
  const int64_t grid = cdiv((int64_t)n * T, FUSE_THREADS);
  hipLaunchKernelGGL(pose_fuse_kernel, dim3((unsigned)grid), dim3(FUSE_THREADS), 0, as_stream(stream), a);
  COMET_CHECK_LAUNCH("comet_pose_fuse");
  return COMET_OK;
}
