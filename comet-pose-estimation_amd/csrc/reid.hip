// Landmark archive of the online path (comet_amd/stream.py LandmarkMap, DESIGN.md "Landmark archive"): the
// accumulator row of a track that dies is retired to a per-stream ring of archive entries, and a track born
// on the projection of an archived landmark gets that landmark's row and identity back.
// comet_landmark_reid does both for the n hops of a push in one launch, between that push's
// comet_pose_fuse and comet_landmark_update launches: one workgroup of 256 threads per hop, no communication
// between workgroups, no global atomics. Slot j is always handled by thread j % 256. The contract is in
// include/comet_hip.h; tests/reid_numpy.py restates it.
#include <cmath>

#include "common.hpp"
#include "lm_solve.hpp"

namespace comet {
namespace {

constexpr int REID_THREADS = 256;
constexpr int REID_WAVES = REID_THREADS / 64;
constexpr int REID_MAX_N = COMET_CARRY_MAX_TRACKS;
constexpr int REID_MAX_C = COMET_LM_ARCH_MAX;
constexpr int ARCH_ROW = COMET_LM_ARCH_ROW;  // doubles per archive entry
constexpr unsigned char ENTRY_IN_USE = 1, ENTRY_CANDIDATE = 2;

// Everything below is plain IEEE double evaluated as written (no contraction into fma), only + - * / and
// sqrt: tests/reid_numpy.py restates it operation by operation.
#pragma clang fp contract(off)

struct ReidArgs {  // by value in the kernel arguments
  const float* tracks;    // [n, T, N, 2]
  const float* R;         // [n, T, 4]
  const double* Tx;       // [n, T, 3]
  const int* ids;         // [n, N]
  const int* src;         // [n, N]
  const int* stream_idx;  // [n]
  const double* intr;     // [n, 4]
  double* acc;            // [rows, LM_ROW]
  int* acc_id;            // [rows]
  int* alias;             // [rows]
  double* arch;           // [entries, ARCH_ROW]
  int* arch_id;           // [entries]
  int* arch_cursor;       // [min(rows / N, entries / C)]
  double* ws;             // [n, N, LM_ROW]
  int* src_lm;            // [n, N]
  int* lm_id;             // [n, N]
  int* state;             // [n, N]
  float* dist;            // [n, N]
  int* stats;             // [n, 4]
  int T, N, C, rows, entries, inverse, arch_min_obs;
  double min_pivot, reid_px, min_cos;
};

// LDS of one workgroup, carved from the dynamic allocation: 21 C + 12 N bytes (132 KiB at C = N = 4096)
__host__ __device__ constexpr size_t reid_lds_bytes(int N, int C) {
  return (size_t)C * 16 + (size_t)C * 4 + (size_t)N * 12 + (((size_t)C + 7) & ~(size_t)7);
}

// Exclusive prefix sum of a 0 / 1 flag over the workgroup (thread order) and the workgroup's total (the
// scheme of comet_track_carry). Every thread of the workgroup must call it (two barriers).
__device__ __forceinline__ int reid_scan(bool flag, int* wsum, int& total) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int off = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < REID_WAVES; ++i) {
    const int v = wsum[i];
    off += i < w ? v : 0;
    total += v;
  }
  __syncthreads();
  return off + pre;
}

// x_cam = Rm X + t
__device__ __forceinline__ void reid_to_camera(const double (&m)[3][3], const double (&t)[3], const double (&X)[3],
                                               double (&xc)[3]) {
  xc[0] = m[0][0] * X[0] + m[0][1] * X[1] + m[0][2] * X[2] + t[0];
  xc[1] = m[1][0] * X[0] + m[1][1] * X[1] + m[1][2] * X[2] + t[1];
  xc[2] = m[2][0] * X[0] + m[2][1] * X[1] + m[2][2] * X[2] + t[2];
}

// unit vector from X to the camera centre c
__device__ __forceinline__ void reid_view_dir(const double (&c)[3], const double (&X)[3], double (&d)[3]) {
  const double v0 = c[0] - X[0], v1 = c[1] - X[1], v2 = c[2] - X[2];
  const double nv = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  d[0] = v0 / nv; d[1] = v1 / nv; d[2] = v2 / nv;
}

__device__ __forceinline__ double reid_dist2(double ex, double ey, float2 p) {
  const double du = ex - (double)p.x, dv = ey - (double)p.y;
  return du * du + dv * dv;
}

__device__ __forceinline__ void reid_load_row(const double* p, double (&r)[LM_ROW]) {
#pragma unroll
  for (int k = 0; k < LM_ROW; k += 2) {
    const double2 d = *reinterpret_cast<const double2*>(p + k);
    r[k] = d.x;
    r[k + 1] = d.y;
  }
}
__device__ __forceinline__ void reid_store_row(double* p, const double (&r)[LM_ROW]) {
#pragma unroll
  for (int k = 0; k < LM_ROW; k += 2) *reinterpret_cast<double2*>(p + k) = double2{r[k], r[k + 1]};
}

__global__ __launch_bounds__(REID_THREADS) void landmark_reid_kernel(ReidArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char reid_lds[];
  __shared__ int wsum[REID_WAVES];
  __shared__ double pose[19];  // Rm (row by row), t, c, (fx, fy, cx, cy)
  __shared__ ReidArgs sa;
  __shared__ int counters[3];  // matched, in-use entries overwritten, entries in use afterwards
  const int h = blockIdx.x, tid = threadIdx.x;
  const int N = a.N, C = a.C, T = a.T;
  double* e_px = reinterpret_cast<double*>(reid_lds);          // [C] projection of every entry on position 0
  double* e_py = e_px + C;                                     // [C]
  int* e_win = reinterpret_cast<int*>(e_py + C);               // [C] the slot an entry accepted, or -1
  int* s_pick = e_win + C;                                     // [N] the entry a born slot picked, or -1
  int* s_rank = s_pick + N;                                    // [N] rank among the retirable rows, or -1
  int* s_sid = s_rank + N;                                     // [N] the id a retirable row is archived under
  unsigned char* e_flag = reinterpret_cast<unsigned char*>(s_sid + N);  // [C] ENTRY_*

  const int sidx = a.stream_idx[h];
  // (the stream indices are checked on the host too: never touch memory outside the state)
  const bool inside = sidx >= 0 && ((long long)sidx + 1) * N <= a.rows && ((long long)sidx + 1) * C <= a.entries;
  COMET_DASSERT(inside);
  if (!inside) return;  // (the whole workgroup: no barrier is skipped by a part of it)
  const size_t row0 = (size_t)sidx * N, ent0 = (size_t)sidx * C, out0 = (size_t)h * N;
  const size_t px0 = (size_t)h * T * N;  // window position 0 of tracks

  // the pose of position 0, the camera centre c = -Rm^T t in the body frame and the intrinsics, kept in LDS
  // (every step reads the part it needs; held in scalar registers across the kernel they would not fit)
  if (tid == 0) {
    double m[3][3];
    lm_rotation(a.R + (size_t)h * T * 4, a.inverse != 0, m);
    const double* tp = a.Tx + (size_t)h * T * 3;
    const double t[3] = {tp[0], tp[1], tp[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      pose[k] = m[0][k]; pose[3 + k] = m[1][k]; pose[6 + k] = m[2][k];
      pose[9 + k] = t[k];
      pose[12 + k] = 0.0 - (m[0][k] * t[0] + m[1][k] * t[1] + m[2][k] * t[2]);
    }
    const double* in = a.intr + (size_t)h * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) pose[15 + k] = in[k];
  }
  if (tid < 3) counters[tid] = 0;
  // The arguments are read from LDS from here on: 19 pointers held in scalar registers across the five steps
  // and their barriers do not fit the scalar register file (the compiler then spills them); read where
  // they are used they are short-lived vector registers.
  if (tid == 0) sa = a;
  __syncthreads();

  // 1. every archive entry of the stream, projected once
  {
    const double m[3][3] = {{pose[0], pose[1], pose[2]}, {pose[3], pose[4], pose[5]}, {pose[6], pose[7], pose[8]}};
    const double t[3] = {pose[9], pose[10], pose[11]}, c[3] = {pose[12], pose[13], pose[14]};
    const double fx = pose[15], fy = pose[16], cx = pose[17], cy = pose[18];
  for (int e = tid; e < C; e += REID_THREADS) {
    unsigned char flag = 0;
    double ex = 0.0, ey = 0.0;
    if (sa.arch_id[ent0 + e] >= 0) {
      flag = ENTRY_IN_USE;
      const double* ap = sa.arch + (ent0 + e) * ARCH_ROW;
      const double2 x01 = *reinterpret_cast<const double2*>(ap + 12), x2d0 = *reinterpret_cast<const double2*>(ap + 14);
      const double2 d12 = *reinterpret_cast<const double2*>(ap + 16);
      const double X[3] = {x01.x, x01.y, x2d0.x};
      double xc[3], dn[3];
      reid_to_camera(m, t, X, xc);
      reid_view_dir(c, X, dn);
      const double cosv = x2d0.y * dn[0] + d12.x * dn[1] + d12.y * dn[2];
      ex = fx * (xc[0] / xc[2]) + cx;
      ey = fy * (xc[1] / xc[2]) + cy;
      if (xc[2] > 0.0 && cosv >= sa.min_cos && isfinite(ex) && isfinite(ey)) flag |= ENTRY_CANDIDATE;
    }
    e_px[e] = ex;
    e_py[e] = ey;
    e_win[e] = -1;
    e_flag[e] = flag;
  }
  }
  __syncthreads();

  // 2. every slot: is its row dying and retirable (its rank; the row goes to the workspace), and the pick
  //    of a born slot. Nothing of the state is written before every read of it is done (step 4 on).
  const double gate2 = sa.reid_px * sa.reid_px;
  int retired = 0;
  bool any_pick = false;
  for (int base = 0; base < N; base += REID_THREADS) {
    const int j = base + tid;
    const bool live = j < N;
    bool retirable = false;
    int id = -1, sr = 0, sid = -1;
    if (live) {
      id = sa.ids[out0 + j];
      sr = sa.src[out0 + j];
      const int aid = sa.acc_id[row0 + j];
      if (aid >= 0 && (id != aid || sr != j)) {  // dying: comet_landmark_update is about to overwrite or clear it
        double r[LM_ROW], X[3];
        reid_load_row(sa.acc + (row0 + j) * LM_ROW, r);
        if (lm_solve(r, sa.min_pivot, X) && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) &&
            r[10] >= (double)sa.arch_min_obs) {
          if (pose[6] * X[0] + pose[7] * X[1] + pose[8] * X[2] + pose[11] > 0.0) {  // in front at position 0
            retirable = true;
            reid_store_row(sa.ws + (out0 + j) * LM_ROW, r);
            const int al = sa.alias[row0 + j];
            sid = al >= 0 ? al : aid;
          }
        }
      }
    }
    int total;
    const int rank = retired + reid_scan(retirable, wsum, total);
    retired += total;
    if (live) {
      s_rank[j] = retirable ? rank : -1;
      s_sid[j] = sid;
      int pick = -1;
      if (id >= 0 && sr < 0) {  // born
        const float2 p = *reinterpret_cast<const float2*>(sa.tracks + (px0 + j) * 2);
        if (isfinite(p.x) && isfinite(p.y)) {
          double best = INFINITY;
          for (int e = 0; e < C; ++e) {
            if (!(e_flag[e] & ENTRY_CANDIDATE)) continue;
            const double d2 = reid_dist2(e_px[e], e_py[e], p);
            if (d2 <= gate2 && d2 < best) {  // (ties: the lower entry stays)
              best = d2;
              pick = e;
            }
          }
        }
      }
      s_pick[j] = pick;
      any_pick |= pick >= 0;
    }
  }

  // 3. every candidate entry accepts the nearest of the slots that picked it
  if (__syncthreads_or(any_pick)) {
    for (int e = tid; e < C; e += REID_THREADS) {
      if (!(e_flag[e] & ENTRY_CANDIDATE)) continue;
      const double ex = e_px[e], ey = e_py[e];
      double best = INFINITY;
      int win = -1;
      for (int j = 0; j < N; ++j) {
        if (s_pick[j] != e) continue;
        const double d2 = reid_dist2(ex, ey, *reinterpret_cast<const float2*>(sa.tracks + (px0 + j) * 2));
        if (d2 < best) {  // (ties: the lower slot stays; a pick's distance is finite)
          best = d2;
          win = j;
        }
      }
      e_win[e] = win;
    }
    __syncthreads();
  }

  // 4. matched slots take their entry's row; every slot's outputs. The archive is only read here (but for
  //    the ids of consumed entries, which nothing reads again before step 5's barrier).
  int matched = 0;
  for (int j = tid; j < N; j += REID_THREADS) {
    const int id = sa.ids[out0 + j], sr = sa.src[out0 + j];
    const int aid = sa.acc_id[row0 + j], al = sa.alias[row0 + j];
    const bool born = id >= 0 && sr < 0;
    const int pick = s_pick[j];
    const bool match = born && pick >= 0 && e_win[pick] == j;
    int st = 0, lm = id >= 0 ? id : -1, so = sr;
    float ds = INFINITY;
    if (match) {
      const size_t e = ent0 + pick;
      double r[LM_ROW];
      reid_load_row(sa.arch + e * ARCH_ROW, r);
      reid_store_row(sa.acc + (row0 + j) * LM_ROW, r);
      lm = sa.arch_id[e];
      sa.acc_id[row0 + j] = id;
      sa.alias[row0 + j] = lm;
      sa.arch_id[e] = -1;
      e_flag[pick] = 0;  // consumed: free for a retirement of this launch
      st = 1;
      so = j;
      ds = (float)sqrt(reid_dist2(e_px[pick], e_py[pick], *reinterpret_cast<const float2*>(sa.tracks + (px0 + j) * 2)));
      ++matched;
    } else {
      if (born) st = pick < 0 ? 2 : 3;
      if (id >= 0 && sr == j && aid == id) {  // carried: the alias stays
        if (al >= 0) lm = al;
      } else {
        sa.alias[row0 + j] = -1;
      }
    }
    sa.src_lm[out0 + j] = so;
    sa.lm_id[out0 + j] = lm;
    sa.state[out0 + j] = st;
    sa.dist[out0 + j] = ds;
  }
  if (matched) atomicAdd(&counters[0], matched);
  __syncthreads();

  // 5. retirements, in rank order from the cursor; of more than C the last C stay (what a loop in rank order
  //    leaves), so every entry is written by one thread
  int cursor = sa.arch_cursor[sidx];
  cursor = ((cursor % C) + C) % C;  // (a cursor from outside [0, C) is folded, not trusted)
  int over = 0;
  for (int j = tid; j < N; j += REID_THREADS) {
    const int rank = s_rank[j];
    if (rank < 0) continue;
    const int e = (cursor + rank) % C;
    if (rank < C && (e_flag[e] & ENTRY_IN_USE)) ++over;  // an entry in use before this launch and not consumed
    if (rank < retired - C) continue;
    const double c[3] = {pose[12], pose[13], pose[14]};
    double r[LM_ROW], X[3], d[3];
    reid_load_row(sa.ws + (out0 + j) * LM_ROW, r);
    lm_solve(r, sa.min_pivot, X);  // (as in step 2: solved, finite)
    reid_view_dir(c, X, d);
    double* ap = sa.arch + (ent0 + e) * ARCH_ROW;
    reid_store_row(ap, r);
    *reinterpret_cast<double2*>(ap + 12) = double2{X[0], X[1]};
    *reinterpret_cast<double2*>(ap + 14) = double2{X[2], d[0]};
    *reinterpret_cast<double2*>(ap + 16) = double2{d[1], d[2]};
    *reinterpret_cast<double2*>(ap + 18) = double2{0.0, 0.0};
    sa.arch_id[ent0 + e] = s_sid[j];
  }
  if (tid == 0 && retired > C) over += retired - C;  // retirements that landed on one of this launch
  if (over) atomicAdd(&counters[1], over);
  __syncthreads();

  int used = 0;
  for (int e = tid; e < C; e += REID_THREADS) used += sa.arch_id[ent0 + e] >= 0;
  if (used) atomicAdd(&counters[2], used);
  __syncthreads();
  if (tid == 0) {
    sa.arch_cursor[sidx] = (cursor + retired) % C;
    int* st = sa.stats + (size_t)h * 4;
    st[0] = retired;
    st[1] = counters[0];
    st[2] = counters[2];
    st[3] = counters[1];
  }
}

}  // namespace
}  // namespace comet

using namespace comet;

extern "C" int comet_landmark_reid(const float* tracks, const float* R, const double* T, const int32_t* ids,
                                   const int32_t* src, const int32_t* stream_idx, const int32_t* stream_idx_host,
                                   const double* intr, const double* intr_host, double* acc, int32_t* acc_id,
                                   int32_t* alias, int rows, double* arch, int32_t* arch_id, int32_t* arch_cursor,
                                   int entries, double* ws, int n, int Tw, int N, int C, int inverse_rotation,
                                   int arch_min_obs, double min_pivot, double reid_px, double reid_min_cos,
                                   int32_t* src_lm, int32_t* lm_id, int32_t* reid_state, float* reid_dist,
                                   int32_t* stats, void* stream) {
  COMET_CHECK_ARG(tracks && R && T && ids && src && stream_idx && stream_idx_host && intr && intr_host && acc &&
                      acc_id && alias && arch && arch_id && arch_cursor && ws && src_lm && lm_id && reid_state &&
                      reid_dist && stats,
                  "comet_landmark_reid: null pointer");
  COMET_CHECK_ARG(n >= 1, "comet_landmark_reid: n must be positive");
  COMET_CHECK_ARG(N >= 1 && N <= REID_MAX_N, "comet_landmark_reid: N outside [1, 4096]");
  COMET_CHECK_ARG(C >= 1 && C <= REID_MAX_C, "comet_landmark_reid: C outside [1, 4096]");
  COMET_CHECK_ARG(Tw >= 2, "comet_landmark_reid: T must be at least 2");
  COMET_CHECK_ARG((int64_t)rows >= (int64_t)n * N, "comet_landmark_reid: rows below n * N");
  COMET_CHECK_ARG((int64_t)entries >= (int64_t)n * C, "comet_landmark_reid: entries below n * C");
  const int streams = rows / N < entries / C ? rows / N : entries / C;
  for (int h = 0; h < n; ++h) {  // two hops on one stream's state would race (n is a handful: compared pairwise)
    COMET_CHECK_ARG(stream_idx_host[h] >= 0 && stream_idx_host[h] < streams,
                    "comet_landmark_reid: stream index outside the state");
    for (int g = 0; g < h; ++g)
      COMET_CHECK_ARG(stream_idx_host[g] != stream_idx_host[h], "comet_landmark_reid: duplicate stream index");
  }
  for (int h = 0; h < n; ++h)
    COMET_CHECK_ARG(std::isfinite(intr_host[4 * h]) && intr_host[4 * h] > 0.0 && std::isfinite(intr_host[4 * h + 1]) &&
                        intr_host[4 * h + 1] > 0.0,
                    "comet_landmark_reid: fx and fy must be finite and positive");
  COMET_CHECK_ARG(inverse_rotation == 0 || inverse_rotation == 1, "comet_landmark_reid: inverse_rotation must be 0 or 1");
  COMET_CHECK_ARG(arch_min_obs >= 2, "comet_landmark_reid: arch_min_obs must be at least 2");
  COMET_CHECK_ARG(min_pivot >= 0.0 && min_pivot < 1.0, "comet_landmark_reid: min_pivot outside [0, 1)");
  COMET_CHECK_ARG(std::isfinite(reid_px) && reid_px > 0.0, "comet_landmark_reid: reid_px must be finite and positive");
  COMET_CHECK_ARG(reid_min_cos >= -1.0 && reid_min_cos <= 1.0, "comet_landmark_reid: reid_min_cos outside [-1, 1]");
  COMET_CHECK_ARG((((uintptr_t)tracks | (uintptr_t)T | (uintptr_t)intr) & 7) == 0 &&
                      (((uintptr_t)R | (uintptr_t)acc | (uintptr_t)arch | (uintptr_t)ws) & 15) == 0,
                  "comet_landmark_reid: tracks, T and intr must be 8-B aligned, R, acc, arch and ws 16-B aligned");
  ReidArgs a{};
  a.tracks = tracks; a.R = R; a.Tx = T; a.ids = ids; a.src = src; a.stream_idx = stream_idx; a.intr = intr;
  a.acc = acc; a.acc_id = acc_id; a.alias = alias; a.arch = arch; a.arch_id = arch_id; a.arch_cursor = arch_cursor;
  a.ws = ws; a.src_lm = src_lm; a.lm_id = lm_id; a.state = reid_state; a.dist = reid_dist; a.stats = stats;
  a.T = Tw; a.N = N; a.C = C; a.rows = rows; a.entries = entries; a.inverse = inverse_rotation;
  a.arch_min_obs = arch_min_obs; a.min_pivot = min_pivot; a.reid_px = reid_px; a.min_cos = reid_min_cos;
  // a workgroup of gfx950 may hold up to 160 KiB; above 64 KiB the kernel has to be told, on every device
  // it runs on (set on each launch: the call is cheap next to a launch and knows nothing of the caller's device)
  const hipError_t attr = hipFuncSetAttribute((const void*)landmark_reid_kernel,
                                              hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)reid_lds_bytes(REID_MAX_N, REID_MAX_C));
  if (attr != hipSuccess) {
    set_error(std::string("comet_landmark_reid: the LDS attribute could not be set: ") + hipGetErrorString(attr));
    return COMET_ELAUNCH;
  }
  hipLaunchKernelGGL(landmark_reid_kernel, dim3((unsigned)n), dim3(REID_THREADS), reid_lds_bytes(N, C),
                     as_stream(stream), a);
  COMET_CHECK_LAUNCH("comet_landmark_reid");
  return COMET_OK;
}
