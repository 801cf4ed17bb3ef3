// Track carry of the online path (comet_amd/stream.py TrackCarry, DESIGN.md "Track carry"): the query
// points of a new window are the previous window's refined tracks on the frame that is now first,
// kept in their slots with their ids; free slots take detector candidates, the rest is padded.
// comet_track_carry serves all n hops of a push in one launch, one workgroup per hop. The contract
// (rules 1-5) is in include/comet_hip.h; tests/carry_numpy.py restates it with sequential loops.
#include <climits>
#include <cmath>

#include "common.hpp"

namespace comet {
namespace {

constexpr int CARRY_THREADS = 256;
constexpr int CARRY_WAVES = CARRY_THREADS / 64;
constexpr int CARRY_MAX_N = COMET_CARRY_MAX_TRACKS;
constexpr int CARRY_MAX_M = COMET_CARRY_MAX_CANDIDATES;
constexpr int CARRY_MAX_CELLS = COMET_CARRY_MAX_CELLS;
constexpr unsigned CARRY_AGE_MAX = (1u << 19) - 1;
constexpr unsigned CARRY_EMPTY = 0xffffffffu;
constexpr unsigned CARRY_CAND = 0x80000000u;

// the lattice pads are plain f32 evaluated as written (tests/carry_numpy.py uses the same expression)
#pragma clang fp contract(off)

struct CarryArgs {  // by value in the kernel arguments
  const float* tracks;      // [n, T, N, 2]
  const float* score;       // [n, T, N]
  const int* ids;           // [n, N]
  const int* age;           // [n, N]
  const unsigned char* mask;  // [n, H, W] or NULL
  const float* cand;        // [n, M, 2] or NULL (M == 0)
  const int* cand_n;        // [n]
  int* next_id;             // [n]
  const int* prev_valid;    // [n]
  float* query;             // [n, N, 2]
  int* ids_out;             // [n, N]
  int* age_out;             // [n, N]
  int* src;                 // [n, N]
  int* stats;               // [n, 4]
  int T, N, M, s, H, W, cell, border, gw, gh, lattice;
  float min_score;
};

// Rule 1 for a position; cell_out: the grid cell (row-major), valid when the point is alive.
__device__ __forceinline__ bool carry_alive(const CarryArgs& a, const unsigned char* mask, float x, float y,
                                            int& cell_out) {
  cell_out = 0;
  if (!(isfinite(x) && isfinite(y))) return false;
  if (!(x >= (float)a.border && x <= (float)(a.W - 1 - a.border))) return false;
  if (!(y >= (float)a.border && y <= (float)(a.H - 1 - a.border))) return false;
  if (mask) {  // round half to even, then clamp: the indexing of filter_and_pad
    const int ix = min(max((int)rintf(x), 0), a.W - 1), iy = min(max((int)rintf(y), 0), a.H - 1);
    if (mask[(size_t)iy * a.W + ix] == 0) return false;
  }
  const int cx = (int)floorf(x / (float)a.cell), cy = (int)floorf(y / (float)a.cell);
  COMET_DASSERT(cx >= 0 && cx < a.gw && cy >= 0 && cy < a.gh);
  if ((unsigned)cx >= (unsigned)a.gw || (unsigned)cy >= (unsigned)a.gh) return false;  // (never: 0 <= x <= W - 1)
  cell_out = cy * a.gw + cx;
  return true;
}

__device__ __forceinline__ unsigned carry_track_key(int age, int j) {
  const unsigned ag = (unsigned)min(max(age, 0), (int)CARRY_AGE_MAX);
  return ((CARRY_AGE_MAX - ag) << 12) | (unsigned)j;
}

// Exclusive prefix sum of a 0 / 1 flag over the workgroup (thread order) and the workgroup's total.
// Every thread of the workgroup must call it (two barriers).
__device__ __forceinline__ int carry_scan(bool flag, int* wsum, int& total) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int off = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < CARRY_WAVES; ++i) {
    const int v = wsum[i];
    off += i < w ? v : 0;
    total += v;
  }
  __syncthreads();
  return off + pre;
}

enum : unsigned char { SLOT_FREE = 0, SLOT_KEPT = 1, SLOT_BORN = 2 };

// One workgroup per hop. Slot j is always handled by thread j % 256, and every pass reads ids / age
// of a slot before it writes ids_out / age_out of that slot, so ids_out == ids and age_out == age
// (in place) is allowed.
__global__ __launch_bounds__(CARRY_THREADS) void track_carry_kernel(CarryArgs a) {
  __shared__ unsigned keys[CARRY_MAX_CELLS];  // 32 KiB: the minimum key of every cell
  __shared__ int list[CARRY_MAX_N];           // 16 KiB: kept candidates by rank, then live slots by rank
  __shared__ unsigned char state[CARRY_MAX_N];  // 4 KiB
  __shared__ int wsum[CARRY_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = a.N, ncells = a.gw * a.gh;
  const bool prev = a.prev_valid[b] != 0;
  const int cn = a.cand ? min(max(a.cand_n[b], 0), a.M) : 0;
  const int id0 = a.next_id[b];
  const float* tr = a.tracks + (((size_t)b * a.T + a.s) * N) * 2;
  const float* sc = a.score + ((size_t)b * a.T + a.s) * N;
  const int* ids = a.ids + (size_t)b * N;
  const int* age = a.age + (size_t)b * N;
  const unsigned char* mask = a.mask ? a.mask + (size_t)b * a.H * a.W : nullptr;
  const float* cand = a.cand ? a.cand + (size_t)b * a.M * 2 : nullptr;
  float* query = a.query + (size_t)b * N * 2;
  int* ids_out = a.ids_out + (size_t)b * N;
  int* age_out = a.age_out + (size_t)b * N;
  int* src = a.src + (size_t)b * N;

  for (int i = tid; i < ncells; i += CARRY_THREADS) keys[i] = CARRY_EMPTY;
  __syncthreads();

  // 1. every alive point posts its key
  if (prev) {
    for (int j = tid; j < N; j += CARRY_THREADS) {
      int cell;
      const float2 p = *reinterpret_cast<const float2*>(tr + 2 * (size_t)j);
      if (ids[j] >= 0 && sc[j] >= a.min_score && carry_alive(a, mask, p.x, p.y, cell))
        atomicMin(&keys[cell], carry_track_key(age[j], j));
    }
  }
  for (int c = tid; c < cn; c += CARRY_THREADS) {
    int cell;
    const float2 p = *reinterpret_cast<const float2*>(cand + 2 * (size_t)c);
    if (carry_alive(a, mask, p.x, p.y, cell)) atomicMin(&keys[cell], CARRY_CAND | (unsigned)c);
  }
  __syncthreads();

  // 2. tracks that hold their cell's minimum stay in their slot
  int survivors = 0, dropped = 0;  // (per thread; summed below)
  for (int j = tid; j < N; j += CARRY_THREADS) {
    bool kept = false;
    if (prev) {
      int cell;
      const float2 p = *reinterpret_cast<const float2*>(tr + 2 * (size_t)j);
      const int id = ids[j], ag = age[j];
      if (id >= 0 && sc[j] >= a.min_score && carry_alive(a, mask, p.x, p.y, cell)) {
        kept = keys[cell] == carry_track_key(ag, j);
        if (kept) {
          *reinterpret_cast<float2*>(query + 2 * (size_t)j) = p;
          ids_out[j] = id;
          age_out[j] = ag < INT_MAX ? max(ag, 0) + 1 : INT_MAX;
          src[j] = j;
          ++survivors;
        } else {
          ++dropped;
        }
      }
    }
    state[j] = kept ? SLOT_KEPT : SLOT_FREE;
  }
  __syncthreads();

  // 3. kept candidates in ascending c -> list[rank] (the first N of them: there are at most N free slots)
  int n_cand = 0;
  for (int base = 0; base < cn; base += CARRY_THREADS) {
    const int c = base + tid;
    bool kept = false;
    if (c < cn) {
      int cell;
      const float2 p = *reinterpret_cast<const float2*>(cand + 2 * (size_t)c);
      kept = carry_alive(a, mask, p.x, p.y, cell) && keys[cell] == (CARRY_CAND | (unsigned)c);
    }
    int total;
    const int r = n_cand + carry_scan(kept, wsum, total);
    if (kept && r < N) list[r] = c;
    n_cand += total;
  }
  __syncthreads();

  // 4. free slots in ascending j: the r-th takes the r-th kept candidate
  int n_free = 0;
  for (int base = 0; base < N; base += CARRY_THREADS) {
    const int j = base + tid;
    const bool free_slot = j < N && state[j] == SLOT_FREE;
    int total;
    const int r = n_free + carry_scan(free_slot, wsum, total);
    if (free_slot && r < n_cand) {  // (r < N always, so list[r] was written)
      const int c = list[r];
      COMET_DASSERT(c >= 0 && c < cn);
      if ((unsigned)c < (unsigned)cn) {
        *reinterpret_cast<float2*>(query + 2 * (size_t)j) = *reinterpret_cast<const float2*>(cand + 2 * (size_t)c);
        ids_out[j] = id0 + r;
        age_out[j] = 0;
        src[j] = -1 - c;
        state[j] = SLOT_BORN;
      }
    }
    n_free += total;
  }
  const int born = min(n_cand, n_free);
  __syncthreads();  // (every read of list as candidates is done; the barrier also publishes query)

  // 5. live slots in ascending j -> list[rank]
  int n_live = 0;
  for (int base = 0; base < N; base += CARRY_THREADS) {
    const int j = base + tid;
    const bool live = j < N && state[j] != SLOT_FREE;
    int total;
    const int r = n_live + carry_scan(live, wsum, total);
    if (live) list[r] = j;
    n_live += total;
  }
  __syncthreads();

  // 6. pads: the r-th slot still free copies live slot r mod L, or is a lattice point when L == 0
  int n_pad = 0;
  for (int base = 0; base < N; base += CARRY_THREADS) {
    const int j = base + tid;
    const bool pad = j < N && state[j] == SLOT_FREE;
    int total;
    const int r = n_pad + carry_scan(pad, wsum, total);
    if (pad) {
      float2 p;
      int from = INT_MIN;
      if (n_live > 0) {
        const int k = list[r % n_live];
        COMET_DASSERT(k >= 0 && k < N);
        p = (unsigned)k < (unsigned)N ? *reinterpret_cast<const float2*>(query + 2 * (size_t)k) : float2{0.f, 0.f};
        from = INT_MIN + k;
      } else {
        const int g = a.lattice;
        p.x = ((float)(r % g) + 0.5f) * (float)a.W / (float)g;
        p.y = ((float)(r / g) + 0.5f) * (float)a.H / (float)g;
      }
      *reinterpret_cast<float2*>(query + 2 * (size_t)j) = p;
      ids_out[j] = -1;
      age_out[j] = 0;
      src[j] = from;
    }
    n_pad += total;
  }

  // statistics: per-thread counts summed over the workgroup through LDS (keys is free again)
  __syncthreads();
  int* red = reinterpret_cast<int*>(keys);
  red[tid] = survivors;
  red[CARRY_THREADS + tid] = dropped;
  __syncthreads();
  if (tid == 0) {
    int sv = 0, dr = 0;
    for (int i = 0; i < CARRY_THREADS; ++i) {
      sv += red[i];
      dr += red[CARRY_THREADS + i];
    }
    int* st = a.stats + (size_t)b * 4;
    st[0] = sv;
    st[1] = born;
    st[2] = n_pad;
    st[3] = dr;
    a.next_id[b] = id0 + born;
  }
}

int isqrt_ceil(int n) {
  int g = 1;
  while ((int64_t)g * g < n) ++g;
  return g;
}

}  // namespace
}  // namespace comet

using namespace comet;

extern "C" int comet_track_carry(const float* tracks, const float* score, const int32_t* ids, const int32_t* age,
                                 const uint8_t* mask, const float* cand, const int32_t* cand_n, int32_t* next_id,
                                 const int32_t* prev_valid, int n, int T, int N, int M, int s, int H, int W, int cell,
                                 int border, float min_score, float* query, int32_t* ids_out, int32_t* age_out,
                                 int32_t* src, int32_t* stats, void* stream) {
  COMET_CHECK_ARG(tracks && score && ids && age && cand_n && next_id && prev_valid && query && ids_out && age_out &&
                      src && stats,
                  "comet_track_carry: null pointer");
  COMET_CHECK_ARG(n >= 1, "comet_track_carry: n must be positive");
  COMET_CHECK_ARG(N >= 1 && N <= CARRY_MAX_N, "comet_track_carry: N outside [1, 4096]");
  COMET_CHECK_ARG(M >= 0 && M <= CARRY_MAX_M, "comet_track_carry: M outside [0, 65536]");
  COMET_CHECK_ARG(cand || M == 0, "comet_track_carry: cand may be null only when M is 0");
  COMET_CHECK_ARG(s >= 1 && s <= T - 1, "comet_track_carry: s outside [1, T - 1]");
  COMET_CHECK_ARG(H >= 1 && W >= 1, "comet_track_carry: H and W must be positive");
  COMET_CHECK_ARG(cell >= 1, "comet_track_carry: cell must be at least 1");
  COMET_CHECK_ARG(border >= 0, "comet_track_carry: negative border");
  const int64_t gw = cdiv(W, cell), gh = cdiv(H, cell);
  COMET_CHECK_ARG(gw * gh <= CARRY_MAX_CELLS, "comet_track_carry: more than 8192 grid cells");
  COMET_CHECK_ARG((((uintptr_t)tracks | (uintptr_t)cand | (uintptr_t)query) & 7) == 0,
                  "comet_track_carry: tracks, cand and query must be 8-B aligned");
  CarryArgs a{};
  a.tracks = tracks; a.score = score; a.ids = ids; a.age = age; a.mask = mask; a.cand = cand; a.cand_n = cand_n;
  a.next_id = next_id; a.prev_valid = prev_valid;
  a.query = query; a.ids_out = ids_out; a.age_out = age_out; a.src = src; a.stats = stats;
  a.T = T; a.N = N; a.M = M; a.s = s; a.H = H; a.W = W; a.cell = cell; a.border = border;
  a.gw = (int)gw; a.gh = (int)gh;
  a.lattice = isqrt_ceil(N);
  a.min_score = min_score;
  hipLaunchKernelGGL(track_carry_kernel, dim3((unsigned)n), dim3(CARRY_THREADS), 0, as_stream(stream), a);
  COMET_CHECK_LAUNCH("comet_track_carry");
  return COMET_OK;
}
