// Frame ring of the online path (comet_amd/stream.py, DESIGN.md "Online / streaming inference"):
// the per-frame tensors of the last `capacity` frames live in device rings; a hop needs the T
// slots of its window contiguous. comet_ring_gather copies them for up to 4 rings in one launch.
// comet_ring_scatter is its inverse: the k new frames of a push (StreamPool: one per stream) go
// from contiguous rows into their ring slots, for up to 4 rings in one launch.
#include <vector>

#include "common.hpp"

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
