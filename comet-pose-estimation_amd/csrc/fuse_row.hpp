// One accumulator row of comet_pose_fuse (include/comet_hip.h: the row layout), shared by the two
// kernels that add a hypothesis to it: pose_fuse_kernel (stream.hip) and landmark_pnp_kernel (pnp.hip),
// which must add it the same way. Plain IEEE double evaluated as written (no contraction into fma), so
// that tests/fuse_numpy.py add_hypothesis restates it operation by operation.
#pragma once
#include "common.hpp"

namespace comet {

constexpr int FUSE_ROW = COMET_FUSE_ROW;  // doubles per accumulator row

__device__ __forceinline__ void load_row(const double* p, double (&r)[FUSE_ROW]) {
#pragma unroll
  for (int k = 0; k < FUSE_ROW; k += 2) {
    const double2 d = *reinterpret_cast<const double2*>(p + k);
    r[k] = d.x;
    r[k + 1] = d.y;
  }
}
__device__ __forceinline__ void store_row(double* p, const double (&r)[FUSE_ROW]) {
#pragma unroll
  for (int k = 0; k < FUSE_ROW; k += 2) *reinterpret_cast<double2*>(p + k) = double2{r[k], r[k + 1]};
}

// row += one hypothesis (unit q, (u, v, z)) of weight w
__device__ __forceinline__ void add_hypothesis(double (&r)[FUSE_ROW], double w, const double (&q)[4],
                                               const double (&x)[3]) {
#pragma clang fp contract(off)
  double h[FUSE_ROW];
  h[0] = w;
  int k = 1;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) h[k++] = w * (q[i] * q[j]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    h[11 + i] = w * x[i];
    h[14 + i] = w * (x[i] * x[i]);
  }
  h[17] = 1.0;
  h[18] = h[19] = 0.0;
#pragma unroll
  for (int i = 0; i < FUSE_ROW; ++i) r[i] += h[i];
}

}  // namespace comet
