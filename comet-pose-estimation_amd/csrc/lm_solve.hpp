// The accumulator solve of the landmark map (include/comet_hip.h: the row layout of comet_landmark_update),
// shared by the two kernels that solve a row: landmark_update_kernel (landmark.hip) and landmark_reid_kernel
// (reid.hip), which must solve it the same way. Plain IEEE double evaluated as written (no contraction into
// fma), only + - * /, so that tests/landmark_numpy.py rotation / solve restate it operation by operation.
#pragma once
#include "common.hpp"

namespace comet {

constexpr int LM_ROW = COMET_LM_ROW;  // doubles per accumulator row

// rows r1, r2, r3 of the matrix of q (minipytorch3d.quaternion_to_matrix), or of its transpose
__device__ __forceinline__ void lm_rotation(const float* q, bool inverse, double (&m)[3][3]) {
#pragma clang fp contract(off)
  const float4 qf = *reinterpret_cast<const float4*>(q);
  const double r = qf.x, i = qf.y, j = qf.z, k = qf.w;
  const double two_s = 2.0 / (r * r + i * i + j * j + k * k);
  const double m00 = 1.0 - two_s * (j * j + k * k), m01 = two_s * (i * j - k * r), m02 = two_s * (i * k + j * r);
  const double m10 = two_s * (i * j + k * r), m11 = 1.0 - two_s * (i * i + k * k), m12 = two_s * (j * k - i * r);
  const double m20 = two_s * (i * k - j * r), m21 = two_s * (j * k + i * r), m22 = 1.0 - two_s * (i * i + j * j);
  m[0][0] = m00; m[1][1] = m11; m[2][2] = m22;
  m[0][1] = inverse ? m10 : m01; m[1][0] = inverse ? m01 : m10;
  m[0][2] = inverse ? m20 : m02; m[2][0] = inverse ? m02 : m20;
  m[1][2] = inverse ? m21 : m12; m[2][1] = inverse ? m12 : m21;
}

// M X = g of the row r by an unpivoted LDL^T -> false when a pivot is at or below min_pivot * max(diag M)
// (ill-conditioned; x is then not written), else true with x = X (which may still be non-finite)
__device__ __forceinline__ bool lm_solve(const double (&r)[LM_ROW], double min_pivot, double (&x)[3]) {
#pragma clang fp contract(off)
  const double thr = min_pivot * fmax(fmax(r[0], r[3]), r[5]);
  const double d0 = r[0];
  const double l10 = r[1] / d0, l20 = r[2] / d0;
  const double d1 = r[3] - l10 * r[1];
  const double u12 = r[4] - l20 * r[1];
  const double l21 = u12 / d1;
  const double d2 = r[5] - l20 * r[2] - l21 * u12;
  if (d0 <= thr || d1 <= thr || d2 <= thr) return false;
  const double y0 = r[6];
  const double y1 = r[7] - l10 * y0;
  const double y2 = r[8] - l20 * y0 - l21 * y1;
  const double x2 = y2 / d2;
  const double x1 = y1 / d1 - l21 * x2;
  const double x0 = y0 / d0 - l10 * x1 - l20 * x2;
  x[0] = x0; x[1] = x1; x[2] = x2;
  return true;
}

}  // namespace comet
