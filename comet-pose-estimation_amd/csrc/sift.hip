// SIFT keypoint detector (difference-of-Gaussians) for the track initialisation (SURVEY §8(f1),
// train_eval_func_new_cp5.py:527-531, 558-570): the reference seeds its tracker with
// LightGlue's SIFT, a wrapper around OpenCV's CPU detector. This is that algorithm on the GPU --
// the 2x base image, the Gaussian scale space, DoG extrema with sub-pixel refinement, the contrast
// and edge tests, and the number of orientation peaks per keypoint (OpenCV emits one keypoint per
// peak and those duplicates take part in its keep-best-n cut; the angles themselves are unused).
// No descriptors: COMET reads only the coordinates.
#include "common.hpp"

#include <cmath>

namespace comet {
namespace {

// ---- separable Gaussian blur, fused: raw tile (+halo) -> LDS, row pass LDS -> LDS, column pass out
constexpr int GB_TW = 64, GB_TH = 32, GB_RMAX = 10;
struct GaussTaps {
  float w[2 * GB_RMAX + 1];
};

// BORDER_REFLECT_101 for any p (images narrower than the kernel radius reflect more than once)
__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  p %= period;
  if (p < 0) p += period;
  return p < n ? p : period - p;
}

// UP: the source is a uint8 image [B, H/2, W/2] and the blurred image is its 2x bilinear up-sample
// (INTER_LINEAR pixel centres, src = (dst + 0.5) / 2 - 0.5, edge-clamped: the weights are 0.25 / 0.75,
// exact in f32). Otherwise the source is f32 [B, H, W]. Taps are summed in ascending order.
// Lanes run along x in every pass, so the LDS reads and writes of a wave are consecutive words.
template <bool UP>
__global__ __launch_bounds__(256) void gauss_blur_kernel(const void* __restrict__ x_, float* __restrict__ y, int H, int W,
                                                         int r, GaussTaps taps) {
  __shared__ float raw[(GB_TH + 2 * GB_RMAX) * (GB_TW + 2 * GB_RMAX)];
  __shared__ float rowb[(GB_TH + 2 * GB_RMAX) * GB_TW];
  const int b = blockIdx.z, x0 = blockIdx.x * GB_TW, y0 = blockIdx.y * GB_TH;
  const int tw = min(GB_TW, W - x0), th = min(GB_TH, H - y0);
  const int RW = tw + 2 * r, RH = th + 2 * r;
  for (int i = threadIdx.x; i < RH * RW; i += 256) {
    const int ry = i / RW, rx = i - ry * RW;
    const int gy = reflect101(y0 - r + ry, H), gx = reflect101(x0 - r + rx, W);
    float v;
    if constexpr (UP) {
      const int sh = H >> 1, sw = W >> 1;
      const unsigned char* p = (const unsigned char*)x_ + (int64_t)b * sh * sw;
      const float fy = gy * 0.5f - 0.25f, fx = gx * 0.5f - 0.25f;
      const int iy = (int)floorf(fy), ix = (int)floorf(fx);
      const float ly = fy - iy, lx = fx - ix;
      const int ya = max(iy, 0), yb = min(iy + 1, sh - 1), xa = max(ix, 0), xb = min(ix + 1, sw - 1);
      const float top = (1.f - lx) * p[ya * sw + xa] + lx * p[ya * sw + xb];
      const float bot = (1.f - lx) * p[yb * sw + xa] + lx * p[yb * sw + xb];
      v = (1.f - ly) * top + ly * bot;
    } else {
      v = ((const float*)x_)[((int64_t)b * H + gy) * W + gx];
    }
    raw[i] = v;
  }
  __syncthreads();
  const int nt = 2 * r + 1;
  for (int i = threadIdx.x; i < RH * tw; i += 256) {
    const int ry = i / tw, ox = i - ry * tw;
    const float* p = raw + ry * RW + ox;
    float acc = 0.f;
    for (int k = 0; k < nt; ++k) acc += taps.w[k] * p[k];
    rowb[i] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < th * tw; i += 256) {
    const int oy = i / tw, ox = i - oy * tw;
    const float* p = rowb + oy * tw + ox;
    float acc = 0.f;
    for (int k = 0; k < nt; ++k) acc += taps.w[k] * p[k * tw];
    y[((int64_t)b * H + y0 + oy) * W + x0 + ox] = acc;
  }
}

// OpenCV's automatic kernel size for float images: ksize = round(8 sigma + 1) | 1; taps in double
bool make_taps(double sigma, GaussTaps& t, int& r) {
  if (!(sigma > 0.0) || !(sigma < 1e3)) return false;
  const int ks = ((int)std::lrint(sigma * 8.0 + 1.0)) | 1;
  r = ks / 2;
  if (r > GB_RMAX) return false;
  double w[2 * GB_RMAX + 1], s = 0.0;
  for (int i = 0; i < ks; ++i) {
    const double d = i - r;
    w[i] = std::exp(-d * d / (2.0 * sigma * sigma));
    s += w[i];
  }
  for (int i = 0; i < 2 * GB_RMAX + 1; ++i) t.w[i] = i < ks ? (float)(w[i] / s) : 0.f;
  return true;
}

__global__ void downsample2_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W) {
  const int oh = H >> 1, ow = W >> 1;
  const int64_t total = (int64_t)B * oh * ow;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int ox = (int)(t % ow);
    const int64_t q = t / ow;
    const int oy = (int)(q % oh);
    const int64_t b = q / oh;
    y[t] = x[(b * H + 2 * oy) * W + 2 * ox];
  }
}

// ---- DoG extrema of one octave -------------------------------------------------------------
constexpr int DT_W = 32, DT_H = 8, SIFT_BORDER = 5, SIFT_STEPS = 5, SIFT_BINS = 36;

// x = -H^-1 g by Gaussian elimination with partial pivoting; false when H is singular
__device__ __forceinline__ bool solve3(float (&A)[3][4]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int p = c;
    float best = fabsf(A[c][c]);
#pragma unroll
    for (int q = c + 1; q < 3; ++q)
      if (fabsf(A[q][c]) > best) {
        best = fabsf(A[q][c]);
        p = q;
      }
    if (best == 0.f) return false;
#pragma unroll
    for (int q = c + 1; q < 3; ++q)
      if (p == q) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float t = A[c][k];
          A[c][k] = A[q][k];
          A[q][k] = t;
        }
      }
#pragma unroll
    for (int q = c + 1; q < 3; ++q) {
      const float f = A[q][c] / A[c][c];
#pragma unroll
      for (int k = c + 1; k < 4; ++k) A[q][k] -= f * A[c][k];
    }
  }
  A[2][3] = A[2][3] / A[2][2];
  A[1][3] = (A[1][3] - A[1][2] * A[2][3]) / A[1][1];
  A[0][3] = (A[0][3] - A[0][1] * A[1][3] - A[0][2] * A[2][3]) / A[0][0];
  return true;
}

// g: the nl + 3 Gaussian images of one octave [B, L, h, w]. One block = a 32 x 8 tile of interior
// pixels of one DoG layer s in 1..nl of one image; the three DoG tiles (+1 halo) are formed from the
// four Gaussian layers once, in LDS. Extrema are rare: the refinement reads the Gaussians directly.
// The orientation histogram of every keypoint a wave found is built by the whole wave: lane-private
// LDS columns (no atomics, a fixed summation order), one wave reduction per bin.
__global__ __launch_bounds__(256) void sift_detect_kernel(const float* __restrict__ g, int L, int h, int w, int octave,
                                                          int nl, float thr, float contrast_thr, float edge_thr,
                                                          float sigma, float* __restrict__ cand, int cap,
                                                          int* __restrict__ count, int* __restrict__ overflow) {
  __shared__ float dog[3][DT_H + 2][DT_W + 2];
  __shared__ float hist[4][SIFT_BINS * 64];
  const int b = blockIdx.z / nl, s = blockIdx.z % nl + 1;
  const int x0 = SIFT_BORDER + blockIdx.x * DT_W, y0 = SIFT_BORDER + blockIdx.y * DT_H;
  const int64_t plane = (int64_t)h * w;
  const float* gb = g + (int64_t)b * L * plane;
  for (int i = threadIdx.x; i < 3 * (DT_H + 2) * (DT_W + 2); i += 256) {
    const int k = i / ((DT_H + 2) * (DT_W + 2)), rem = i - k * ((DT_H + 2) * (DT_W + 2));
    const int yy = rem / (DT_W + 2), xx = rem - yy * (DT_W + 2);
    const int gy = y0 - 1 + yy, gx = x0 - 1 + xx;
    float v = 0.f;
    if (gy < h && gx < w) {
      const float* p = gb + (s - 1 + k) * plane + (int64_t)gy * w + gx;
      v = p[plane] - p[0];
    }
    dog[k][yy][xx] = v;
  }
  __syncthreads();
  const int tx = threadIdx.x & (DT_W - 1), ty = threadIdx.x / DT_W;
  const int lane = threadIdx.x & 63;
  int c = x0 + tx, r = y0 + ty, layer = s;
  bool found = false;
  if (c < w - SIFT_BORDER && r < h - SIFT_BORDER) {
    const float v = dog[1][ty + 1][tx + 1];
    if (fabsf(v) > thr) {
      bool is_max = v > 0.f, is_min = v < 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const float n = dog[k][ty + dy][tx + dx];
            is_max = is_max && v >= n;
            is_min = is_min && v <= n;
          }
      found = is_max || is_min;
    }
  }
  float kx = 0.f, ky = 0.f, ksize = 0.f, kresp = 0.f, kscl = 0.f;
  if (found) {
    found = false;
    const float ds = 0.5f / 255.f, d2s = 1.f / 255.f, dcs = 0.25f / 255.f;
    auto D = [&](int l, int rr, int cc) {
      const float* p = gb + l * plane + (int64_t)rr * w + cc;
      return p[plane] - p[0];
    };
    float xc = 0.f, xr = 0.f, xi = 0.f;
    for (int it = 0; it < SIFT_STEPS; ++it) {
      const float v2 = 2.f * D(layer, r, c);
      const float cxp = D(layer, r, c + 1), cxm = D(layer, r, c - 1), cyp = D(layer, r + 1, c), cym = D(layer, r - 1, c);
      const float np_ = D(layer + 1, r, c), pp_ = D(layer - 1, r, c);
      const float gx = (cxp - cxm) * ds, gy = (cyp - cym) * ds, gs = (np_ - pp_) * ds;
      const float dxx = (cxp + cxm - v2) * d2s, dyy = (cyp + cym - v2) * d2s, dss = (np_ + pp_ - v2) * d2s;
      const float dxy = (D(layer, r + 1, c + 1) - D(layer, r + 1, c - 1) - D(layer, r - 1, c + 1) + D(layer, r - 1, c - 1)) * dcs;
      const float dxs = (D(layer + 1, r, c + 1) - D(layer + 1, r, c - 1) - D(layer - 1, r, c + 1) + D(layer - 1, r, c - 1)) * dcs;
      const float dys = (D(layer + 1, r + 1, c) - D(layer + 1, r - 1, c) - D(layer - 1, r + 1, c) + D(layer - 1, r - 1, c)) * dcs;
      float A[3][4] = {{dxx, dxy, dxs, -gx}, {dxy, dyy, dys, -gy}, {dxs, dys, dss, -gs}};
      if (!solve3(A)) break;
      xc = A[0][3];
      xr = A[1][3];
      xi = A[2][3];
      if (fabsf(xc) < 0.5f && fabsf(xr) < 0.5f && fabsf(xi) < 0.5f) {
        const float contr = 0.5f * v2 * d2s + 0.5f * (gx * xc + gy * xr + gs * xi);
        const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
        if (fabsf(contr) * nl >= contrast_thr && det > 0.f &&
            tr * tr * edge_thr < (edge_thr + 1.f) * (edge_thr + 1.f) * det) {
          const float oscale = (float)(1 << octave);
          kscl = sigma * exp2f((layer + xi) / nl);
          kx = (c + xc) * oscale;
          ky = (r + xr) * oscale;
          ksize = kscl * oscale * 2.f;
          kresp = fabsf(contr);
          found = true;
        }
        break;
      }
      if (!(fabsf(xc) < 1e6f && fabsf(xr) < 1e6f && fabsf(xi) < 1e6f)) break;
      c += (int)rintf(xc);
      r += (int)rintf(xr);
      layer += (int)rintf(xi);
      if (layer < 1 || layer > nl || c < SIFT_BORDER || c >= w - SIFT_BORDER || r < SIFT_BORDER || r >= h - SIFT_BORDER)
        break;
    }
  }
  // orientation peaks: every lane of the wave stays here (wave-uniform loop over the found keypoints)
  float* hw = hist[threadIdx.x >> 6];
  int nori = 0;
  unsigned long long todo = __ballot(found);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int pc = __shfl(c, src, 64), pr = __shfl(r, src, 64), pl = __shfl(layer, src, 64);
    const float scl = __shfl(kscl, src, 64);
    const float* img = gb + pl * plane;
    const int rad = (int)rintf(4.5f * scl);
    const float sg = 1.5f * scl, es = -1.f / (2.f * sg * sg);
#pragma unroll 4
    for (int k = 0; k < SIFT_BINS; ++k) hw[k * 64 + lane] = 0.f;
    const int side = 2 * rad + 1, npix = side * side;
    for (int p = lane; p < npix; p += 64) {
      const int i = p / side - rad, j = p % side - rad;
      const int yy = pr + i, xx = pc + j;
      if (yy <= 0 || yy >= h - 1 || xx <= 0 || xx >= w - 1) continue;
      const float* q = img + (int64_t)yy * w + xx;
      const float dx = q[1] - q[-1], dy = q[-w] - q[w];
      const float wgt = expf((float)(i * i + j * j) * es);
      float ang = atan2f(dy, dx) * 57.29577951308232f;
      if (ang < 0.f) ang += 360.f;
      int bin = (int)rintf(ang * (SIFT_BINS / 360.f));
      if (bin >= SIFT_BINS) bin -= SIFT_BINS;
      if (bin < 0) bin += SIFT_BINS;
      bin = min(max(bin, 0), SIFT_BINS - 1);
      hw[bin * 64 + lane] += wgt * sqrtf(dx * dx + dy * dy);
    }
    float mine = 0.f;
    for (int k = 0; k < SIFT_BINS; ++k) {
      const float t = wave_sum(hw[k * 64 + lane]);
      if (lane == k) mine = t;
    }
    const int k0 = lane < SIFT_BINS ? lane : 0;
    const float m2 = __shfl(mine, (k0 + SIFT_BINS - 2) % SIFT_BINS, 64), m1 = __shfl(mine, (k0 + SIFT_BINS - 1) % SIFT_BINS, 64);
    const float p1 = __shfl(mine, (k0 + 1) % SIFT_BINS, 64), p2 = __shfl(mine, (k0 + 2) % SIFT_BINS, 64);
    const float sm = (m2 + p2) * (1.f / 16.f) + (m1 + p1) * (4.f / 16.f) + mine * (6.f / 16.f);
    const float mx = wave_max(lane < SIFT_BINS ? sm : -INFINITY);
    const float lft = __shfl(sm, (k0 + SIFT_BINS - 1) % SIFT_BINS, 64), rgt = __shfl(sm, (k0 + 1) % SIFT_BINS, 64);
    const bool peak = lane < SIFT_BINS && sm > lft && sm > rgt && sm >= 0.8f * mx;
    const int cnt = __popcll(__ballot(peak));
    if (lane == src) nori = cnt;
  }
  if (found) {
    const int idx = atomicAdd(&count[b], 1);
    if (idx < cap) {
      float* o = cand + ((int64_t)b * cap + idx) * 8;
      reinterpret_cast<float4*>(o)[0] = float4{kx, ky, ksize, kresp};
      reinterpret_cast<float4*>(o)[1] = float4{(float)nori, (float)octave, (float)layer, 0.f};
    } else {
      atomicOr(overflow, 1);
    }
  }
}

int launch_blur(bool up, const void* x, float* y, int B, int H, int W, double sigma, void* stream, const char* name) {
  GaussTaps taps;
  int r = 0;
  COMET_CHECK_ARG(make_taps(sigma, taps, r),
                  std::string(name) + ": sigma must be positive with a kernel radius of at most 10 (sigma <= 2.56)");
  const dim3 grid((unsigned)cdiv(W, GB_TW), (unsigned)cdiv(H, GB_TH), (unsigned)B);
  if (up)
    hipLaunchKernelGGL((gauss_blur_kernel<true>), grid, dim3(256), 0, as_stream(stream), x, y, H, W, r, taps);
  else
    hipLaunchKernelGGL((gauss_blur_kernel<false>), grid, dim3(256), 0, as_stream(stream), x, y, H, W, r, taps);
  COMET_CHECK_LAUNCH(name);
  return COMET_OK;
}

constexpr int SIFT_MAX_DIM = 16384;  // 32-bit tile index math; grid.y limit

}  // namespace
}  // namespace comet

using namespace comet;

extern "C" int comet_sift_base(const uint8_t* gray, float* base, int B, int H, int W, void* stream) {
  COMET_CHECK_ARG(gray && base && B > 0 && B <= 65535 && H > 0 && W > 0 && H <= SIFT_MAX_DIM / 2 && W <= SIFT_MAX_DIM / 2,
                  "comet_sift_base: bad args");
  // the input is taken to carry a blur of 0.5 px (1.0 after the up-sampling); bring it to sigma 1.6
  const double sig = std::sqrt(std::fmax(1.6 * 1.6 - 4.0 * 0.5 * 0.5, 0.01));
  return launch_blur(true, gray, base, B, 2 * H, 2 * W, sig, stream, "comet_sift_base");
}

extern "C" int comet_gauss_blur(const float* x, float* y, int B, int H, int W, float sigma, void* stream) {
  COMET_CHECK_ARG(x && y && x != y && B > 0 && B <= 65535 && H > 0 && W > 0 && H <= SIFT_MAX_DIM && W <= SIFT_MAX_DIM,
                  "comet_gauss_blur: bad args");
  return launch_blur(false, x, y, B, H, W, (double)sigma, stream, "comet_gauss_blur");
}

extern "C" int comet_downsample2(const float* x, float* y, int B, int H, int W, void* stream) {
  COMET_CHECK_ARG(x && y && x != y && B > 0 && H >= 2 && W >= 2 && H <= SIFT_MAX_DIM && W <= SIFT_MAX_DIM,
                  "comet_downsample2: bad args");
  int64_t gsz = cdiv((int64_t)B * (H / 2) * (W / 2), 256);
  if (gsz > 65536) gsz = 65536;
  hipLaunchKernelGGL(downsample2_kernel, dim3((unsigned)gsz), dim3(256), 0, as_stream(stream), x, y, B, H, W);
  COMET_CHECK_LAUNCH("comet_downsample2");
  return COMET_OK;
}

extern "C" int comet_sift_detect(const float* gauss, int B, int n_layers, int h, int w, int octave,
                                 float contrast_threshold, float edge_threshold, float sigma, float* cand, int cap,
                                 int* count, int* overflow, void* stream) {
  COMET_CHECK_ARG(gauss && cand && count && overflow && B > 0 && h > 0 && w > 0 && h <= SIFT_MAX_DIM && w <= SIFT_MAX_DIM,
                  "comet_sift_detect: bad args");
  COMET_CHECK_ARG(n_layers >= 1 && n_layers <= 8 && (int64_t)B * n_layers <= 65535 && octave >= 0 && octave < 24 &&
                      cap > 0 && sigma > 0.f && contrast_threshold >= 0.f && edge_threshold > 0.f,
                  "comet_sift_detect: bad parameters");
  COMET_CHECK_ARG(((uintptr_t)cand & 15) == 0, "comet_sift_detect: the candidate buffer must be 16-byte aligned");
  if (h <= 2 * SIFT_BORDER || w <= 2 * SIFT_BORDER) return COMET_OK;  // no pixel inside the 5-px border
  const float thr = std::floor(0.5f * contrast_threshold / n_layers * 255.f);
  const dim3 grid((unsigned)cdiv(w - 2 * SIFT_BORDER, DT_W), (unsigned)cdiv(h - 2 * SIFT_BORDER, DT_H),
                  (unsigned)(B * n_layers));
  hipLaunchKernelGGL(sift_detect_kernel, grid, dim3(256), 0, as_stream(stream), gauss, n_layers + 3, h, w, octave,
                     n_layers, thr, contrast_threshold, edge_threshold, sigma, cand, cap, count, overflow);
  COMET_CHECK_LAUNCH("comet_sift_detect");
  return COMET_OK;
}
