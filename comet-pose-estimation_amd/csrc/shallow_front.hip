// The fine ShallowEncoder's front in one kernel (blocks.py:114-196 + modules.py:39-116 of the
// reference; ShallowEncoder.forward / ResidualBlock.forward here): per 31 x 31 x 8 bf16 patch
//   x    = relu(IN(conv1 3x3 s2 (patch)))                                   [16, 16, 32]
//   tmp1 = relu(IN(l1.down 1x1 s2 (x))    + relu(IN(l1.conv2(relu(IN(l1.conv1 3x3 s2 (x)))))))     [8, 8, 32]
//   tmp2 = relu(IN(l2.down 1x1 s2 (tmp1)) + relu(IN(l2.conv2(relu(IN(l2.conv1 3x3 s2 (tmp1)))))))  [4, 4, 32]
// -- seven convolutions and seven InstanceNorms that ran as 14 launches, every map written to HBM,
// re-read by its InstanceNorm, written again and re-read by the next convolution. Here one wave owns
// one patch from its input to tmp2: the patch is copied to LDS once (coalesced 16-B loads, the next
// patch's in flight while this one computes), every convolution takes its B fragments from the LDS
// map of its input and leaves its output in registers (MFMA accumulator layout), the InstanceNorm
// runs on those registers, and only the three results the encoder's tail reads go to HBM.
//
// Bit-identical to the unfused launches:
//  * convolutions as conv_skinny_kernel (gemm.hip): v_mfma_f32_16x16x32_bf16 with W as the A operand,
//    one accumulator chain from zero over the 32-wide k chunks in (tap, ci) order, zero fragments for
//    padding taps and k >= K, + bias in f32, rounded to bf16;
//  * InstanceNorm as in_wave_kernel (norm.hip) through the shared helpers of common.hpp: the MFMA
//    accumulator layout already has in_wave_kernel's order of summation -- lane li of a 16-pixel
//    step holds pixel 16 k + li exactly as in_wave_kernel's slot li holds pixels li + 16 k, so the
//    per-lane partial sums run over k in the same order, and the butterfly over the 16 lanes of a
//    row (lane ^ 1, 2, 4, 8; on DPP, no LDS round trip) pairs the same slots in the same order as
//    offsets 4 .. 32 do there.
//
// One workgroup (4 waves, one per SIMD) per CU, persistent: the four 3x3 c32 weights (pitch K + 8, so
// the b128 A-fragment reads of 16 rows are conflict-free), the two 1x1 weights and the biases stay in
// LDS for the whole launch (80 KiB); each wave has a private 20 KiB map region (pixel pitch C + 8 as
// conv3_rows_kernel), which holds the input patch, then x, then the 8 x 8 and 4 x 4 maps. 159 KiB of
// the CU's 160: a second wave per SIMD does not fit, the prefetch of the next patch hides the HBM
// latency instead. Waves never share map data, so the phases are ordered by wave-scope fences only.
#include <cstdlib>

#include "common.hpp"

namespace comet {
namespace {
namespace sf {

constexpr int P = 31, CIN = 8, C = 32, NCONV = 7;  // patch side, padded input channels, channels
constexpr int H0 = 16, H1 = 8, H2 = 4;             // map sides after conv1 / layer1 / layer2
constexpr int K1 = 9 * CIN, K3 = 9 * C;            // k of conv1 and of the 3x3 c32 convolutions
constexpr int PXP = C + 8;                         // pixel pitch of a c32 map in LDS (elements)
constexpr int WP3 = K3 + 8;                        // 3x3 weight row pitch in LDS (elements)
constexpr int W3 = C * WP3, W1 = C * C;            // one 3x3 / 1x1 weight in LDS (elements)
constexpr int MAP = H0 * H0 * PXP;                 // one wave's map region (elements)
constexpr int NW = 4;                              // waves (= patches in flight) per workgroup
constexpr int IN_VEC = P * P;                      // 16-B vectors (= pixels) of one input patch
constexpr int IN_REGS = (IN_VEC + 63) / 64;        // of those per lane
static_assert(IN_VEC * CIN <= MAP, "the input patch shares the map region");
// map region: x at 0; once x is dead the 8 x 8 maps y1 (layer1.conv1's) at 0 and tmp1 behind it, then
// the 4 x 4 map y2 (layer2.conv1's)
constexpr int OFF_Y1 = 0, OFF_T1 = H1 * H1 * PXP, OFF_Y2 = 2 * H1 * H1 * PXP;
static_assert(OFF_Y2 + H2 * H2 * PXP <= MAP, "map region");
constexpr size_t LDS_BYTES = (size_t)(4 * W3 + 2 * W1 + NW * MAP) * sizeof(__bf16) + NCONV * C * sizeof(float);
static_assert(LDS_BYTES <= 160 * 1024, "LDS");

// convolution order of the weight / bias arrays
enum { CONV1 = 0, L1C1, L1C2, L1DS, L2C1, L2C2, L2DS };

struct Params {
  const __bf16* w[NCONV];
  const float* b[NCONV];
};

// LDS traffic between the lanes of one wave: the hardware runs a wave's LDS operations in order, the
// fences keep the compiler from moving them across
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int CTRL>
__device__ __forceinline__ float row_dpp(float v) {
  return __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), CTRL, 0xF, 0xF, false));
}

__device__ __forceinline__ float round_bf16(float v) { return to_f32(from_f32<__bf16>(v)); }

// 16-pixel steps of a KS x KS / stride / pad convolution of the IH x IH x 32 LDS map `map` with the
// LDS weight `wl` (row pitch WPITCH), + bias, rounded to bf16: out[s][nt][r] = channel
// 16 nt + 4 g + r of output pixel 16 s + li. The A fragments of a tap are read once for all steps.
template <int IH, int KS, int STRIDE, int PAD, int WPITCH, int STEPS>
__device__ __forceinline__ void conv_c32(const __bf16* map, const __bf16* wl, const float* bl, int li, int g,
                                         float (&out)[STEPS][2][4]) {
  constexpr int OH = (IH + 2 * PAD - KS) / STRIDE + 1;
  static_assert(OH * OH == 16 * STEPS, "whole 16-pixel steps");
  f32x4 acc[STEPS][2];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) acc[s][0] = acc[s][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < KS * KS; ++t) {
    const int ky = t / KS, kx = t % KS;
    const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(wl + li * WPITCH + 32 * t + 8 * g);
    const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(wl + (16 + li) * WPITCH + 32 * t + 8 * g);
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int m = 16 * s + li;
      const int iy = (m / OH) * STRIDE - PAD + ky, ix = (m % OH) * STRIDE - PAD + kx;
      const bool ok = iy >= 0 && iy < IH && ix >= 0 && ix < IH;
      const int px = ok ? iy * IH + ix : 0;
      COMET_DASSERT(px >= 0 && px < IH * IH);
      bf16x8 b = *reinterpret_cast<const bf16x8*>(map + px * PXP + 8 * g);
      if (!ok) b = bf16x8{};
      acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc[s][0], 0, 0, 0);
      acc[s][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc[s][1], 0, 0, 0);
    }
  }
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(bl + 4 * g), b1 = *reinterpret_cast<const f32x4*>(bl + 16 + 4 * g);
#pragma unroll
  for (int s = 0; s < STEPS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      out[s][0][r] = round_bf16(acc[s][0][r] + b0[r]);
      out[s][1][r] = round_bf16(acc[s][1][r] + b1[r]);
    }
}

// InstanceNorm of a 16 STEPS-pixel map held in the accumulator layout (in place, rounded to bf16):
// in_wave_kernel's arithmetic, see the head of the file
template <int STEPS, bool RELU_INNER, bool RES, bool RELU>
__device__ __forceinline__ void inorm(float (&v)[STEPS][2][4], const float (&res)[STEPS][2][4], float eps, int lane) {
  const float inv = 1.f / (float)(16 * STEPS);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float K = __shfl(v[0][nt][r], lane & 48, 64);  // pixel 0 of this lane's channel
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int s = 0; s < STEPS; ++s) in_moment_add(v[s][nt][r], K, a, b);
      // the xor butterfly over the 16 lanes of a row on DPP: after the two quad steps every lane of a
      // quad holds the quad's sum (the same bits: addition commutes), so any lane of the other quad
      // (half mirror), then of the other half row (mirror), is the xor 4 / xor 8 partner's value
      a += row_dpp<0xB1>(a);   // quad_perm [1,0,3,2]: lane ^ 1
      b += row_dpp<0xB1>(b);
      a += row_dpp<0x4E>(a);   // quad_perm [2,3,0,1]: lane ^ 2
      b += row_dpp<0x4E>(b);
      a += row_dpp<0x141>(a);  // row_half_mirror
      b += row_dpp<0x141>(b);
      a += row_dpp<0x140>(a);  // row_mirror
      b += row_dpp<0x140>(b);
      float mu, rs;
      in_mean_rstd(a, b, inv, K, eps, mu, rs);
#pragma unroll
      for (int s = 0; s < STEPS; ++s)
        v[s][nt][r] = round_bf16(in_normalize(v[s][nt][r], mu, rs, RELU_INNER, RES, RES ? res[s][nt][r] : 0.f, RELU));
    }
}

// a map from the accumulator layout to LDS (pixel pitch PXP) and / or HBM (dense), 16 B per lane and
// step: channel blocks 0 / 1 exchange lane-group halves as conv_skinny_kernel's wide stores do
template <int STEPS>
__device__ __forceinline__ void store_map(const float (&v)[STEPS][2][4], __bf16* ls, __bf16* gs, int li, int g) {
  const int wcol = 16 * (g & 1) + 8 * (g >> 1);
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const unsigned p00 = pack_bf16x2(v[s][0][0], v[s][0][1]), p01 = pack_bf16x2(v[s][0][2], v[s][0][3]);
    const unsigned p10 = pack_bf16x2(v[s][1][0], v[s][1][1]), p11 = pack_bf16x2(v[s][1][2], v[s][1][3]);
    const auto s0 = __builtin_amdgcn_permlane16_swap(p00, p10, false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap(p01, p11, false, false);
    const uint4 u = uint4{s0[0], s1[0], s0[1], s1[1]};
    const int px = 16 * s + li;
    COMET_DASSERT(px < 16 * STEPS);
    if (ls) *reinterpret_cast<uint4*>(ls + px * PXP + wcol) = u;
    if (gs) *reinterpret_cast<uint4*>(gs + px * C + wcol) = u;
  }
}

__global__ void __launch_bounds__(64 * NW)
shallow_front_kernel(const __bf16* __restrict__ patches, Params pr, __bf16* __restrict__ xo, __bf16* __restrict__ t1o,
                     __bf16* __restrict__ t2o, int n, float eps) {
  extern __shared__ __attribute__((aligned(16))) __bf16 lds[];
  __bf16* w3s = lds;                                               // [4][C][WP3]: l1.conv1, l1.conv2, l2.conv1, l2.conv2
  __bf16* w1s = w3s + 4 * W3;                                      // [2][C][C]: l1.down, l2.down
  __bf16* maps = w1s + 2 * W1;                                     // [NW][MAP]
  float* bs = reinterpret_cast<float*>(maps + NW * MAP);           // [NCONV][C]
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4, wv = tid >> 6;

  // weights and biases: once per workgroup
  constexpr int w3src[4] = {L1C1, L1C2, L2C1, L2C2}, w1src[2] = {L1DS, L2DS};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    for (int i = tid; i < C * (K3 / 8); i += 64 * NW) {
      const int co = i / (K3 / 8), c = i % (K3 / 8);
      *reinterpret_cast<uint4*>(w3s + j * W3 + co * WP3 + 8 * c) = *reinterpret_cast<const uint4*>(pr.w[w3src[j]] + co * K3 + 8 * c);
    }
#pragma unroll
  for (int j = 0; j < 2; ++j)
    for (int i = tid; i < W1 / 8; i += 64 * NW)
      *reinterpret_cast<uint4*>(w1s + j * W1 + 8 * i) = *reinterpret_cast<const uint4*>(pr.w[w1src[j]] + 8 * i);
#pragma unroll
  for (int j = 0; j < NCONV; ++j)
    if (tid < C) bs[j * C + tid] = pr.b[j][tid];
  // conv1's weight (K = 72: three k chunks, the third a quarter full) as register A fragments, and
  // the tap of each of this lane's k chunks
  bf16x8 wf1[2][3];
  int tky[3], tkx[3];
  bool tv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int k0 = 32 * c + 8 * g, tap = k0 / CIN;
    tv[c] = k0 < K1;
    tky[c] = tap / 3;
    tkx[c] = tap - 3 * tky[c];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      wf1[nt][c] = tv[c] ? *reinterpret_cast<const bf16x8*>(pr.w[CONV1] + (nt * 16 + li) * K1 + k0) : bf16x8{};
  }
  __syncthreads();

  __bf16* mp = maps + wv * MAP;
  const int first = blockIdx.x * NW + wv, stride = gridDim.x * NW;
  uint4 pin[IN_REGS];
  auto prefetch = [&](int p) {
    const uint4* src = reinterpret_cast<const uint4*>(patches + (int64_t)p * (IN_VEC * CIN));
#pragma unroll
    for (int i = 0; i < IN_REGS; ++i) {
      const int idx = lane + 64 * i;
      pin[i] = idx < IN_VEC ? src[idx] : uint4{0, 0, 0, 0};
    }
  };
  if (first < n) prefetch(first);
  for (int p = first; p < n; p += stride) {
    wave_sync();  // the previous patch's last map reads
#pragma unroll
    for (int i = 0; i < IN_REGS; ++i) {
      const int idx = lane + 64 * i;
      if (idx < IN_VEC) reinterpret_cast<uint4*>(mp)[idx] = pin[i];
    }
    if (p + stride < n) prefetch(p + stride);
    wave_sync();

    // conv1 (3x3 s2 p1, c8 -> 32): step s = output row s, lane li = output column
    float x[H0][2][4];
    {
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(bs + CONV1 * C + 4 * g);
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(bs + CONV1 * C + 16 + 4 * g);
#pragma unroll
      for (int s = 0; s < H0; ++s) {
        f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int iy = 2 * s - 1 + tky[c], ix = 2 * li - 1 + tkx[c];
          const bool ok = tv[c] && iy >= 0 && iy < P && ix >= 0 && ix < P;
          const int px = ok ? iy * P + ix : 0;
          COMET_DASSERT(px >= 0 && px < IN_VEC);
          bf16x8 b = *reinterpret_cast<const bf16x8*>(mp + px * CIN);
          if (!ok) b = bf16x8{};
          a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1[0][c], b, a0, 0, 0, 0);
          a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1[1][c], b, a1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[s][0][r] = round_bf16(a0[r] + b0[r]);
          x[s][1][r] = round_bf16(a1[r] + b1[r]);
        }
      }
    }
    inorm<H0, false, false, true>(x, x, eps, lane);
    wave_sync();  // the input patch is read: x goes over it
    store_map<H0>(x, mp, xo + (int64_t)p * (H0 * H0 * C), li, g);
    wave_sync();

    // layer1: conv1 3x3 s2 and the 1x1 s2 shortcut read x; conv2 reads conv1's normalised output
    float y[H1 * H1 / 16][2][4], d[H1 * H1 / 16][2][4];
    conv_c32<H0, 3, 2, 1, WP3>(mp, w3s + 0 * W3, bs + L1C1 * C, li, g, y);
    inorm<H1 * H1 / 16, false, false, true>(y, y, eps, lane);
    conv_c32<H0, 1, 2, 0, C>(mp, w1s + 0 * W1, bs + L1DS * C, li, g, d);
    inorm<H1 * H1 / 16, false, false, false>(d, d, eps, lane);
    wave_sync();  // x is read: the 8 x 8 maps go over it
    store_map<H1 * H1 / 16>(y, mp + OFF_Y1, nullptr, li, g);
    wave_sync();
    conv_c32<H1, 3, 1, 1, WP3>(mp + OFF_Y1, w3s + 1 * W3, bs + L1C2 * C, li, g, y);
    inorm<H1 * H1 / 16, true, true, true>(y, d, eps, lane);
    store_map<H1 * H1 / 16>(y, mp + OFF_T1, t1o + (int64_t)p * (H1 * H1 * C), li, g);
    wave_sync();

    // layer2 the same on tmp1
    float z[1][2][4], e[1][2][4];
    conv_c32<H1, 3, 2, 1, WP3>(mp + OFF_T1, w3s + 2 * W3, bs + L2C1 * C, li, g, z);
    inorm<1, false, false, true>(z, z, eps, lane);
    conv_c32<H1, 1, 2, 0, C>(mp + OFF_T1, w1s + 1 * W1, bs + L2DS * C, li, g, e);
    inorm<1, false, false, false>(e, e, eps, lane);
    store_map<1>(z, mp + OFF_Y2, nullptr, li, g);
    wave_sync();
    conv_c32<H2, 3, 1, 1, WP3>(mp + OFF_Y2, w3s + 3 * W3, bs + L2C2 * C, li, g, z);
    inorm<1, true, true, true>(z, e, eps, lane);
    store_map<1>(z, nullptr, t2o + (int64_t)p * (H2 * H2 * C), li, g);
  }
}

int num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      cus = v;
    else
      cus = 256;
  }
  return cus;
}

}  // namespace sf
}  // namespace
}  // namespace comet

extern "C" int comet_shallow_front_nhwc(int dtype, const void* patches, const void* const* weights,
                                        const float* const* biases, void* x, void* tmp1, void* tmp2, int64_t n,
                                        int64_t p, int64_t c, float eps, void* stream) {
  using namespace comet;
  COMET_CHECK_ARG(dtype == COMET_BF16, "comet_shallow_front_nhwc: patches, weights and outputs must be bf16");
  COMET_CHECK_ARG(patches && weights && biases && x && tmp1 && tmp2, "comet_shallow_front_nhwc: null pointer");
  COMET_CHECK_ARG(p == sf::P && c == sf::CIN,
                  "comet_shallow_front_nhwc: written for the ShallowEncoder's geometry (31 x 31 patches of 8 channels)");
  COMET_CHECK_ARG(n > 0 && n < (1ll << 31) / 256, "comet_shallow_front_nhwc: n must be in [1, 2^31 / 256)");
  COMET_CHECK_ARG(((uintptr_t)patches | (uintptr_t)x | (uintptr_t)tmp1 | (uintptr_t)tmp2) % 16 == 0,
                  "comet_shallow_front_nhwc: patches and outputs must be 16-byte aligned");
  sf::Params pr;
  for (int i = 0; i < sf::NCONV; ++i) {
    COMET_CHECK_ARG(weights[i] && biases[i], "comet_shallow_front_nhwc: null weight or bias");
    COMET_CHECK_ARG((uintptr_t)weights[i] % 16 == 0 && (uintptr_t)biases[i] % 4 == 0,
                    "comet_shallow_front_nhwc: weights must be 16-byte aligned (biases 4)");
    pr.w[i] = reinterpret_cast<const __bf16*>(weights[i]);
    pr.b[i] = biases[i];
  }
  hipStream_t s = as_stream(stream);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)sf::shallow_front_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)sf::LDS_BYTES);
    attr = true;
  }
  int64_t grid = cdiv(n, sf::NW);
  if (grid > sf::num_cus()) grid = sf::num_cus();
  hipLaunchKernelGGL(sf::shallow_front_kernel, dim3((unsigned)grid), dim3(64 * sf::NW), sf::LDS_BYTES, s,
                     (const __bf16*)patches, pr, (__bf16*)x, (__bf16*)tmp1, (__bf16*)tmp2, (int)n, eps);
  COMET_CHECK_LAUNCH("comet_shallow_front_nhwc");
  return COMET_OK;
}
