// LPIPS(net="vgg", version="0.1") around the VGG16 convolutions (which run through vneti_gemm_f16): the scaling layer fused
// with conv1_1's 3-channel im2col, the ReLU of the eight untapped convolutions, ReLU + 2x2 max-pool after the five tapped
// ones, and the per-layer distance (channel-normalised squared difference weighted by the linear head, spatial mean).
// Restates lpips 0.1.4 (lpips/pretrained_networks.py vgg16, lpips/lpips.py LPIPS.forward, ScalingLayer, normalize_tensor,
// spatial_average) as the reference calls it in training/inference_dtu.py and scripts/summarize_dtu.py.
//
// Deterministic: the distance sums per block in a fixed order, writes the block partials to a workspace and a second kernel
// finishes them in block order; no float atomics, so a pair's value depends only on its two feature maps.
#include "common.h"
#include "../../include/vneti.h"

namespace {

// lpips.ScalingLayer: x' = (x - shift) / scale (f32, IEEE division: the oracle's arithmetic)
__device__ __forceinline__ float lp_scale(float v, int c) {
  const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
  const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
  return (v - shift) / scale;
}

// out[m][tap*3 + c] (row length 64, columns 27..63 zero), m = (b, y, x): the scaled image's 3x3 neighbourhood with the
// zero padding of conv1_1 applied AFTER scaling (a padded tap is 0, not (0 - shift) / scale)
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ x, long long sb, long long sc,
                                                         long long sy, long long sx, half_t* __restrict__ out, int M,
                                                         int H, int W) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)M * 8) return;
  const int m = (int)(gid >> 3), ch = (int)(gid & 7);
  const int HW = H * W;
  const int b = m / HW, r = m - b * HW, oy = r / W, ox = r - oy * W;
  half8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = ch * 8 + j;
    float val = 0.f;
    if (k < 27) {
      const int tap = k / 3, c = k - tap * 3;
      const int dy = tap / 3, dx = tap - dy * 3;
      const int iy = oy + dy - 1, ix = ox + dx - 1;
      if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
        val = lp_scale(x[(long long)b * sb + (long long)c * sc + (long long)iy * sy + (long long)ix * sx], c);
    }
    v[j] = (half_t)val;
  }
  *reinterpret_cast<half8*>(out + (long long)m * 64 + ch * 8) = v;
}

// ReLU that keeps NaN (torch.relu does): a non-finite activation must reach the result, where the engine checks it
__device__ __forceinline__ half_t lp_relu(half_t v) { return v < (half_t)0.f ? (half_t)0.f : v; }
// max that keeps NaN (F.max_pool2d does)
__device__ __forceinline__ half_t lp_max(half_t a, half_t b) { return (b != b || b > a) ? b : a; }

__global__ __launch_bounds__(256) void relu_kernel(half_t* __restrict__ x, long long n8) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n8) return;
  half8 v = reinterpret_cast<half8*>(x)[gid];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = lp_relu(v[j]);
  reinterpret_cast<half8*>(x)[gid] = v;
}

// NHWC [Bn][H][W][C] -> [Bn][H/2][W/2][C] (floor): relu(max of the 2x2 window), eight channels per thread
__global__ __launch_bounds__(256) void relu_maxpool_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, int Bn,
                                                          int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, cch = C / 8;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)Bn * Ho * Wo * cch) return;
  const int c = (int)(gid % cch) * 8;
  const long long p = gid / cch;
  const int ox = (int)(p % Wo);
  const long long q = p / Wo;
  const int oy = (int)(q % Ho), b = (int)(q / Ho);
  const half_t* s = x + (((long long)b * H + 2 * oy) * W + 2 * ox) * C + c;
  const half8 a0 = *reinterpret_cast<const half8*>(s);
  const half8 a1 = *reinterpret_cast<const half8*>(s + C);
  const half8 a2 = *reinterpret_cast<const half8*>(s + (long long)W * C);
  const half8 a3 = *reinterpret_cast<const half8*>(s + (long long)W * C + C);
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = lp_relu(lp_max(lp_max(lp_max(a0[j], a1[j]), a2[j]), a3[j]));
  *reinterpret_cast<half8*>(y + gid * 8) = o;
}

// blocks per pair of the distance: a function of the layer's geometry only, so a pair's reduction order never depends on
// how many pairs share the launch or where it sits in the table
constexpr int kDistThreads = 256;
inline int lp_dist_blocks(int C, int HW) {
  const int ppi = kDistThreads / (C / 8);  // pixels per block iteration
  int nb = cdiv(HW, ppi * 16);
  return nb < 1 ? 1 : (nb > 128 ? 128 : nb);
}

template <int L>  // lanes per pixel = C / 8
__device__ __forceinline__ float lp_group_sum(float v) {
#pragma unroll
  for (int o = 1; o < L; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// stage 1: block `blk` of pair p sums d over its pixel range into ws[p * nblk + blk]
template <int L>
__global__ __launch_bounds__(kDistThreads) void lpips_dist_kernel(const half_t* __restrict__ feat, int n_img,
                                                                  const int* __restrict__ pairs, const float* __restrict__ w,
                                                                  int HW, int nblk, float* __restrict__ ws) {
  constexpr int C = L * 8, PPI = kDistThreads / L;
  const int p = blockIdx.y, blk = blockIdx.x;
  const int t = threadIdx.x, g = t / L, q = t % L;
  const int i0 = pairs[2 * p], i1 = pairs[2 * p + 1];
  __shared__ float red[kDistThreads];
  float acc = 0.f;
  if ((unsigned)i0 < (unsigned)n_img && (unsigned)i1 < (unsigned)n_img) {
    float wr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wr[j] = w[q * 8 + j];
    const int per = cdiv_dev(HW, nblk), beg = blk * per, end = min(HW, beg + per);
    const half_t* f0 = feat + (long long)i0 * HW * C + q * 8;
    const half_t* f1 = feat + (long long)i1 * HW * C + q * 8;
    for (int base = beg; base < end; base += PPI) {
      const int pix = base + g;
      const bool live = pix < end;  // the whole L-lane group agrees: shuffles stay inside live groups
      half8 a = {}, b = {};
      if (live) {
        a = *reinterpret_cast<const half8*>(f0 + (long long)pix * C);
        b = *reinterpret_cast<const half8*>(f1 + (long long)pix * C);
      }
      float x0[8], x1[8], s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x0[j] = (float)lp_relu(a[j]);
        x1[j] = (float)lp_relu(b[j]);
        s0 += x0[j] * x0[j];
        s1 += x1[j] * x1[j];
      }
      s0 = lp_group_sum<L>(s0);
      s1 = lp_group_sum<L>(s1);
      const float r0 = sqrtf(s0) + 1e-10f, r1 = sqrtf(s1) + 1e-10f;
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float e = x0[j] / r0 - x1[j] / r1;
        d += wr[j] * (e * e);
      }
      d = lp_group_sum<L>(d);
      if (live && q == 0) acc += d;
    }
  } else {
    acc = (t == 0) ? __builtin_nanf("") : 0.f;  // a pair outside the feature batch: NaN, which the engine refuses
  }
  red[t] = acc;
  __syncthreads();
#pragma unroll
  for (int s = kDistThreads / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) ws[(long long)p * nblk + blk] = red[0];
}

// stage 2: out[p] (+)= (sum of the pair's partials in block order) / HW
__global__ __launch_bounds__(256) void lpips_dist_finish_kernel(const float* __restrict__ ws, int P, int nblk, int HW,
                                                                float* __restrict__ out, int accumulate) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += (double)ws[(long long)p * nblk + k];
  const float mean = (float)(s / (double)HW);
  out[p] = accumulate ? out[p] + mean : mean;
}

}  // namespace

extern "C" int vneti_lpips_prep(const float* x, long long sb, long long sc, long long sy, long long sx, void* out, int Bn,
                                int H, int W, void* stream) {
  VN_REQUIRE(x && out && Bn > 0 && H > 0 && W > 0, "lpips_prep: bad arguments");
  const long long M = (long long)Bn * H * W;
  VN_REQUIRE_OUT("lpips_prep", vn_out_bytes(M, 64, 64, 2));
  hipLaunchKernelGGL(lpips_prep_kernel, dim3((unsigned)cdivl(M * 8, 256)), dim3(256), 0, (hipStream_t)stream, x, sb, sc,
                     sy, sx, (half_t*)out, (int)M, H, W);
  return vneti_check_launch("lpips_prep");
}

extern "C" int vneti_relu_f16(void* x, long long n, void* stream) {
  VN_REQUIRE(x && n > 0 && n % 8 == 0, "relu_f16: n=%lld must be a positive multiple of 8", n);
  VN_REQUIRE_OUT("relu_f16", n * 2);
  hipLaunchKernelGGL(relu_kernel, dim3((unsigned)cdivl(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, (half_t*)x, n / 8);
  return vneti_check_launch("relu_f16");
}

extern "C" int vneti_relu_maxpool2x2_f16(const void* x, void* y, int Bn, int H, int W, int C, void* stream) {
  VN_REQUIRE(x && y && x != y && Bn > 0 && H >= 2 && W >= 2 && C > 0 && C % 8 == 0,
             "relu_maxpool2x2: bad arguments (H=%d W=%d C=%d; C %% 8 == 0, H, W >= 2, out of place)", H, W, C);
  VN_REQUIRE_OUT("relu_maxpool2x2 input", vn_out_bytes((long long)Bn * H * W, C, C, 2));
  const long long n = (long long)Bn * (H / 2) * (W / 2) * (C / 8);
  hipLaunchKernelGGL(relu_maxpool_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)x, (half_t*)y, Bn, H, W, C);
  return vneti_check_launch("relu_maxpool2x2");
}

extern "C" long long vneti_lpips_ws_floats(int P, int C, int HW) {
  if (P <= 0 || HW <= 0 || (C != 64 && C != 128 && C != 256 && C != 512)) return -1;
  return (long long)P * lp_dist_blocks(C, HW);
}

extern "C" int vneti_lpips_distance(const void* feat, int n_img, const int* pairs, int P, const float* w, int C, int HW,
                                    float* ws, long long ws_floats, float* out, int accumulate, void* stream) {
  VN_REQUIRE(feat && pairs && w && ws && out && n_img > 0 && P > 0 && HW > 0, "lpips_distance: bad arguments");
  VN_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512, "lpips_distance: C=%d must be 64, 128, 256 or 512", C);
  VN_REQUIRE(P <= 65535, "lpips_distance: %d pairs, at most 65535 per launch", P);
  VN_REQUIRE((long long)n_img * HW * C * 2 < 0x7fffffffLL, "lpips_distance: feature batch larger than 2 GiB");
  const int nblk = lp_dist_blocks(C, HW);
  VN_REQUIRE(ws_floats >= (long long)P * nblk, "lpips_distance: workspace needs %lld floats", (long long)P * nblk);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nblk, P);
  const half_t* f = (const half_t*)feat;
  switch (C) {
    case 64: hipLaunchKernelGGL(lpips_dist_kernel<8>, grid, dim3(kDistThreads), 0, st, f, n_img, pairs, w, HW, nblk, ws); break;
    case 128: hipLaunchKernelGGL(lpips_dist_kernel<16>, grid, dim3(kDistThreads), 0, st, f, n_img, pairs, w, HW, nblk, ws); break;
    case 256: hipLaunchKernelGGL(lpips_dist_kernel<32>, grid, dim3(kDistThreads), 0, st, f, n_img, pairs, w, HW, nblk, ws); break;
    default: hipLaunchKernelGGL(lpips_dist_kernel<64>, grid, dim3(kDistThreads), 0, st, f, n_img, pairs, w, HW, nblk, ws); break;
  }
  const int rc = vneti_check_launch("lpips_distance");
  if (rc != VNETI_OK) return rc;
  hipLaunchKernelGGL(lpips_dist_finish_kernel, dim3(cdiv(P, 256)), dim3(256), 0, st, ws, P, nblk, HW, out, accumulate ? 1 : 0);
  return vneti_check_launch("lpips_distance_finish");
}
