// Small HBM/latency-bound kernels around the GEMMs: residual add, GEGLU, quick-GELU, sinusoidal
// timestep embedding, 2x2 gradient pooling (nearest-upsample backward), the fused latent
// sampling + DDPM add-noise, MSE loss + its gradient seed, AdamW with GradScaler semantics and
// the device-side RNG that keeps the whole train step hipGraph-capturable.
//
// Reference call sites: training/coach.py:165-183 (latent sample, randn_like, randint,
// add_noise), :201-214 (target, mse_loss, backward), :216-218 (AdamW step) and diffusers'
// GEGLU / Timesteps / Upsample2D inside `self.unet(...)` (:197).
#include "common.h"
#include "../../include/vneti.h"

namespace {

__device__ __forceinline__ uint32_t hash_u32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
// counter-based standard normal (Box-Muller on two hashed uniforms)
__device__ __forceinline__ float rng_normal(uint32_t seed, uint32_t ctr, uint32_t idx) {
  uint32_t a = hash_u32(idx * 0x9E3779B1U + seed);
  a = hash_u32(a ^ (ctr * 0x85EBCA6BU + 0x632BE5ABU));
  uint32_t b = hash_u32(a + 0x68E31DA4U);
  float u1 = ((a >> 8) + 1u) * (1.0f / 16777216.0f);  // (0, 1]
  float u2 = (b >> 8) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * __logf(u1)) * __cosf(6.283185307179586f * u2);
}

__global__ __launch_bounds__(256) void add_kernel(const half_t* a, long long lda, const half_t* b, long long ldb,
                                                  half_t* out, long long ldo, int rows, int cchunks) {
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)rows * cchunks) return;
  int r = (int)(gid / cchunks), c = (int)(gid - (long long)r * cchunks) * 8;
  half8 x = *reinterpret_cast<const half8*>(a + (long long)r * lda + c);
  half8 y = *reinterpret_cast<const half8*>(b + (long long)r * ldb + c);
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)x[j] + (float)y[j]);
  vn_st16_wt(vn_make_rsrc(out, 0x7fffffffu), (uint32_t)(((long long)r * ldo + c) * 2), o);
}

// GEGLU: p = [h | g] (each C4 wide); out = h * gelu_erf(g)
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const half_t* p, long long ldp, half_t* out, long long ldo,
                                                        int rows, int C4) {
  int cch = C4 / 8;
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)rows * cch) return;
  int r = (int)(gid / cch), c = (int)(gid - (long long)r * cch) * 8;
  half8 h = *reinterpret_cast<const half8*>(p + (long long)r * ldp + c);
  half8 g = *reinterpret_cast<const half8*>(p + (long long)r * ldp + C4 + c);
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)h[j] * vn_gelu_erf((float)g[j]));
  *reinterpret_cast<half8*>(out + (long long)r * ldo + c) = o;
}
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const half_t* dy, long long lddy, const half_t* p,
                                                        long long ldp, half_t* dp, long long lddp, int rows,
                                                        int C4) {
  int cch = C4 / 8;
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)rows * cch) return;
  int r = (int)(gid / cch), c = (int)(gid - (long long)r * cch) * 8;
  half8 d = *reinterpret_cast<const half8*>(dy + (long long)r * lddy + c);
  half8 h = *reinterpret_cast<const half8*>(p + (long long)r * ldp + c);
  half8 g = *reinterpret_cast<const half8*>(p + (long long)r * ldp + C4 + c);
  half8 dh, dg;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float gv = (float)g[j], dv = (float)d[j], hv = (float)h[j];
    float cdf, xpdf;
    vn_gelu_parts(gv, cdf, xpdf);
    dh[j] = (half_t)(dv * gv * cdf);
    dg[j] = (half_t)(dv * hv * (cdf + xpdf));
  }
  *reinterpret_cast<half8*>(dp + (long long)r * lddp + c) = dh;
  *reinterpret_cast<half8*>(dp + (long long)r * lddp + C4 + c) = dg;
}

// y = act(x) and dx = dy * act'(x) for the CLIP MLP (quick-GELU or exact GELU), f16
__global__ __launch_bounds__(256) void act_fwd_kernel(const half_t* x, half_t* y, long long n8, int act) {
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n8) return;
  half8 v = *reinterpret_cast<const half8*>(x + gid * 8), o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f = (float)v[j];
    o[j] = (half_t)(act == 2 ? vn_quick_gelu(f) : (act == 3 ? vn_gelu_erf(f) : vn_silu(f)));
  }
  *reinterpret_cast<half8*>(y + gid * 8) = o;
}
__global__ __launch_bounds__(256) void act_bwd_kernel(const half_t* dy, const half_t* x, half_t* dx, long long n8,
                                                      int act) {
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n8) return;
  half8 d = *reinterpret_cast<const half8*>(dy + gid * 8);
  half8 v = *reinterpret_cast<const half8*>(x + gid * 8), o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f = (float)v[j], g;
    if (act == 2) {
      float s = vn_sigmoid(1.702f * f);
      g = s * (1.f + 1.702f * f * (1.f - s));
    } else if (act == 3) {
      g = vn_gelu_erf_grad(f);
    } else {
      float s = vn_sigmoid(f);
      g = s * (1.f + f * (1.f - s));
    }
    o[j] = (half_t)((float)d[j] * g);
  }
  *reinterpret_cast<half8*>(dx + gid * 8) = o;
}

// Timesteps(dim, flip_sin_to_cos=True, freq_shift=0): out[b] = [cos(t f_i) | sin(t f_i)], f16
__global__ void timestep_embedding_kernel(const long long* t, half_t* out, int Bn, int dim) {
  int half_dim = dim / 2;
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= Bn * half_dim) return;
  int b = gid / half_dim, i = gid - b * half_dim;
  float f = __expf(-9.210340371976184f * (float)i / (float)half_dim);
  float e = (float)t[b] * f;
  out[(long long)b * dim + i] = (half_t)cosf(e);
  out[(long long)b * dim + half_dim + i] = (half_t)sinf(e);
}

// out[b][y][x][:] = sum of the 2x2 block of in[b][2y..][2x..][:]  (nearest-2x upsample backward)
__global__ __launch_bounds__(256) void sum2x2_kernel(const half_t* in, long long ldi, half_t* out, long long ldo,
                                                     int Bn, int H, int Wd, int cch) {
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  long long total = (long long)Bn * H * Wd * cch;
  if (gid >= total) return;
  int c = (int)(gid % cch) * 8;
  long long pix = gid / cch;
  int x = (int)(pix % Wd);
  long long t2 = pix / Wd;
  int y = (int)(t2 % H), b = (int)(t2 / H);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      long long ip = ((long long)b * 2 * H + 2 * y + dy) * (2 * Wd) + 2 * x + dx;
      half8 v = *reinterpret_cast<const half8*>(in + ip * ldi + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
    }
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (half_t)acc[j];
  vn_st16_wt(vn_make_rsrc(out, 0x7fffffffu), (uint32_t)((pix * ldo + c) * 2), o);
}

// ---- device RNG -----------------------------------------------------------------------------
// state[0] = seed, state[1] = step counter (advanced by rng_advance_kernel once per step)
__global__ void fill_normal_kernel(float* out, long long n, const uint32_t* state, uint32_t stream_id) {
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  out[gid] = rng_normal(state[0] + stream_id * 0x9E3779B9U, state[1], (uint32_t)gid);
}
__global__ void fill_randint_kernel(long long* out, int n, int high, const uint32_t* state, uint32_t stream_id) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n) return;
  uint32_t h = hash_u32((uint32_t)gid * 0x9E3779B1U + state[0] + stream_id * 0x9E3779B9U);
  h = hash_u32(h ^ (state[1] * 0x85EBCA6BU + 0x27D4EB2FU));
  out[gid] = (long long)(h % (uint32_t)high);
}
// nested dropout (models/neti_mapper.py:401-414): one Bernoulli(prob) draw per mapper call (= per UNet
// layer l); when it fires every sample b gets its own truncation index ~ U{0..hidden-1} and the
// hidden vector is zeroed from there on.  mask[(l,b)][j] = 1 if kept.
__global__ void nested_dropout_mask_kernel(float* mask, int nl, int Bn, int hidden, float prob,
                                           const uint32_t* state, uint32_t stream_id) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nl * Bn * hidden) return;
  const int j = gid % hidden, r = gid / hidden, l = r / Bn;
  const uint32_t seed = state[0] + stream_id * 0x9E3779B9U;
  uint32_t hl = hash_u32(hash_u32((uint32_t)l * 0x9E3779B1U + seed) ^ (state[1] * 0x85EBCA6BU + 0x27D4EB2FU));
  const bool fire = (float)(hl >> 8) * (1.f / 16777216.f) < prob;
  uint32_t hr = hash_u32(hash_u32((uint32_t)(r + 0x10000) * 0x9E3779B1U + seed) ^ (state[1] * 0x85EBCA6BU + 0x27D4EB2FU));
  const int idx = (int)(hr % (uint32_t)hidden);
  mask[gid] = (!fire || j < idx) ? 1.f : 0.f;
}
__global__ void rng_advance_kernel(uint32_t* state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) state[1] += 1u;
}

// ---- latent sampling + add-noise ----------------------------------------------------------------
// moments: NHWC f16 [B][h][w][2*Lc] (mean | logvar).  eps, noise: f32 [B][Lc][h][w] (NCHW, the
// layout torch.randn_like(latents) has in the reference).  Outputs (all NCHW f32):
//   latents = (mean + exp(0.5*clamp(logvar,-30,20))*eps) * scaling
//   noisy   = sqrt(ac[t]) * latents + sqrt(1-ac[t]) * noise
//   target  = noise (epsilon) or sqrt(ac)*noise - sqrt(1-ac)*latents (v_prediction)
// (the three steps are device helpers so that the split entry points below — vneti_latent_sample / vneti_add_noise, the
// module-call seam of compat/sd_modules.py — round exactly as the fused kernel does)
__device__ __forceinline__ float vn_latent_sample(const half_t* m, int c, int Lc, float eps, float scaling) {
  float mean = (float)m[c];
  float logvar = fminf(fmaxf((float)m[Lc + c], -30.f), 20.f);
  return fmaf(__expf(0.5f * logvar), eps, mean) * scaling;  // explicit fma: the same rounding in every kernel that inlines this
}
__device__ __forceinline__ void vn_add_noise(float z, float n, float a, int vpred, float& noisy, float& target) {
  float sa = sqrtf(a), sb = sqrtf(1.f - a);
  noisy = fmaf(sa, z, sb * n);
  target = vpred ? fmaf(sa, n, -(sb * z)) : n;
}

// OFFSET (the _offset entry): the noise is n' = noise + offset * offs[b][c], one draw per (sample, channel) broadcast over
// the pixels (diffusers' noise_offset); noisy and target are formed from n', the noise buffer is only read.  offset = 0
// changes no bit.  OFFSET = false is the body the plain entry always had: offs and offset are never read.
template <bool OFFSET>
__global__ void sample_add_noise_kernel(const half_t* moments, long long ldm, const float* eps,
                                        const float* noise, const long long* t, const float* ac, float scaling,
                                        int vpred, float* latents, float* noisy, float* target, int Bn, int Lc,
                                        int HW, const float* offs, float offset) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  int total = Bn * Lc * HW;
  if (gid >= total) return;
  int p = gid % HW;
  int c = (gid / HW) % Lc;
  int b = gid / (HW * Lc);
  float z = vn_latent_sample(moments + ((long long)b * HW + p) * ldm, c, Lc, eps[gid], scaling);
  float n = noise[gid];
  if constexpr (OFFSET) n = fmaf(offset, offs[b * Lc + c], n);
  float ny, tg;
  vn_add_noise(z, n, ac[t[b]], vpred, ny, tg);
  latents[gid] = z;
  noisy[gid] = ny;
  target[gid] = tg;
}

// latent_dist.sample() (* scaling) alone: AutoencoderKL.encode(x).latent_dist.sample() of the module-call seam
__global__ void latent_sample_kernel(const half_t* moments, long long ldm, const float* eps, float scaling,
                                     float* latents, int Bn, int Lc, int HW) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= Bn * Lc * HW) return;
  int p = gid % HW;
  int c = (gid / HW) % Lc;
  int b = gid / (HW * Lc);
  latents[gid] = vn_latent_sample(moments + ((long long)b * HW + p) * ldm, c, Lc, eps[gid], scaling);
}

// DDPMScheduler.add_noise / get_velocity alone (noisy and / or target may be null)
__global__ void add_noise_kernel(const float* latents, const float* noise, const long long* t, const float* ac, int vpred,
                                 float* noisy, float* target, int Bn, int Lc, int HW) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= Bn * Lc * HW) return;
  int b = gid / (HW * Lc);
  float ny, tg;
  vn_add_noise(latents[gid], noise[gid], ac[t[b]], vpred, ny, tg);
  if (noisy) noisy[gid] = ny;
  if (target) target[gid] = tg;
}

// ---- inference: classifier-free guidance + one sampler step (sd_pipeline_call.py:72-103) ---------------
// pred: NHWC f16 [2*B*HW][ldp], rows [0,B*HW) unconditional, [B*HW,2*B*HW) conditional.  x, m_prev: NCHW f32
// [B][Lc][HW].  e = u + g (c-u);  x0 = (x - sigma_t e)/alpha_t (epsilon) or alpha_t x - sigma_t e (v);
// x <- cx x + c0 x0 + c1 m_prev;  m_prev <- x0;  x_in (NCHW f32 [2B][Lc][HW], the UNet input) <- x in both halves.
__global__ void cfg_sampler_step_kernel(const half_t* pred, long long ldp, float* x, float* m_prev, float* x_in,
                                        int Bn, int Lc, int HW, float guidance, float alpha_t, float sigma_t, float cx,
                                        float c0, float c1, int vpred) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  int total = Bn * Lc * HW;
  if (gid >= total) return;
  int p = gid % HW;
  int c = (gid / HW) % Lc;
  int b = gid / (HW * Lc);
  float u = (float)pred[((long long)b * HW + p) * ldp + c];
  float cnd = (float)pred[((long long)(Bn + b) * HW + p) * ldp + c];
  float e = u + guidance * (cnd - u);
  float xv = x[gid];
  float x0 = vpred ? (alpha_t * xv - sigma_t * e) : (xv - sigma_t * e) / alpha_t;
  float xn = cx * xv + c0 * x0 + c1 * m_prev[gid];
  x[gid] = xn;
  m_prev[gid] = x0;
  x_in[gid] = xn;
  x_in[(long long)total + gid] = xn;
}
// graph-replayable variant: the per-step scalars {alpha_t, sigma_t, cx, c0, c1} come from a device table row
// selected by a device step counter, so ONE captured sampler step replays for every timestep
__global__ void cfg_sampler_step_table_kernel(const half_t* pred, long long ldp, float* x, float* m_prev, float* x_in,
                                              int Bn, int Lc, int HW, float guidance, const float* coef_table,
                                              const int* step, int vpred) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  int total = Bn * Lc * HW;
  if (gid >= total) return;
  const float* cf = coef_table + 5 * step[0];
  const float alpha_t = cf[0], sigma_t = cf[1], cx = cf[2], c0 = cf[3], c1 = cf[4];
  int p = gid % HW;
  int c = (gid / HW) % Lc;
  int b = gid / (HW * Lc);
  float u = (float)pred[((long long)b * HW + p) * ldp + c];
  float cnd = (float)pred[((long long)(Bn + b) * HW + p) * ldp + c];
  float e = u + guidance * (cnd - u);
  float xv = x[gid];
  float x0 = vpred ? (alpha_t * xv - sigma_t * e) : (xv - sigma_t * e) / alpha_t;
  float xn = cx * xv + c0 * x0 + c1 * m_prev[gid];
  x[gid] = xn;
  m_prev[gid] = x0;
  x_in[gid] = xn;
  x_in[(long long)total + gid] = xn;
}
// stochastic DDIM (eta > 0): the same step plus the scheduler's variance term,  x <- cx x + c0 x0 + c1 m_prev + cn noise,
// noise: one f32 NCHW [B][Lc][HW] row of N(0,1) draws (DDIMScheduler.step's `variance_noise`).  Each thread owns V
// consecutive pixels of one (b, c) plane: V = 4 moves x, m_prev and noise as one 16-byte load each and writes the four
// output planes with 16-byte write-through stores (the next launches, the UNet's conv_in and the next step, read them);
// V = 1 serves an HW that is no multiple of 4 or unaligned buffers.  cn == 0 returns r itself, and eta = 0 must reproduce
// cfg_sampler_step_kernel bit for bit.  The same C++ expressions do not: under the default -ffp-contract=fast the compiler
// fuses them one way there and another way here (per instantiation: V = 1 fused alpha_t x - sigma_t e into one fma, V = 4
// split c1 m_prev off into a rounded product and an add).  So contraction is off in this body and every fma of that
// kernel's ISA is written out: e = fma(g, c-u, u); x0 = fma(-sigma_t, e, x) / alpha_t (IEEE division), or
// alpha_t x - sigma_t e with both products rounded; r = fma(c1, m_prev, fma(cx, x, c0 x0)).
//
// SCALED (guidance rescale, the _scaled entries): e <- e * factor[b] as one rounded multiply of its own between the
// guidance fma and x0, factor[b] written by cfg_rescale_finish_kernel; a factor of exactly 1 changes no bit.  There `noise`
// may be null (eta = 0): nothing is loaded through it and cn is not looked at.  SCALED = false is the body as it was.
struct StepCoef {
  float alpha_t, sigma_t, cx, c0, c1, cn;
};
template <int V, bool SCALED = false>
__device__ __forceinline__ void cfg_sampler_step_noise_body(const half_t* pred, long long ldp, float* x, float* m_prev,
                                                            float* x_in, const float* noise, int Bn, int Lc, int HW,
                                                            float guidance, const StepCoef k, int vpred,
                                                            const float* factor = nullptr) {
#pragma clang fp contract(off)
  const int total = Bn * Lc * HW;
  const int gid = (blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (gid >= total) return;
  const int p = gid % HW;
  const int c = (gid / HW) % Lc;
  const int b = gid / (HW * Lc);
  float xv[V], mp[V], nz[V], x0[V], xn[V];
  if constexpr (V == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + gid);
    const f32x4 m = *reinterpret_cast<const f32x4*>(m_prev + gid);
    f32x4 n = {0.f, 0.f, 0.f, 0.f};
    if (!SCALED || noise) n = *reinterpret_cast<const f32x4*>(noise + gid);
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[j] = a[j], mp[j] = m[j], nz[j] = n[j];
  } else {
    xv[0] = x[gid], mp[0] = m_prev[gid], nz[0] = (!SCALED || noise) ? noise[gid] : 0.f;
  }
  const bool with_noise = k.cn != 0.f && (!SCALED || noise);
  float fb = 1.f;
  if constexpr (SCALED) fb = factor[b];
  const half_t* pu = pred + ((long long)b * HW + p) * ldp + c;
  const half_t* pc = pred + ((long long)(Bn + b) * HW + p) * ldp + c;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float u = (float)pu[j * ldp];
    float cnd = (float)pc[j * ldp];
    float e = fmaf(guidance, cnd - u, u);
    if constexpr (SCALED) e = e * fb;
    x0[j] = vpred ? (k.alpha_t * xv[j] - k.sigma_t * e) : fmaf(-k.sigma_t, e, xv[j]) / k.alpha_t;
    float r = fmaf(k.c1, mp[j], fmaf(k.cx, xv[j], k.c0 * x0[j]));
    xn[j] = with_noise ? fmaf(k.cn, nz[j], r) : r;
  }
  if constexpr (V == 4) {
    const f32x4 o = {xn[0], xn[1], xn[2], xn[3]}, d = {x0[0], x0[1], x0[2], x0[3]};
    const uint32_t plane = (uint32_t)total * 4u, off = (uint32_t)gid * 4u;  // launcher: 2 * plane < 2 GiB
    vn_st16_wt(vn_make_rsrc(x, plane), off, o);
    vn_st16_wt(vn_make_rsrc(m_prev, plane), off, d);
    const __amdgpu_buffer_rsrc_t ri = vn_make_rsrc(x_in, 2u * plane);
    vn_st16_wt(ri, off, o);
    vn_st16_wt(ri, plane + off, o);
  } else {
    x[gid] = xn[0];
    m_prev[gid] = x0[0];
    x_in[gid] = xn[0];
    x_in[(long long)total + gid] = xn[0];
  }
}
template <int V>
__global__ __launch_bounds__(256) void cfg_sampler_step_noise_kernel(const half_t* pred, long long ldp, float* x,
                                                                     float* m_prev, float* x_in, const float* noise,
                                                                     int Bn, int Lc, int HW, float guidance, StepCoef k,
                                                                     int vpred) {
  cfg_sampler_step_noise_body<V>(pred, ldp, x, m_prev, x_in, noise, Bn, Lc, HW, guidance, k, vpred);
}
// graph-replayable: row step[0] of the T x 6 table {alpha_t, sigma_t, cx, c0, c1, cn} and of the [T][B][Lc][HW] noise table
template <int V>
__global__ __launch_bounds__(256) void cfg_sampler_step_noise_table_kernel(const half_t* pred, long long ldp, float* x,
                                                                           float* m_prev, float* x_in, int Bn, int Lc,
                                                                           int HW, float guidance, const float* coef_table,
                                                                           const float* noise_table, const int* step,
                                                                           int vpred) {
  const int s = step[0];
  const float* cf = coef_table + 6 * s;
  const StepCoef k = {cf[0], cf[1], cf[2], cf[3], cf[4], cf[5]};
  cfg_sampler_step_noise_body<V>(pred, ldp, x, m_prev, x_in, noise_table + (long long)s * Bn * Lc * HW, Bn, Lc, HW,
                                 guidance, k, vpred);
}
// guidance rescale: the same two forms with e * factor[b]; noise / noise_table may be null
template <int V>
__global__ __launch_bounds__(256) void cfg_sampler_step_scaled_kernel(const half_t* pred, long long ldp, float* x,
                                                                      float* m_prev, float* x_in, const float* noise,
                                                                      const float* factor, int Bn, int Lc, int HW,
                                                                      float guidance, StepCoef k, int vpred) {
  cfg_sampler_step_noise_body<V, true>(pred, ldp, x, m_prev, x_in, noise, Bn, Lc, HW, guidance, k, vpred, factor);
}
template <int V>
__global__ __launch_bounds__(256) void cfg_sampler_step_scaled_table_kernel(const half_t* pred, long long ldp, float* x,
                                                                            float* m_prev, float* x_in, int Bn, int Lc,
                                                                            int HW, float guidance, const float* coef_table,
                                                                            const float* noise_table, const float* factor,
                                                                            const int* step, int vpred) {
  const int s = step[0];
  const float* cf = coef_table + 6 * s;
  const StepCoef k = {cf[0], cf[1], cf[2], cf[3], cf[4], cf[5]};
  cfg_sampler_step_noise_body<V, true>(pred, ldp, x, m_prev, x_in,
                                       noise_table ? noise_table + (long long)s * Bn * Lc * HW : nullptr, Bn, Lc, HW,
                                       guidance, k, vpred, factor);
}

// ---- guidance rescale factor (Lin et al. 2023, section 3.4; diffusers' rescale_noise_cfg) -------------------------------
// f[b] = phi * std(c[b]) / std(e[b]) + (1 - phi) over the Lc * HW elements of sample b, with the very u, c and
// e = fma(g, c - u, u) the step body above forms (contraction off here too).  Both standard deviations are centred and the
// N - 1 of both cancels, so f needs the four sums S(c), S(c^2), S(e), S(e^2) only.  They are taken in f64: the square of
// an f32 is exact in f64, so the only rounding is that of the f64 additions, and S(v^2) - S(v)^2 / N keeps ~16 digits minus
// log10(1 + mean^2 / var) (a prediction of mean 3 and deviation 1 loses one).  Two stages in a FIXED order, no float atomics
// and no "last block" counter (as mse_per_sample_kernel): block (chunk, b) owns the kRescaleChunk pixels
// [chunk * kRescaleChunk, ...) of sample b; thread t takes pixels t, t + 256, ... of the chunk, channels in order; the four
// sums go down the wave64 by shuffles (offsets 32, 16, .. 1), then lane 0 of each wave leaves them in LDS and thread 0 adds
// the waves in wave order; ws[(b * nchunk + chunk) * 4 + {0..3}] is the partial.  The finish adds a sample's partials in
// chunk order, forms the centred sums, the ratio and f in f64 and rounds ONCE to f32.  The partition depends on HW alone:
// f[b] is a function of sample b's data and (Lc, HW, g, phi), whatever Bn and wherever b sits.  A prediction whose centred
// sum of squares of e is not positive (a constant e[b]) gets f = 1, where diffusers divides by zero.
// VEC: Lc == 4, ldp % 4 == 0 and an 8-byte aligned base: the four channels of a pixel are one 8-byte load per CFG half.
constexpr int kRescaleChunk = 512;
template <bool VEC>
__global__ __launch_bounds__(256) void cfg_rescale_partial_kernel(const half_t* __restrict__ pred, long long ldp,
                                                                  double* __restrict__ ws, int Bn, int Lc, int HW,
                                                                  int nchunk, float guidance) {
#pragma clang fp contract(off)
  __shared__ double red[4][4];
  const int chunk = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};  // S(c), S(c^2), S(e), S(e^2)
#pragma unroll
  for (int j = 0; j < kRescaleChunk / 256; ++j) {
    const int p = chunk * kRescaleChunk + j * 256 + t;
    if (p < HW) {
      const half_t* pu = pred + ((long long)b * HW + p) * ldp;
      const half_t* pc = pred + ((long long)(Bn + b) * HW + p) * ldp;
      if constexpr (VEC) {
        const half4 u4 = *reinterpret_cast<const half4*>(pu);
        const half4 c4 = *reinterpret_cast<const half4*>(pc);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float u = (float)u4[c], cnd = (float)c4[c];
          const double cd = (double)cnd, ed = (double)fmaf(guidance, cnd - u, u);
          s[0] += cd, s[1] += cd * cd, s[2] += ed, s[3] += ed * ed;
        }
      } else {
        for (int c = 0; c < Lc; ++c) {
          const float u = (float)pu[c], cnd = (float)pc[c];
          const double cd = (double)cnd, ed = (double)fmaf(guidance, cnd - u, u);
          s[0] += cd, s[1] += cd * cd, s[2] += ed, s[3] += ed * ed;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[t >> 6][k] = s[k];
  }
  __syncthreads();
  if (t < 4) ws[((long long)b * nchunk + chunk) * 4 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}
__global__ __launch_bounds__(256) void cfg_rescale_finish_kernel(const double* __restrict__ ws, int Bn, int nchunk,
                                                                 double n_elem, float rescale, float* __restrict__ factor) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= Bn) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < nchunk; ++k) {
    const double* w = ws + ((long long)b * nchunk + k) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += w[q];
  }
  const double ss_c = s[1] - s[0] * s[0] / n_elem, ss_e = s[3] - s[2] * s[2] / n_elem;
  const double phi = (double)rescale;
  double f = 1.0;
  if (ss_e > 0.0) f = phi * sqrt(fmax(ss_c, 0.0) / ss_e) + (1.0 - phi);
  factor[b] = (float)f;
}
__global__ void table_fill_i64_kernel(long long* dst, int n, const long long* table, const int* step) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid < n) dst[gid] = table[step[0]];
}
__global__ void counter_advance_kernel(int* c) {
  if (threadIdx.x == 0 && blockIdx.x == 0) c[0] += 1;
}
// tiny 1x1 conv on NCHW f32 latents (AutoencoderKL.post_quant_conv after the 1/scaling_factor of
// pipeline.decode_latents): out[b][o][p] = bias[o] + sum_c W[o][c] * x[b][c][p] * in_scale,  C <= 8
__global__ void conv1x1_nchw_kernel(const float* x, const float* W, const float* bias, float* out, int Bn, int Ci,
                                    int Co, int HW, float in_scale) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= Bn * Co * HW) return;
  int p = gid % HW;
  int o = (gid / HW) % Co;
  int b = gid / (HW * Co);
  float acc = bias ? bias[o] : 0.f;
  for (int c = 0; c < Ci; ++c) acc += W[o * Ci + c] * x[((long long)b * Ci + c) * HW + p] * in_scale;
  out[gid] = acc;
}
// decoder output NHWC f16 [B*HW][ldi] (3 channels) -> (v/2 + 0.5).clamp(0,1) as f32 [B][HW][3]
// (pipeline.decode_latents, sd_pipeline_call.py:115)
__global__ void image_postprocess_kernel(const half_t* img, long long ldi, float* out, long long n_pix, int ch) {
  long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n_pix * ch) return;
  long long p = gid / ch;
  int c = (int)(gid - p * ch);
  float v = (float)img[p * ldi + c] * 0.5f + 0.5f;
  out[gid] = fminf(fmaxf(v, 0.f), 1.f);
}

// ---- MSE loss + gradient seed -------------------------------------------------------------------
// pred: NHWC f16 [B*HW][ldp] (Lc channels used); target NCHW f32.  loss_sum += sum (p-t)^2 (one
// atomic per block); dpred (NHWC f16) = 2*(p-t)/N * loss_scale[0].
// SNR (the _snr entry): sample b's terms are multiplied by the Min-SNR-gamma weight w_b of its timestep (diffusers
// compute_snr: snr = ac/(1-ac); w = min(snr, gamma)/snr, or /(snr+1) for v-prediction), computed here in f32 —
// always, also when w is 1 (then it changes no bit).  SNR = false is the body the unweighted entry always had: t, ac,
// gamma and vpred are never read.
// WQ (the _weighted entry): one more factor per latent pixel, q[b][p] (f32 [Bn][HW], the normalised object
// mask of vneti_loss_weights_from_mask): the term's weight is w_b * q_bp — q_bp alone without SNR — one rounded f32
// product, also when q is 1 (then it changes no bit against the entry without q).  WQ = false never reads q: the two
// bodies above are the ones the kernel always had.
template <bool SNR, bool WQ = false>
__global__ __launch_bounds__(256) void mse_loss_grad_kernel(const half_t* pred, long long ldp, const float* target,
                                                            half_t* dpred, long long lddp, float* loss_sum,
                                                            const float* loss_scale, int Bn, int Lc, int HW,
                                                            const long long* t, const float* ac, float gamma,
                                                            int vpred, const float* q) {
  __shared__ float red[4];
  int gid = blockIdx.x * 256 + threadIdx.x;
  int total = Bn * Lc * HW;
  float sq = 0.f;
  if (gid < total) {
    int c = gid % Lc;
    int p = (gid / Lc) % HW;
    int b = gid / (Lc * HW);
    float pv = (float)pred[((long long)b * HW + p) * ldp + c];
    float tv = target[((long long)b * Lc + c) * HW + p];
    float d = pv - tv;
    if constexpr (WQ) {
      float w = q[(long long)b * HW + p];
      if constexpr (SNR) {
        float a = ac[t[b]];
        float snr = a / (1.f - a);
        w = fminf(snr, gamma) / (vpred ? snr + 1.f : snr) * w;
      }
      sq = d * d * w;
      dpred[((long long)b * HW + p) * lddp + c] = (half_t)(2.f * d * w / (float)total * loss_scale[0]);
    } else if constexpr (SNR) {
      float a = ac[t[b]];
      float snr = a / (1.f - a);
      float w = fminf(snr, gamma) / (vpred ? snr + 1.f : snr);
      sq = d * d * w;
      dpred[((long long)b * HW + p) * lddp + c] = (half_t)(2.f * d * w / (float)total * loss_scale[0]);
    } else {
      sq = d * d;
      dpred[((long long)b * HW + p) * lddp + c] = (half_t)(2.f * d / (float)total * loss_scale[0]);
    }
  }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss_sum, red[0] + red[1] + red[2] + red[3]);
}

// ---- per-sample MSE, forward only (held-out evaluation) -----------------------------------------
// The same layouts as mse_loss_grad_kernel; out[b] = mean over (c, p) of (pred - target)^2 of sample b alone.  Two stages in a
// FIXED order, no float atomics (as lpips_dist_kernel / lpips_dist_finish_kernel): block (chunk, b) owns the kMseChunk pixels
// [chunk * kMseChunk, ...) of sample b — one pixel per thread, its Lc channels summed in channel order, then the LDS tree —
// and writes ws[b * nchunk + chunk]; the finish adds a sample's partials in chunk order in f64.  The partition depends on
// (Lc, HW) only, never on Bn or on b: a sample's value is bit-identical wherever it sits in whatever batch.  A non-finite
// element poisons the partial of its own sample only.
constexpr int kMseChunk = 256;
__global__ __launch_bounds__(kMseChunk) void mse_per_sample_kernel(const half_t* __restrict__ pred, long long ldp,
                                                                   const float* __restrict__ target, float* __restrict__ ws,
                                                                   int Lc, int HW, int nchunk) {
  __shared__ float red[kMseChunk];
  const int b = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
  const int p = chunk * kMseChunk + t;
  float acc = 0.f;
  if (p < HW) {
    const half_t* pr = pred + ((long long)b * HW + p) * ldp;
    const float* tg = target + (long long)b * Lc * HW + p;
    for (int c = 0; c < Lc; ++c) {
      const float d = (float)pr[c] - tg[(long long)c * HW];
      acc = fmaf(d, d, acc);
    }
  }
  red[t] = acc;
  __syncthreads();
#pragma unroll
  for (int s = kMseChunk / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) ws[(long long)b * nchunk + chunk] = red[0];
}
// The weighted sibling: the pixel's channel sum, formed exactly as above, times q[b][p] — one rounded f32
// product, so q == 1 leaves every partial, and with the shared finish every out[b], bit-identical to the kernel above.
// The same blocks, the same tree, the same workspace: out[b] = sum_{c,p} q_bp d^2 / (Lc HW).
__global__ __launch_bounds__(kMseChunk) void mse_per_sample_weighted_kernel(const half_t* __restrict__ pred, long long ldp,
                                                                            const float* __restrict__ target,
                                                                            const float* __restrict__ q,
                                                                            float* __restrict__ ws, int Lc, int HW,
                                                                            int nchunk) {
  __shared__ float red[kMseChunk];
  const int b = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
  const int p = chunk * kMseChunk + t;
  float acc = 0.f;
  if (p < HW) {
    const half_t* pr = pred + ((long long)b * HW + p) * ldp;
    const float* tg = target + (long long)b * Lc * HW + p;
    for (int c = 0; c < Lc; ++c) {
      const float d = (float)pr[c] - tg[(long long)c * HW];
      acc = fmaf(d, d, acc);
    }
    acc *= q[(long long)b * HW + p];
  }
  red[t] = acc;
  __syncthreads();
#pragma unroll
  for (int s = kMseChunk / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) ws[(long long)b * nchunk + chunk] = red[0];
}
__global__ __launch_bounds__(256) void mse_per_sample_finish_kernel(const float* __restrict__ ws, int Bn, int nchunk,
                                                                    double inv_n, float* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= Bn) return;
  double s = 0.0;
  for (int k = 0; k < nchunk; ++k) s += (double)ws[(long long)b * nchunk + k];
  out[b] = (float)(s * inv_n);
}

// ---- AdamW over a flat f32 bucket with torch.cuda.amp.GradScaler semantics ---------------------
// scaler[0] = loss scale, scaler[1] = growth tracker, scaler[2] = found_inf (this step),
// hyper: lr, beta1, beta2, eps, weight_decay, grad_div (= world size for DP mean)
__global__ __launch_bounds__(256) void grads_check_finite_kernel(const float* g, long long n, float* scaler) {
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (gid < n) {
    float v = g[gid];
    bad = !(v == v) || fabsf(v) == INFINITY;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) scaler[2] = 1.f;
}
// CLIP (the _clipped entries): the unscaled gradient is multiplied by clip[0], torch.nn.utils.clip_grad_norm_'s
// `g.mul_(clip_coef_clamped)` — always, also when the coefficient is 1 (then it changes no bit).  CLIP = false is the body
// the unclipped entries always had: `clip` is never read.
template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_kernel(float* p, const float* g, float* m, float* v, long long n,
                                                    const float* hyper, const float* scaler, const int* step,
                                                    const float* clip) {
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  if (scaler[2] != 0.f) return;  // GradScaler.step(): skip the update when grads are non-finite
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], gdiv = hyper[5];
  const int t = step[0] + 1;
  float grad = g[gid] / (scaler[0] * gdiv);
  if constexpr (CLIP) grad *= clip[0];
  float pv = p[gid] * (1.f - lr * wd);
  float mv = b1 * m[gid] + (1.f - b1) * grad;
  float vv = b2 * v[gid] + (1.f - b2) * grad * grad;
  float bc1 = 1.f - powf(b1, (float)t), bc2 = 1.f - powf(b2, (float)t);
  float denom = sqrtf(vv) / sqrtf(bc2) + eps;
  p[gid] = pv - (lr / bc1) * mv / denom;
  m[gid] = mv;
  v[gid] = vv;
}
// AdamW over a bucket of equal-length segments (one per mapper) with torch's per-parameter state:
// a segment joins the update set the first time it receives a gradient (grad None -> skipped,
// torch/optim/adamw.py) and from then on is stepped every iteration, with a zero gradient when it
// was not in the batch (zero_grad() keeps zero tensors in torch 1.13), each with its own `step`.
template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_segments_kernel(float* p, const float* g, float* m, float* v,
                                                             long long n, long long seg_len, const int* seg_step,
                                                             const int* active, int n_active, const float* hyper,
                                                             const float* scaler, const float* clip) {
  long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  if (scaler[2] != 0.f) return;
  const int seg = (int)(gid / seg_len);
  bool is_active = false;
  for (int i = 0; i < n_active; ++i) is_active |= active[i] == seg;
  const int t0 = seg_step[seg];
  if (t0 == 0 && !is_active) return;  // never had a gradient: not in the optimizer's update set yet
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], gdiv = hyper[5];
  const int t = t0 + 1;
  float grad = is_active ? g[gid] / (scaler[0] * gdiv) : 0.f;
  if constexpr (CLIP) grad *= clip[0];
  float pv = p[gid] * (1.f - lr * wd);
  float mv = b1 * m[gid] + (1.f - b1) * grad;
  float vv = b2 * v[gid] + (1.f - b2) * grad * grad;
  float bc1 = 1.f - powf(b1, (float)t), bc2 = 1.f - powf(b2, (float)t);
  float denom = sqrtf(vv) / sqrtf(bc2) + eps;
  p[gid] = pv - (lr / bc1) * mv / denom;
  m[gid] = mv;
  v[gid] = vv;
}
__global__ void segments_step_kernel(int* seg_step, int n_seg, const int* active, int n_active, const float* scaler) {
  int seg = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= n_seg || scaler[2] != 0.f) return;
  bool is_active = false;
  for (int i = 0; i < n_active; ++i) is_active |= active[i] == seg;
  if (seg_step[seg] > 0 || is_active) seg_step[seg] += 1;
}
// finite check restricted to the active segments (the others hold stale or zero gradients)
__global__ __launch_bounds__(256) void grads_check_finite_segments_kernel(const float* g, long long seg_len,
                                                                          const int* active, float* scaler) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < seg_len) {
    float x = g[(long long)active[blockIdx.y] * seg_len + i];
    bad = !(x == x) || fabsf(x) == INFINITY;  // torch's isfinite, as grads_check_finite_kernel: 3.2e38 is a finite gradient
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) scaler[2] = 1.f;
}
// GradScaler.update(): backoff 0.5 on inf, growth x2 every `interval` clean steps; advance step.
// growth_interval <= 0: a STATIC scale (the bf16 branch: accelerate creates no GradScaler there) — a non-finite step is
// still skipped, but the scale neither backs off nor grows
__global__ void scaler_update_kernel(float* scaler, int* step, int growth_interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (growth_interval <= 0) {
    if (scaler[2] == 0.f) step[0] += 1;
  } else if (scaler[2] != 0.f) {
    scaler[0] *= 0.5f;
    scaler[1] = 0.f;
  } else {
    step[0] += 1;
    scaler[1] += 1.f;
    if ((int)scaler[1] >= growth_interval) {
      scaler[0] *= 2.f;
      scaler[1] = 0.f;
    }
  }
  scaler[2] = 0.f;
}

// ---- gradient norm (clipping, per-step record) --------------------------------------------------
// Sum of squares of an f32 gradient bucket in two stages, in a FIXED order and without float atomics (as
// mse_per_sample_kernel): block (chunk, s) owns the kGradChunk floats [chunk * kGradChunk, ...) of segment s — the flat
// range when `active` is null, else segment active[s] of length `len` (grads_check_finite_segments_kernel's addressing) —
// thread t adds the squares of elements t, t + 256, ... in that order, then the LDS tree; ws[s * nchunk + chunk] is the
// partial.  Squares and sums are f64: (3.4e38)^2 = 1.2e77 is a finite double, so the total is non-finite exactly when an
// element is.  Scalar loads: the view mapper's range starts wherever the object mappers end, no alignment holds.  The
// bucket is ~0.5 MiB per mapper: the launch is the cost, not the bytes.
constexpr int kGradChunk = 4096;
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long len,
                                                         const int* __restrict__ active, double* __restrict__ ws,
                                                         int nchunk) {
  __shared__ double red[256];
  const int chunk = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
  const float* base = g + (active ? (long long)active[s] * len : 0LL);
  const long long lo = (long long)chunk * kGradChunk;
  double acc = 0.0;
#pragma unroll 4
  for (int j = 0; j < kGradChunk / 256; ++j) {
    const long long i = lo + j * 256 + t;
    if (i < len) {
      const double x = (double)base[i];
      acc = fma(x, x, acc);
    }
  }
  red[t] = acc;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) ws[(long long)s * nchunk + chunk] = red[0];
}
// One block: the partials of the object side, then of the view side, added in index order in f64 (either side may be
// absent: its norm reads -1).  out = {norm_object, norm_view, norm_total, finite, clip_coef}, norms of the UNSCALED mean
// gradient: sqrt(sum) / (scaler[0] * hyper[5]).  clip_coef = min(1, max_norm / (norm_total + 1e-6)) in f32, torch's
// clip_grad_norm_; exactly 1 when max_norm[0] <= 0 (clipping off) or the sum is non-finite (the step is skipped anyway).
// ring (optional): the same values, the loss scale and the lr go into the row of the micro-step that closed the group,
// (count[0] - 1) % rows, with its "closed a group" flag.
__global__ __launch_bounds__(64) void grad_norm_finish_kernel(const double* __restrict__ ws_o, int n_o,
                                                              const double* __restrict__ ws_v, int n_v,
                                                              const float* __restrict__ scaler,
                                                              const float* __restrict__ hyper,
                                                              const float* __restrict__ max_norm, float* __restrict__ out,
                                                              float* __restrict__ ring, const int* __restrict__ count,
                                                              int rows, int row_floats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double so = 0.0, sv = 0.0;
  for (int k = 0; k < n_o; ++k) so += ws_o[k];
  for (int k = 0; k < n_v; ++k) sv += ws_v[k];
  const double tot = so + sv;
  const float scale = scaler[0];
  const double div = (double)(scale * hyper[5]);
  const float no = n_o > 0 ? (float)(sqrt(so) / div) : -1.f;
  const float nv = n_v > 0 ? (float)(sqrt(sv) / div) : -1.f;
  const float nt = (float)(sqrt(tot) / div);
  const bool finite = tot == tot && tot != (double)INFINITY;
  const float mx = max_norm[0];
  float coef = 1.f;
  if (finite && mx > 0.f) coef = fminf(1.f, mx / (nt + 1e-6f));
  out[0] = no;
  out[1] = nv;
  out[2] = nt;
  out[3] = finite ? 1.f : 0.f;
  out[4] = coef;
  if (ring) {
    const int c = count[0];
    if (c > 0) {
      float* row = ring + (long long)((unsigned)(c - 1) % (unsigned)rows) * row_floats;
      row[VNETI_TELEMETRY_CLOSED] = 1.f;
      row[VNETI_TELEMETRY_NORM_OBJECT] = no;
      row[VNETI_TELEMETRY_NORM_VIEW] = nv;
      row[VNETI_TELEMETRY_NORM_TOTAL] = nt;
      row[VNETI_TELEMETRY_FINITE] = finite ? 1.f : 0.f;
      row[VNETI_TELEMETRY_CLIP_COEF] = coef;
      row[VNETI_TELEMETRY_LOSS_SCALE] = scale;
      row[VNETI_TELEMETRY_LR] = hyper[0];
    }
  }
}
// The micro-step's part of ring row count[0] % rows: sequence number (count mod 2^24, exact in f32: a reader tells the
// laps of the ring apart by it), micro index (0 when `first`, else the previous row's + 1), a cleared "closed a group"
// part, the Bn timesteps and per-sample losses.  Then count[0] += 1.  One block; every thread reads the counter before the
// barrier, thread 0 advances it after.
__global__ __launch_bounds__(256) void train_record_kernel(float* __restrict__ ring, int* __restrict__ count, int rows,
                                                           int row_floats, int first, const long long* __restrict__ t,
                                                           const float* __restrict__ losses, int Bn) {
  const int c = count[0];
  const unsigned r = (unsigned)c % (unsigned)rows, rp = (unsigned)(c + rows - 1) % (unsigned)rows;
  float* row = ring + (long long)r * row_floats;
  const float prev_micro = ring[(long long)rp * row_floats + VNETI_TELEMETRY_MICRO];
  __syncthreads();  // rows == 1: the previous row is this one
  for (int i = threadIdx.x; i < VNETI_TELEMETRY_HEADER; i += 256) {
    float x = 0.f;
    if (i == VNETI_TELEMETRY_SEQ) x = (float)(c & 0xFFFFFF);
    if (i == VNETI_TELEMETRY_MICRO) x = first ? 0.f : prev_micro + 1.f;
    row[i] = x;
  }
  for (int b = threadIdx.x; b < Bn; b += 256) {
    row[VNETI_TELEMETRY_HEADER + b] = (float)t[b];
    row[VNETI_TELEMETRY_HEADER + Bn + b] = losses[b];
  }
  __syncthreads();
  if (threadIdx.x == 0) count[0] = c + 1;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vneti_add_f16(const void* a, long long lda, const void* b, long long ldb, void* out, long long ldo,
                             int rows, int cols, void* stream) {
  VN_REQUIRE(a && b && out && rows > 0 && cols > 0 && cols % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldo % 8 == 0,
             "add_f16: bad arguments");
  VN_REQUIRE_OUT("add_f16", vn_out_bytes(rows, ldo, cols, 2));
  long long n = (long long)rows * (cols / 8);
  hipLaunchKernelGGL(add_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST, (const half_t*)a, lda,
                     (const half_t*)b, ldb, (half_t*)out, ldo, rows, cols / 8);
  return vneti_check_launch("add_f16");
}

extern "C" int vneti_geglu_fwd(const void* p, long long ldp, void* out, long long ldo, int rows, int C4,
                               void* stream) {
  VN_REQUIRE(p && out && rows > 0 && C4 > 0 && C4 % 8 == 0 && ldp % 8 == 0 && ldo % 8 == 0, "geglu_fwd: bad arguments");
  long long n = (long long)rows * (C4 / 8);
  hipLaunchKernelGGL(geglu_fwd_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST, (const half_t*)p, ldp,
                     (half_t*)out, ldo, rows, C4);
  return vneti_check_launch("geglu_fwd");
}

extern "C" int vneti_geglu_bwd(const void* dy, long long lddy, const void* p, long long ldp, void* dp,
                               long long lddp, int rows, int C4, void* stream) {
  VN_REQUIRE(dy && p && dp && rows > 0 && C4 > 0 && C4 % 8 == 0 && ldp % 8 == 0 && lddy % 8 == 0 && lddp % 8 == 0,
             "geglu_bwd: bad arguments");
  long long n = (long long)rows * (C4 / 8);
  hipLaunchKernelGGL(geglu_bwd_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST, (const half_t*)dy, lddy,
                     (const half_t*)p, ldp, (half_t*)dp, lddp, rows, C4);
  return vneti_check_launch("geglu_bwd");
}

extern "C" int vneti_act_fwd_f16(const void* x, void* y, long long n, int act, void* stream) {
  VN_REQUIRE(x && y && n > 0 && n % 8 == 0 && act >= 1 && act <= 3, "act_fwd: bad arguments");
  hipLaunchKernelGGL(act_fwd_kernel, dim3((unsigned)cdivl(n / 8, 256)), dim3(256), 0, ST, (const half_t*)x,
                     (half_t*)y, n / 8, act);
  return vneti_check_launch("act_fwd");
}

extern "C" int vneti_act_bwd_f16(const void* dy, const void* x, void* dx, long long n, int act, void* stream) {
  VN_REQUIRE(dy && x && dx && n > 0 && n % 8 == 0 && act >= 1 && act <= 3, "act_bwd: bad arguments");
  hipLaunchKernelGGL(act_bwd_kernel, dim3((unsigned)cdivl(n / 8, 256)), dim3(256), 0, ST, (const half_t*)dy,
                     (const half_t*)x, (half_t*)dx, n / 8, act);
  return vneti_check_launch("act_bwd");
}

extern "C" int vneti_timestep_embedding(const void* t, void* out, int Bn, int dim, void* stream) {
  VN_REQUIRE(t && out && Bn > 0 && dim > 0 && dim % 2 == 0, "timestep_embedding: bad arguments");
  int n = Bn * dim / 2;
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, (const long long*)t,
                     (half_t*)out, Bn, dim);
  return vneti_check_launch("timestep_embedding");
}

extern "C" int vneti_sum2x2_f16(const void* in, long long ldi, void* out, long long ldo, int Bn, int H, int W,
                                int C, void* stream) {
  VN_REQUIRE(in && out && Bn > 0 && H > 0 && W > 0 && C % 8 == 0 && ldi % 8 == 0 && ldo % 8 == 0,
             "sum2x2: bad arguments");
  VN_REQUIRE_OUT("sum2x2", vn_out_bytes((long long)Bn * H * W, ldo, C, 2));
  long long n = (long long)Bn * H * W * (C / 8);
  hipLaunchKernelGGL(sum2x2_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST, (const half_t*)in, ldi,
                     (half_t*)out, ldo, Bn, H, W, C / 8);
  return vneti_check_launch("sum2x2");
}

extern "C" int vneti_rng_fill_normal(void* out, long long n, const void* state, unsigned stream_id, void* stream) {
  VN_REQUIRE(out && state && n > 0 && n < 0xffffffffLL, "rng_fill_normal: bad arguments");
  hipLaunchKernelGGL(fill_normal_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST, (float*)out, n,
                     (const uint32_t*)state, stream_id);
  return vneti_check_launch("rng_fill_normal");
}

extern "C" int vneti_rng_fill_randint(void* out, int n, int high, const void* state, unsigned stream_id,
                                      void* stream) {
  VN_REQUIRE(out && state && n > 0 && high > 0, "rng_fill_randint: bad arguments");
  hipLaunchKernelGGL(fill_randint_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, (long long*)out, n, high,
                     (const uint32_t*)state, stream_id);
  return vneti_check_launch("rng_fill_randint");
}

extern "C" int vneti_nested_dropout_mask(float* mask, int nl, int Bn, int hidden, float prob, const void* state,
                                         unsigned stream_id, void* stream) {
  VN_REQUIRE(mask && state && nl > 0 && Bn > 0 && hidden > 0 && prob >= 0.f && prob <= 1.f,
             "nested_dropout_mask: bad arguments");
  int n = nl * Bn * hidden;
  hipLaunchKernelGGL(nested_dropout_mask_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, mask, nl, Bn, hidden, prob,
                     (const uint32_t*)state, (uint32_t)stream_id);
  return vneti_check_launch("nested_dropout_mask");
}

extern "C" int vneti_rng_advance(void* state, void* stream) {
  VN_REQUIRE(state, "rng_advance: null state");
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(64), 0, ST, (uint32_t*)state);
  return vneti_check_launch("rng_advance");
}

extern "C" int vneti_sample_add_noise(const void* moments, long long ldm, const float* eps, const float* noise,
                                      const void* timesteps, const float* alphas_cumprod, float scaling,
                                      int v_prediction, float* latents, float* noisy, float* target, int Bn,
                                      int Lc, int HW, void* stream) {
  VN_REQUIRE(moments && eps && noise && timesteps && alphas_cumprod && latents && noisy && target,
             "sample_add_noise: null pointer");
  int n = Bn * Lc * HW;
  hipLaunchKernelGGL(sample_add_noise_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, ST, (const half_t*)moments, ldm,
                     eps, noise, (const long long*)timesteps, alphas_cumprod, scaling, v_prediction, latents, noisy,
                     target, Bn, Lc, HW, (const float*)nullptr, 0.f);
  return vneti_check_launch("sample_add_noise");
}

extern "C" int vneti_sample_add_noise_offset(const void* moments, long long ldm, const float* eps, const float* noise,
                                             const void* timesteps, const float* alphas_cumprod, float scaling,
                                             int v_prediction, float* latents, float* noisy, float* target, int Bn,
                                             int Lc, int HW, const float* offs, float offset, void* stream) {
  VN_REQUIRE(moments && eps && noise && timesteps && alphas_cumprod && latents && noisy && target && offs,
             "sample_add_noise_offset: null pointer");
  VN_REQUIRE(Bn > 0 && Lc > 0 && HW > 0 && ldm >= 2LL * Lc && (long long)Bn * Lc * HW < 0x7fffffffLL,
             "sample_add_noise_offset: bad shape Bn=%d Lc=%d HW=%d ldm=%lld", Bn, Lc, HW, ldm);
  int n = Bn * Lc * HW;
  hipLaunchKernelGGL(sample_add_noise_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, ST, (const half_t*)moments, ldm,
                     eps, noise, (const long long*)timesteps, alphas_cumprod, scaling, v_prediction, latents, noisy,
                     target, Bn, Lc, HW, offs, offset);
  return vneti_check_launch("sample_add_noise_offset");
}

extern "C" int vneti_latent_sample(const void* moments, long long ldm, const float* eps, float scaling, float* latents,
                                   int Bn, int Lc, int HW, void* stream) {
  VN_REQUIRE(moments && eps && latents && Bn > 0 && Lc > 0 && HW > 0, "latent_sample: bad arguments");
  int n = Bn * Lc * HW;
  hipLaunchKernelGGL(latent_sample_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, (const half_t*)moments, ldm, eps, scaling,
                     latents, Bn, Lc, HW);
  return vneti_check_launch("latent_sample");
}

extern "C" int vneti_add_noise(const float* latents, const float* noise, const void* timesteps_i64,
                               const float* alphas_cumprod, int v_prediction, float* noisy, float* target, int Bn, int Lc,
                               int HW, void* stream) {
  VN_REQUIRE(latents && noise && timesteps_i64 && alphas_cumprod && (noisy || target) && Bn > 0 && Lc > 0 && HW > 0,
             "add_noise: bad arguments");
  int n = Bn * Lc * HW;
  hipLaunchKernelGGL(add_noise_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, latents, noise,
                     (const long long*)timesteps_i64, alphas_cumprod, v_prediction, noisy, target, Bn, Lc, HW);
  return vneti_check_launch("add_noise");
}

extern "C" int vneti_cfg_sampler_step(const void* pred, long long ldp, float* x, float* m_prev, float* x_in, int Bn,
                                      int Lc, int HW, float guidance, float alpha_t, float sigma_t, float cx, float c0,
                                      float c1, int v_prediction, void* stream) {
  VN_REQUIRE(pred && x && m_prev && x_in && Bn > 0 && Lc > 0 && HW > 0 && alpha_t > 0.f,
             "cfg_sampler_step: bad arguments");
  int n = Bn * Lc * HW;
  hipLaunchKernelGGL(cfg_sampler_step_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, (const half_t*)pred, ldp, x,
                     m_prev, x_in, Bn, Lc, HW, guidance, alpha_t, sigma_t, cx, c0, c1, v_prediction);
  return vneti_check_launch("cfg_sampler_step");
}

extern "C" int vneti_cfg_sampler_step_table(const void* pred, long long ldp, float* x, float* m_prev, float* x_in,
                                            int Bn, int Lc, int HW, float guidance, const float* coef_table,
                                            const int* step, int v_prediction, void* stream) {
  VN_REQUIRE(pred && x && m_prev && x_in && coef_table && step && Bn > 0 && Lc > 0 && HW > 0,
             "cfg_sampler_step_table: bad arguments");
  int n = Bn * Lc * HW;
  hipLaunchKernelGGL(cfg_sampler_step_table_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, (const half_t*)pred, ldp, x,
                     m_prev, x_in, Bn, Lc, HW, guidance, coef_table, step, v_prediction);
  return vneti_check_launch("cfg_sampler_step_table");
}

// 16-byte path: whole float4 groups inside one (b, c) plane and 16-byte aligned f32 buffers (any torch allocation is)
static bool step_noise_vec4(int HW, const void* x, const void* m_prev, const void* x_in, const void* noise) {
  return HW % 4 == 0 && (((uintptr_t)x | (uintptr_t)m_prev | (uintptr_t)x_in | (uintptr_t)noise) & 15u) == 0;
}

extern "C" int vneti_cfg_sampler_step_noise(const void* pred, long long ldp, float* x, float* m_prev, float* x_in,
                                            const float* noise, int Bn, int Lc, int HW, float guidance, float alpha_t,
                                            float sigma_t, float cx, float c0, float c1, float cn, int v_prediction,
                                            void* stream) {
  VN_REQUIRE(pred && x && m_prev && x_in && noise && Bn > 0 && Lc > 0 && HW > 0 && alpha_t > 0.f,
             "cfg_sampler_step_noise: bad arguments");
  const long long n = (long long)Bn * Lc * HW;
  VN_REQUIRE_OUT("cfg_sampler_step_noise (x_in)", 2 * n * 4);
  const StepCoef k = {alpha_t, sigma_t, cx, c0, c1, cn};
  if (step_noise_vec4(HW, x, m_prev, x_in, noise))
    hipLaunchKernelGGL(cfg_sampler_step_noise_kernel<4>, dim3(cdiv((int)(n / 4), 256)), dim3(256), 0, ST,
                       (const half_t*)pred, ldp, x, m_prev, x_in, noise, Bn, Lc, HW, guidance, k, v_prediction);
  else
    hipLaunchKernelGGL(cfg_sampler_step_noise_kernel<1>, dim3(cdiv((int)n, 256)), dim3(256), 0, ST, (const half_t*)pred,
                       ldp, x, m_prev, x_in, noise, Bn, Lc, HW, guidance, k, v_prediction);
  return vneti_check_launch("cfg_sampler_step_noise");
}

extern "C" int vneti_cfg_sampler_step_noise_table(const void* pred, long long ldp, float* x, float* m_prev, float* x_in,
                                                  int Bn, int Lc, int HW, float guidance, const float* coef_table,
                                                  const float* noise_table, const int* step, int v_prediction,
                                                  void* stream) {
  VN_REQUIRE(pred && x && m_prev && x_in && coef_table && noise_table && step && Bn > 0 && Lc > 0 && HW > 0,
             "cfg_sampler_step_noise_table: bad arguments");
  const long long n = (long long)Bn * Lc * HW;
  VN_REQUIRE_OUT("cfg_sampler_step_noise_table (noise_table row)", n * 4);
  VN_REQUIRE_OUT("cfg_sampler_step_noise_table (x_in)", 2 * n * 4);
  if (step_noise_vec4(HW, x, m_prev, x_in, noise_table))
    hipLaunchKernelGGL(cfg_sampler_step_noise_table_kernel<4>, dim3(cdiv((int)(n / 4), 256)), dim3(256), 0, ST,
                       (const half_t*)pred, ldp, x, m_prev, x_in, Bn, Lc, HW, guidance, coef_table, noise_table, step,
                       v_prediction);
  else
    hipLaunchKernelGGL(cfg_sampler_step_noise_table_kernel<1>, dim3(cdiv((int)n, 256)), dim3(256), 0, ST,
                       (const half_t*)pred, ldp, x, m_prev, x_in, Bn, Lc, HW, guidance, coef_table, noise_table, step,
                       v_prediction);
  return vneti_check_launch("cfg_sampler_step_noise_table");
}

extern "C" long long vneti_cfg_rescale_ws_doubles(int Bn, int HW) {
  if (Bn <= 0 || HW <= 0) return -1;
  return 4LL * Bn * cdiv(HW, kRescaleChunk);
}

extern "C" int vneti_cfg_rescale_factor(const void* pred, long long ldp, float* factor, void* ws, int Bn, int Lc, int HW,
                                        float guidance, float rescale, void* stream) {
  VN_REQUIRE(pred && factor && ws, "cfg_rescale_factor: null pointer");
  VN_REQUIRE(Bn > 0 && Bn <= 65535 && Lc > 0 && HW > 0 && ldp >= Lc,
             "cfg_rescale_factor: bad shape Bn=%d Lc=%d HW=%d ldp=%lld (0 < Bn <= 65535, ldp >= Lc)", Bn, Lc, HW, ldp);
  VN_REQUIRE((long long)Bn * Lc * HW < 0x7fffffffLL, "cfg_rescale_factor: Bn * Lc * HW over 2^31");
  VN_REQUIRE(((uintptr_t)ws & 7u) == 0, "cfg_rescale_factor: ws must be 8-byte aligned");
  VN_REQUIRE(rescale >= 0.f && rescale <= 1.f, "cfg_rescale_factor: rescale = %g outside [0, 1]", (double)rescale);
  const int nchunk = cdiv(HW, kRescaleChunk);
  if (Lc == 4 && ldp % 4 == 0 && ((uintptr_t)pred & 7u) == 0)
    hipLaunchKernelGGL(cfg_rescale_partial_kernel<true>, dim3(nchunk, Bn), dim3(256), 0, ST, (const half_t*)pred, ldp,
                       (double*)ws, Bn, Lc, HW, nchunk, guidance);
  else
    hipLaunchKernelGGL(cfg_rescale_partial_kernel<false>, dim3(nchunk, Bn), dim3(256), 0, ST, (const half_t*)pred, ldp,
                       (double*)ws, Bn, Lc, HW, nchunk, guidance);
  const int rc = vneti_check_launch("cfg_rescale_factor");
  if (rc != VNETI_OK) return rc;
  hipLaunchKernelGGL(cfg_rescale_finish_kernel, dim3(cdiv(Bn, 256)), dim3(256), 0, ST, (const double*)ws, Bn, nchunk,
                     (double)Lc * (double)HW, rescale, factor);
  return vneti_check_launch("cfg_rescale_factor_finish");
}

extern "C" int vneti_cfg_sampler_step_scaled(const void* pred, long long ldp, float* x, float* m_prev, float* x_in,
                                             const float* noise, const float* factor, int Bn, int Lc, int HW,
                                             float guidance, float alpha_t, float sigma_t, float cx, float c0, float c1,
                                             float cn, int v_prediction, void* stream) {
  VN_REQUIRE(pred && x && m_prev && x_in && factor && Bn > 0 && Lc > 0 && HW > 0 && ldp >= Lc && alpha_t > 0.f,
             "cfg_sampler_step_scaled: bad arguments");
  const long long n = (long long)Bn * Lc * HW;
  VN_REQUIRE_OUT("cfg_sampler_step_scaled (x_in)", 2 * n * 4);
  const StepCoef k = {alpha_t, sigma_t, cx, c0, c1, cn};
  if (step_noise_vec4(HW, x, m_prev, x_in, noise))
    hipLaunchKernelGGL(cfg_sampler_step_scaled_kernel<4>, dim3(cdiv((int)(n / 4), 256)), dim3(256), 0, ST,
                       (const half_t*)pred, ldp, x, m_prev, x_in, noise, factor, Bn, Lc, HW, guidance, k, v_prediction);
  else
    hipLaunchKernelGGL(cfg_sampler_step_scaled_kernel<1>, dim3(cdiv((int)n, 256)), dim3(256), 0, ST, (const half_t*)pred,
                       ldp, x, m_prev, x_in, noise, factor, Bn, Lc, HW, guidance, k, v_prediction);
  return vneti_check_launch("cfg_sampler_step_scaled");
}

extern "C" int vneti_cfg_sampler_step_scaled_table(const void* pred, long long ldp, float* x, float* m_prev, float* x_in,
                                                   int Bn, int Lc, int HW, float guidance, const float* coef_table,
                                                   const float* noise_table, const float* factor, const int* step,
                                                   int v_prediction, void* stream) {
  VN_REQUIRE(pred && x && m_prev && x_in && coef_table && factor && step && Bn > 0 && Lc > 0 && HW > 0 && ldp >= Lc,
             "cfg_sampler_step_scaled_table: bad arguments");
  const long long n = (long long)Bn * Lc * HW;
  VN_REQUIRE_OUT("cfg_sampler_step_scaled_table (noise_table row)", n * 4);
  VN_REQUIRE_OUT("cfg_sampler_step_scaled_table (x_in)", 2 * n * 4);
  if (step_noise_vec4(HW, x, m_prev, x_in, noise_table))
    hipLaunchKernelGGL(cfg_sampler_step_scaled_table_kernel<4>, dim3(cdiv((int)(n / 4), 256)), dim3(256), 0, ST,
                       (const half_t*)pred, ldp, x, m_prev, x_in, Bn, Lc, HW, guidance, coef_table, noise_table, factor,
                       step, v_prediction);
  else
    hipLaunchKernelGGL(cfg_sampler_step_scaled_table_kernel<1>, dim3(cdiv((int)n, 256)), dim3(256), 0, ST,
                       (const half_t*)pred, ldp, x, m_prev, x_in, Bn, Lc, HW, guidance, coef_table, noise_table, factor,
                       step, v_prediction);
  return vneti_check_launch("cfg_sampler_step_scaled_table");
}

extern "C" int vneti_table_fill_i64(void* dst, int n, const void* table, const int* step, void* stream) {
  VN_REQUIRE(dst && table && step && n > 0, "table_fill_i64: bad arguments");
  hipLaunchKernelGGL(table_fill_i64_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, (long long*)dst, n,
                     (const long long*)table, step);
  return vneti_check_launch("table_fill_i64");
}

extern "C" int vneti_counter_advance(int* counter, void* stream) {
  VN_REQUIRE(counter, "counter_advance: null pointer");
  hipLaunchKernelGGL(counter_advance_kernel, dim3(1), dim3(64), 0, ST, counter);
  return vneti_check_launch("counter_advance");
}

extern "C" int vneti_conv1x1_nchw_f32(const float* x, const float* W, const float* bias, float* out, int Bn, int Ci,
                                      int Co, int HW, float in_scale, void* stream) {
  VN_REQUIRE(x && W && out && Bn > 0 && Ci > 0 && Ci <= 8 && Co > 0 && Co <= 8 && HW > 0, "conv1x1_nchw: bad arguments");
  int n = Bn * Co * HW;
  hipLaunchKernelGGL(conv1x1_nchw_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, x, W, bias, out, Bn, Ci, Co, HW,
                     in_scale);
  return vneti_check_launch("conv1x1_nchw");
}

extern "C" int vneti_image_postprocess(const void* img, long long ldi, float* out, long long n_pix, int channels,
                                       void* stream) {
  VN_REQUIRE(img && out && n_pix > 0 && channels > 0 && channels <= ldi, "image_postprocess: bad arguments");
  hipLaunchKernelGGL(image_postprocess_kernel, dim3((unsigned)cdivl(n_pix * channels, 256)), dim3(256), 0, ST,
                     (const half_t*)img, ldi, out, n_pix, channels);
  return vneti_check_launch("image_postprocess");
}

extern "C" int vneti_mse_loss_grad(const void* pred, long long ldp, const float* target, void* dpred,
                                   long long lddp, float* loss_sum, const float* loss_scale, int Bn, int Lc,
                                   int HW, void* stream) {
  VN_REQUIRE(pred && target && dpred && loss_sum && loss_scale, "mse_loss_grad: null pointer");
  int n = Bn * Lc * HW;
  hipLaunchKernelGGL(mse_loss_grad_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, ST, (const half_t*)pred, ldp, target,
                     (half_t*)dpred, lddp, loss_sum, loss_scale, Bn, Lc, HW, (const long long*)nullptr,
                     (const float*)nullptr, 0.f, 0, (const float*)nullptr);
  return vneti_check_launch("mse_loss_grad");
}

extern "C" int vneti_mse_loss_grad_snr(const void* pred, long long ldp, const float* target, void* dpred,
                                       long long lddp, float* loss_sum, const float* loss_scale, int Bn, int Lc,
                                       int HW, const void* timesteps, const float* alphas_cumprod, float gamma,
                                       int v_prediction, void* stream) {
  VN_REQUIRE(pred && target && dpred && loss_sum && loss_scale && timesteps && alphas_cumprod,
             "mse_loss_grad_snr: null pointer");
  VN_REQUIRE(Bn > 0 && Lc > 0 && HW > 0 && ldp >= Lc && lddp >= Lc && (long long)Bn * Lc * HW < 0x7fffffffLL,
             "mse_loss_grad_snr: bad shape Bn=%d Lc=%d HW=%d ldp=%lld lddp=%lld", Bn, Lc, HW, ldp, lddp);
  VN_REQUIRE(gamma > 0.f, "mse_loss_grad_snr: gamma must be > 0 (+inf: every weight is 1)");
  int n = Bn * Lc * HW;
  hipLaunchKernelGGL(mse_loss_grad_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, ST, (const half_t*)pred, ldp, target,
                     (half_t*)dpred, lddp, loss_sum, loss_scale, Bn, Lc, HW, (const long long*)timesteps,
                     alphas_cumprod, gamma, v_prediction, (const float*)nullptr);
  return vneti_check_launch("mse_loss_grad_snr");
}

extern "C" int vneti_mse_loss_grad_weighted(const void* pred, long long ldp, const float* target, void* dpred,
                                            long long lddp, float* loss_sum, const float* loss_scale, const float* q,
                                            int Bn, int Lc, int HW, const void* timesteps, const float* alphas_cumprod,
                                            float gamma, int v_prediction, void* stream) {
  VN_REQUIRE(pred && target && dpred && loss_sum && loss_scale && q, "mse_loss_grad_weighted: null pointer");
  VN_REQUIRE((timesteps == nullptr) == (alphas_cumprod == nullptr),
             "mse_loss_grad_weighted: timesteps and alphas_cumprod come as a pair (both null: no Min-SNR factor)");
  VN_REQUIRE(Bn > 0 && Lc > 0 && HW > 0 && ldp >= Lc && lddp >= Lc && (long long)Bn * Lc * HW < 0x7fffffffLL,
             "mse_loss_grad_weighted: bad shape Bn=%d Lc=%d HW=%d ldp=%lld lddp=%lld", Bn, Lc, HW, ldp, lddp);
  VN_REQUIRE((long long)Bn * HW * ldp * 2 < 0x7fffffffLL && (long long)Bn * HW * lddp * 2 < 0x7fffffffLL,
             "mse_loss_grad_weighted: pred / dpred span 2 GiB or more (Bn=%d HW=%d ldp=%lld lddp=%lld)", Bn, HW, ldp, lddp);
  int n = Bn * Lc * HW;
  if (timesteps) {
    VN_REQUIRE(gamma > 0.f, "mse_loss_grad_weighted: gamma must be > 0 (+inf: every Min-SNR weight is 1)");
    hipLaunchKernelGGL((mse_loss_grad_kernel<true, true>), dim3(cdiv(n, 256)), dim3(256), 0, ST, (const half_t*)pred, ldp,
                       target, (half_t*)dpred, lddp, loss_sum, loss_scale, Bn, Lc, HW, (const long long*)timesteps,
                       alphas_cumprod, gamma, v_prediction, q);
  } else {
    hipLaunchKernelGGL((mse_loss_grad_kernel<false, true>), dim3(cdiv(n, 256)), dim3(256), 0, ST, (const half_t*)pred, ldp,
                       target, (half_t*)dpred, lddp, loss_sum, loss_scale, Bn, Lc, HW, (const long long*)nullptr,
                       (const float*)nullptr, 0.f, 0, q);
  }
  return vneti_check_launch("mse_loss_grad_weighted");
}

extern "C" long long vneti_mse_loss_per_sample_ws_floats(int Bn, int HW) {
  if (Bn <= 0 || HW <= 0) return -1;
  return (long long)Bn * cdiv(HW, kMseChunk);
}

extern "C" int vneti_mse_loss_per_sample(const void* pred, long long ldp, const float* target, float* out, float* ws,
                                         int Bn, int Lc, int HW, void* stream) {
  VN_REQUIRE(pred && target && out && ws, "mse_loss_per_sample: null pointer");
  VN_REQUIRE(Bn > 0 && Bn <= 65535 && Lc > 0 && HW > 0 && ldp >= Lc,
             "mse_loss_per_sample: bad shape Bn=%d Lc=%d HW=%d ldp=%lld (0 < Bn <= 65535, ldp >= Lc)", Bn, Lc, HW, ldp);
  VN_REQUIRE((long long)Bn * Lc * HW < 0x7fffffffLL, "mse_loss_per_sample: Bn * Lc * HW over 2^31");
  const int nchunk = cdiv(HW, kMseChunk);
  hipLaunchKernelGGL(mse_per_sample_kernel, dim3(nchunk, Bn), dim3(kMseChunk), 0, ST, (const half_t*)pred, ldp, target, ws,
                     Lc, HW, nchunk);
  const int rc = vneti_check_launch("mse_loss_per_sample");
  if (rc != VNETI_OK) return rc;
  hipLaunchKernelGGL(mse_per_sample_finish_kernel, dim3(cdiv(Bn, 256)), dim3(256), 0, ST, (const float*)ws, Bn, nchunk,
                     1.0 / ((double)Lc * (double)HW), out);
  return vneti_check_launch("mse_loss_per_sample_finish");
}

extern "C" int vneti_mse_loss_per_sample_weighted(const void* pred, long long ldp, const float* target, const float* q,
                                                  float* out, float* ws, int Bn, int Lc, int HW, void* stream) {
  VN_REQUIRE(pred && target && q && out && ws, "mse_loss_per_sample_weighted: null pointer");
  VN_REQUIRE(Bn > 0 && Bn <= 65535 && Lc > 0 && HW > 0 && ldp >= Lc,
             "mse_loss_per_sample_weighted: bad shape Bn=%d Lc=%d HW=%d ldp=%lld (0 < Bn <= 65535, ldp >= Lc)", Bn, Lc, HW,
             ldp);
  VN_REQUIRE((long long)Bn * Lc * HW < 0x7fffffffLL, "mse_loss_per_sample_weighted: Bn * Lc * HW over 2^31");
  VN_REQUIRE((long long)Bn * HW * ldp * 2 < 0x7fffffffLL,
             "mse_loss_per_sample_weighted: pred spans 2 GiB or more (Bn=%d HW=%d ldp=%lld)", Bn, HW, ldp);
  const int nchunk = cdiv(HW, kMseChunk);
  hipLaunchKernelGGL(mse_per_sample_weighted_kernel, dim3(nchunk, Bn), dim3(kMseChunk), 0, ST, (const half_t*)pred, ldp,
                     target, q, ws, Lc, HW, nchunk);
  const int rc = vneti_check_launch("mse_loss_per_sample_weighted");
  if (rc != VNETI_OK) return rc;
  hipLaunchKernelGGL(mse_per_sample_finish_kernel, dim3(cdiv(Bn, 256)), dim3(256), 0, ST, (const float*)ws, Bn, nchunk,
                     1.0 / ((double)Lc * (double)HW), out);
  return vneti_check_launch("mse_loss_per_sample_finish");
}

static int adamw_segments_launch(const char* what, float* p, const float* g, float* m, float* v, long long seg_len,
                                 int n_seg, int* seg_step, const int* active, int n_active, const float* hyper,
                                 float* scaler, int* step, int growth_interval, int phases, const float* clip,
                                 void* stream) {
  const long long n = seg_len * n_seg;
  if (phases & 1)
    hipLaunchKernelGGL(grads_check_finite_segments_kernel, dim3((unsigned)cdivl(seg_len, 256), n_active), dim3(256),
                       0, ST, g, seg_len, active, scaler);
  if (phases & 2) {
    if (clip)
      hipLaunchKernelGGL(adamw_segments_kernel<true>, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST, p, g, m, v, n,
                         seg_len, (const int*)seg_step, active, n_active, hyper, (const float*)scaler, clip);
    else
      hipLaunchKernelGGL(adamw_segments_kernel<false>, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST, p, g, m, v, n,
                         seg_len, (const int*)seg_step, active, n_active, hyper, (const float*)scaler,
                         (const float*)nullptr);
    hipLaunchKernelGGL(segments_step_kernel, dim3(cdiv(n_seg, 256)), dim3(256), 0, ST, seg_step, n_seg, active,
                       n_active, (const float*)scaler);
  }
  if (phases & 4) hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, ST, scaler, step, growth_interval);
  return vneti_check_launch(what);
}

extern "C" int vneti_adamw_segments(float* p, const float* g, float* m, float* v, long long seg_len, int n_seg,
                                    int* seg_step, const int* active, int n_active, const float* hyper,
                                    float* scaler, int* step, int growth_interval, int phases, void* stream) {
  VN_REQUIRE(p && g && m && v && hyper && scaler && step && seg_step && active && seg_len > 0 && n_seg > 0 &&
                 n_active > 0 && n_active <= 8 && phases > 0 && phases < 8,
             "adamw_segments: bad arguments");
  return adamw_segments_launch("adamw_segments", p, g, m, v, seg_len, n_seg, seg_step, active, n_active, hyper, scaler,
                               step, growth_interval, phases, nullptr, stream);
}

extern "C" int vneti_adamw_segments_clipped(float* p, const float* g, float* m, float* v, long long seg_len, int n_seg,
                                            int* seg_step, const int* active, int n_active, const float* hyper,
                                            float* scaler, int* step, int growth_interval, int phases,
                                            const float* clip_coef, void* stream) {
  VN_REQUIRE(p && g && m && v && hyper && scaler && step && seg_step && active && clip_coef && seg_len > 0 && n_seg > 0 &&
                 n_active > 0 && n_active <= 8 && phases > 0 && phases < 8,
             "adamw_segments_clipped: bad arguments");
  return adamw_segments_launch("adamw_segments_clipped", p, g, m, v, seg_len, n_seg, seg_step, active, n_active, hyper,
                               scaler, step, growth_interval, phases, clip_coef, stream);
}

static int adamw_flat_launch(const char* what, float* p, const float* g, float* m, float* v, long long n,
                             const float* hyper, float* scaler, int* step, int growth_interval, int phases,
                             const float* clip, void* stream) {
  unsigned blocks = (unsigned)cdivl(n, 256);
  if (phases & 1) hipLaunchKernelGGL(grads_check_finite_kernel, dim3(blocks), dim3(256), 0, ST, g, n, scaler);
  if (phases & 2) {
    if (clip)
      hipLaunchKernelGGL(adamw_kernel<true>, dim3(blocks), dim3(256), 0, ST, p, g, m, v, n, hyper, (const float*)scaler,
                         (const int*)step, clip);
    else
      hipLaunchKernelGGL(adamw_kernel<false>, dim3(blocks), dim3(256), 0, ST, p, g, m, v, n, hyper, (const float*)scaler,
                         (const int*)step, (const float*)nullptr);
  }
  if (phases & 4) hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, ST, scaler, step, growth_interval);
  return vneti_check_launch(what);
}

extern "C" int vneti_adamw_flat(float* p, const float* g, float* m, float* v, long long n, const float* hyper,
                                float* scaler, int* step, int growth_interval, int phases, void* stream) {
  VN_REQUIRE(p && g && m && v && hyper && scaler && step && n > 0 && phases > 0 && phases < 8,
             "adamw_flat: bad arguments");
  return adamw_flat_launch("adamw_flat", p, g, m, v, n, hyper, scaler, step, growth_interval, phases, nullptr, stream);
}

extern "C" int vneti_adamw_flat_clipped(float* p, const float* g, float* m, float* v, long long n, const float* hyper,
                                        float* scaler, int* step, int growth_interval, int phases, const float* clip_coef,
                                        void* stream) {
  VN_REQUIRE(p && g && m && v && hyper && scaler && step && clip_coef && n > 0 && phases > 0 && phases < 8,
             "adamw_flat_clipped: bad arguments");
  return adamw_flat_launch("adamw_flat_clipped", p, g, m, v, n, hyper, scaler, step, growth_interval, phases, clip_coef,
                           stream);
}

extern "C" long long vneti_grad_sumsq_ws_doubles(long long len, int n_active) {
  if (len <= 0 || n_active < 0 || n_active > 8 || cdivl(len, kGradChunk) > 0x7fffffLL) return -1;
  return cdivl(len, kGradChunk) * (n_active > 0 ? n_active : 1);
}

extern "C" int vneti_grad_sumsq(const float* g, long long len, const int* active, int n_active, void* ws, void* stream) {
  VN_REQUIRE(g && ws && len > 0, "grad_sumsq: bad arguments");
  VN_REQUIRE(active ? (n_active > 0 && n_active <= 8) : n_active == 0,
             "grad_sumsq: n_active=%d (1..8 segment ids with `active`, 0 for the flat range without)", n_active);
  const long long nchunk = cdivl(len, kGradChunk);
  VN_REQUIRE(nchunk <= 0x7fffffLL, "grad_sumsq: %lld floats is more than one launch covers", len);
  VN_REQUIRE(((uintptr_t)ws & 7u) == 0, "grad_sumsq: the f64 workspace must be 8-byte aligned");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nchunk, active ? n_active : 1), dim3(256), 0, ST, g, len, active,
                     (double*)ws, (int)nchunk);
  return vneti_check_launch("grad_sumsq");
}

extern "C" int vneti_grad_norm_finish(const void* ws_object, long long n_object, const void* ws_view, long long n_view,
                                      const float* scaler, const float* hyper, const float* max_norm, float* out,
                                      float* ring, const int* count, int rows, int row_floats, void* stream) {
  VN_REQUIRE(scaler && hyper && max_norm && out && n_object >= 0 && n_view >= 0 && n_object + n_view > 0 &&
                 n_object < 0x7fffffffLL && n_view < 0x7fffffffLL && (n_object == 0 || ws_object) && (n_view == 0 || ws_view),
             "grad_norm_finish: bad arguments");
  VN_REQUIRE(!ring || (count && rows > 0 && row_floats >= VNETI_TELEMETRY_HEADER),
             "grad_norm_finish: a telemetry ring needs its counter, rows > 0 and row_floats >= %d", VNETI_TELEMETRY_HEADER);
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(64), 0, ST, (const double*)ws_object, (int)n_object,
                     (const double*)ws_view, (int)n_view, scaler, hyper, max_norm, out, ring, count, rows, row_floats);
  return vneti_check_launch("grad_norm_finish");
}

extern "C" int vneti_train_record(float* ring, int* count, int rows, int row_floats, int first_micro,
                                  const void* timesteps_i64, const float* losses, int Bn, void* stream) {
  VN_REQUIRE(ring && count && timesteps_i64 && losses && rows > 0 && Bn > 0, "train_record: bad arguments");
  VN_REQUIRE(row_floats == VNETI_TELEMETRY_HEADER + 2 * Bn, "train_record: row_floats=%d, a row of Bn=%d samples has %d",
             row_floats, Bn, VNETI_TELEMETRY_HEADER + 2 * Bn);
  hipLaunchKernelGGL(train_record_kernel, dim3(1), dim3(256), 0, ST, ring, count, rows, row_floats, first_micro,
                     (const long long*)timesteps_i64, losses, Bn);
  return vneti_check_launch("train_record");
}

// ---- exponential moving average of the trained bucket (extension: optim.ema_decay) --------------
// Two launches in stream order, the idiom of adamw_flat_launch with scaler_update_kernel.  prepare (one thread) decides from
// device scalars whether the optimizer step before it was applied (`opt_step` advances on applied steps only,
// scaler_update_kernel) and, if so, this update's decay: diffusers' EMAModel.get_decay with inv_gamma 1 and min_decay 0,
// restated from the published code, in f64.  coef = {one_minus_decay, apply}: apply 0 = nothing to do (skipped step),
// 1 = the update, 2 = decay exactly 0, a bit copy (e + 1 * (p - e) is not p in f32).
__global__ void ema_prepare_kernel(const int* opt_step, int* count, const float* hyper, float* coef) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int cur = opt_step[0];
  if (cur == count[1]) {  // skipped on found_inf: neither the count nor the average moves
    coef[1] = 0.f;
    return;
  }
  const long long k = (long long)count[0] + 1;
  const long long after = (long long)hyper[1];
  const long long s = k - after - 1 > 0 ? k - after - 1 : 0;
  const double max_decay = (double)hyper[0], power = (double)hyper[2];
  double d = 0.0;
  if (s > 0) d = power == 0.0 ? (1.0 + (double)s) / (10.0 + (double)s) : 1.0 - pow(1.0 + (double)s, -power);
  d = fmin(d, max_decay);
  d = fmax(d, 0.0);
  coef[0] = (float)(1.0 - d);
  coef[1] = d == 0.0 ? 2.f : 1.f;
  count[0] = (int)k;
  count[1] = cur;
}
// The flat ranges are split at the FIRST operand's 16-byte boundaries into a head of 0..3 floats, 16-byte vectors and a tail
// of 0..3 floats; the second operand's vectors are loaded (stored) as one 16-byte access when it happens to share that
// alignment and as four dwords when it does not (a uniform branch).  Nothing but 4-byte alignment is assumed of either.
// Plain 64-bit pointers: no buffer resource, no 2 GiB bound.  Thread gid owns vector gid; threads 0..2 also own the edges.
struct FlatSplit {
  long long head, nvec, tail;
};
__device__ __forceinline__ FlatSplit flat_split(const void* first, long long n) {
  FlatSplit s;
  s.head = (long long)(((16u - (unsigned)((uintptr_t)first & 15u)) & 15u) >> 2);
  if (s.head > n) s.head = n;
  s.nvec = (n - s.head) >> 2;
  s.tail = n - s.head - 4 * s.nvec;
  return s;
}
__device__ __forceinline__ uint4 ld4_u32(const uint32_t* q, bool aligned) {
  if (aligned) return *reinterpret_cast<const uint4*>(q);
  return make_uint4(q[0], q[1], q[2], q[3]);
}
__device__ __forceinline__ void st4_u32(uint32_t* q, uint4 v, bool aligned) {
  if (aligned) {
    *reinterpret_cast<uint4*>(q) = v;
  } else {
    q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
  }
}
__device__ __forceinline__ uint32_t ema_one(uint32_t e, uint32_t q, float c, bool copy) {
  if (copy) return q;  // the bits of p: NaN payloads and -0.0 included
  const float ef = __uint_as_float(e), qf = __uint_as_float(q);
  return __float_as_uint(fmaf(c, qf - ef, ef));  // diffusers: s_param.sub_(one_minus_decay * (s_param - param))
}
__global__ __launch_bounds__(256) void ema_apply_kernel(uint32_t* __restrict__ ema, const uint32_t* __restrict__ p,
                                                        long long n, const float* __restrict__ coef) {
  const float mode = coef[1];
  if (mode == 0.f) return;
  const float c = coef[0];
  const bool copy = mode == 2.f;
  const FlatSplit sp = flat_split(ema, n);
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid < sp.nvec) {
    const long long i = sp.head + 4 * gid;
    const bool p_al = ((uintptr_t)(p + sp.head) & 15u) == 0;
    const uint4 e = *reinterpret_cast<const uint4*>(ema + i);
    const uint4 q = ld4_u32(p + i, p_al);
    *reinterpret_cast<uint4*>(ema + i) = make_uint4(ema_one(e.x, q.x, c, copy), ema_one(e.y, q.y, c, copy),
                                                    ema_one(e.z, q.z, c, copy), ema_one(e.w, q.w, c, copy));
  }
  if (gid < sp.head) ema[gid] = ema_one(ema[gid], p[gid], c, copy);
  if (gid < sp.tail) {
    const long long i = sp.head + 4 * sp.nvec + gid;
    ema[i] = ema_one(ema[i], p[i], c, copy);
  }
}
// a[i] <-> b[i], bit for bit, each element read and written by one thread: no temporary
__global__ __launch_bounds__(256) void swap_u32_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, long long n) {
  const FlatSplit sp = flat_split(a, n);
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid < sp.nvec) {
    const long long i = sp.head + 4 * gid;
    const bool b_al = ((uintptr_t)(b + sp.head) & 15u) == 0;
    const uint4 x = *reinterpret_cast<const uint4*>(a + i);
    const uint4 y = ld4_u32(b + i, b_al);
    *reinterpret_cast<uint4*>(a + i) = y;
    st4_u32(b + i, x, b_al);
  }
  if (gid < sp.head) {
    const uint32_t x = a[gid];
    a[gid] = b[gid];
    b[gid] = x;
  }
  if (gid < sp.tail) {
    const long long i = sp.head + 4 * sp.nvec + gid;
    const uint32_t x = a[i];
    a[i] = b[i];
    b[i] = x;
  }
}
// blocks of 256 threads, one per 16-byte vector of a range of n floats at any alignment (at least one: the edges)
static inline long long flat_blocks(long long n) { return cdivl(n / 4 + 1, 256); }

extern "C" int vneti_ema_update(float* ema, const float* p, long long n, const int* opt_step, int* ema_count,
                                const float* ema_hyper, float* ema_coef, void* stream) {
  VN_REQUIRE(ema && p && opt_step && ema_count && ema_hyper && ema_coef && n > 0, "ema_update: bad arguments");
  VN_REQUIRE((((uintptr_t)ema | (uintptr_t)p) & 3u) == 0, "ema_update: ema and p must be 4-byte aligned");
  VN_REQUIRE(ema + n <= p || p + n <= ema, "ema_update: ema and p overlap");
  VN_REQUIRE(flat_blocks(n) <= 0x7fffffffLL, "ema_update: %lld floats is more than one launch covers", n);
  hipLaunchKernelGGL(ema_prepare_kernel, dim3(1), dim3(64), 0, ST, opt_step, ema_count, ema_hyper, ema_coef);
  hipLaunchKernelGGL(ema_apply_kernel, dim3((unsigned)flat_blocks(n)), dim3(256), 0, ST, (uint32_t*)ema,
                     (const uint32_t*)p, n, (const float*)ema_coef);
  return vneti_check_launch("ema_update");
}

extern "C" int vneti_swap_f32(float* a, float* b, long long n, void* stream) {
  VN_REQUIRE(a && b && n > 0, "swap_f32: bad arguments");
  VN_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3u) == 0, "swap_f32: a and b must be 4-byte aligned");
  VN_REQUIRE(a + n <= b || b + n <= a, "swap_f32: the ranges overlap");
  VN_REQUIRE(flat_blocks(n) <= 0x7fffffffLL, "swap_f32: %lld floats is more than one launch covers", n);
  hipLaunchKernelGGL(swap_u32_kernel, dim3((unsigned)flat_blocks(n)), dim3(256), 0, ST, (uint32_t*)a, (uint32_t*)b, n);
  return vneti_check_launch("swap_f32");
}
