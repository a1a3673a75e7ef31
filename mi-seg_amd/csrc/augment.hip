// Free rotation / zoom, gamma contrast and Gaussian noise on the resident-volume augmenter (include/miseg_hip.h: miseg_augment_affine; DESIGN.md
// section 7.11).  One gather pass per batch, as augment_kernel of training.hip: 256 threads, a grid-stride loop over the patch voxels with W
// fastest (coalesced stores), blockIdx.z = the sample, the per-sample descriptors in the kernel arguments.
//   crop -> affine resample about the crop centre -> flip 0, 1, 2 -> rot90 (aug_source inverts the last two); image: -> gamma ->
//   fma(v, 1 + scale, shift) -> noise.  Every operation is rounded on its own (contraction is off for the whole file) except that one explicit
//   fused multiply-add, which is what augment_kernel's `v * mul + shift` compiles to: an identity sample carries that kernel's bits.
//   Gamma needs the sample's minimum and maximum first: the resample launch stores the raw values of such a sample and reduces them (wave
//   shuffles -> LDS -> one integer atomicMax per workgroup on an order-preserving code), a second launch finishes those samples in place.
//   Samples without gamma are finished by the first launch.  Plain vector loads and stores, integer atomics on the 16-byte scratch row of a
//   sample only; no float atomics.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace miseg {

struct AffArgs {
  int C, D, H, W, rd, rh, rw, n, pad;
  uint64_t key;                    // dropout_host_key(seed, draw)
  miseg_aug_affine_sample s[MISEG_AUG_MAX_SAMPLES];
};
static_assert(sizeof(AffArgs) + 64 < 4096, "the descriptors travel in the kernel arguments");

// order-preserving code of a float: a < b  <=>  code(a) < code(b) as unsigned
__device__ __forceinline__ uint32_t float_code(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float code_float(uint32_t c) { return __uint_as_float((c & 0x80000000u) ? (c & 0x7fffffffu) : ~c); }

__device__ __forceinline__ uint64_t noise_sample_key(uint64_t key, int sample) { return mix64(key ^ ((uint64_t)sample * 0x9E3779B97F4A7C15ull)); }
// Box-Muller from one hash: u1 = bits 63..40 (+ 1: in (0, 1]), u2 = bits 39..16
__device__ __forceinline__ float noise_z(uint64_t ks, int64_t e) {
  const uint64_t h = mix64(ks + (uint64_t)e * 0xD1342543DE82EF95ull);
  const float u1 = (float)((uint32_t)(h >> 40) + 1u) * 0x1p-24f;
  const float u2 = (float)((uint32_t)(h >> 16) & 0xffffffu) * 0x1p-24f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// what follows gamma: v * (1 + scale) + shift as ONE fma (augment_kernel's expression is contracted to one), then the noise of element e
__device__ __forceinline__ float aug_finish(float v, float mul, float shift, bool noisy, float nmean, float nstd, uint64_t ks, int64_t e) {
  v = fmaf(v, mul, shift);
  if (noisy) v = v + (nmean + nstd * noise_z(ks, e));
  return v;
}

__device__ __forceinline__ bool aug_is_identity(const miseg_aug_affine_sample& s) {
  return s.m[0] == 1.f && s.m[1] == 0.f && s.m[2] == 0.f && s.m[3] == 0.f && s.m[4] == 1.f && s.m[5] == 0.f && s.m[6] == 0.f && s.m[7] == 0.f &&
         s.m[8] == 1.f && s.t[0] == 0.f && s.t[1] == 0.f && s.t[2] == 0.f;
}

// floor(s) as an index, held in [-2, n + 1]: everything out there is padding either way (and a NaN cannot reach the conversion)
__device__ __forceinline__ int floor_index(float fl, int n) { return (int)fminf(fmaxf(fl, -2.f), (float)n + 1.f); }
__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

template <class LB>
static __global__ void __launch_bounds__(256) augment_affine_kernel(const float* __restrict__ image, const LB* __restrict__ label, float* __restrict__ oimg,
                                                                     LB* __restrict__ olab, uint32_t* __restrict__ minmax, AffArgs a) {
  const int n = blockIdx.z;
  const miseg_aug_affine_sample& sm = a.s[n];
  const int64_t pvol = (int64_t)a.rd * a.rh * a.rw, vvol = (int64_t)a.D * a.H * a.W;
  const float mul = 1.f + sm.scale;
  const bool identity = aug_is_identity(sm), defer = sm.gamma > 0.f, noisy = sm.noise_std > 0.f, zeros = a.pad == MISEG_AUG_PAD_ZEROS;
  const uint64_t ks = noisy ? noise_sample_key(a.key, n) : 0ull;
  const float c0 = 0.5f * (float)(a.rd - 1), c1 = 0.5f * (float)(a.rh - 1), c2 = 0.5f * (float)(a.rw - 1);
  const float b0 = (float)sm.origin[0] + c0, b1 = (float)sm.origin[1] + c1, b2 = (float)sm.origin[2] + c2;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < pvol; o += (int64_t)gridDim.x * 256) {
    const int k = (int)(o % a.rw), j = (int)((o / a.rw) % a.rh), i = (int)(o / ((int64_t)a.rw * a.rh));
    int si, sj, sk;
    aug_source(sm, a.rd, a.rh, a.rw, i, j, k, si, sj, sk);
    float* dst = oimg + (int64_t)n * a.C * pvol + o;
    if (identity) {
      const int64_t src = ((int64_t)(sm.origin[0] + si) * a.H + (sm.origin[1] + sj)) * a.W + (sm.origin[2] + sk);
      for (int c = 0; c < a.C; ++c) {
        float v = image[(int64_t)c * vvol + src];
        if (defer) { v = v + 0.f; mn = fminf(mn, v); mx = fmaxf(mx, v); }
        else v = aug_finish(v, mul, sm.shift, noisy, sm.noise_mean, sm.noise_std, ks, (int64_t)c * pvol + o);
        dst[(int64_t)c * pvol] = v;
      }
      if (label) olab[(int64_t)n * pvol + o] = label[src];
      continue;
    }
    const float d0 = (float)si - c0, d1 = (float)sj - c1, d2 = (float)sk - c2;
    const float s0 = (((sm.m[0] * d0 + sm.m[1] * d1) + sm.m[2] * d2) + sm.t[0]) + b0;
    const float s1 = (((sm.m[3] * d0 + sm.m[4] * d1) + sm.m[5] * d2) + sm.t[1]) + b1;
    const float s2 = (((sm.m[6] * d0 + sm.m[7] * d1) + sm.m[8] * d2) + sm.t[2]) + b2;
    const float l0 = floorf(s0), l1 = floorf(s1), l2 = floorf(s2);
    const float f0 = s0 - l0, f1 = s1 - l1, f2 = s2 - l2;
    const int i0 = floor_index(l0, a.D), j0 = floor_index(l1, a.H), k0 = floor_index(l2, a.W);
    // the 8 neighbours: in-volume flags (zeros mode drops the others) and clamped indices (always safe to read)
    const bool vi[2] = {i0 >= 0 && i0 < a.D, i0 + 1 >= 0 && i0 + 1 < a.D};
    const bool vj[2] = {j0 >= 0 && j0 < a.H, j0 + 1 >= 0 && j0 + 1 < a.H};
    const bool vk[2] = {k0 >= 0 && k0 < a.W, k0 + 1 >= 0 && k0 + 1 < a.W};
    const int64_t ri[2] = {(int64_t)clampi(i0, a.D) * a.H * a.W, (int64_t)clampi(i0 + 1, a.D) * a.H * a.W};
    const int64_t rj[2] = {(int64_t)clampi(j0, a.H) * a.W, (int64_t)clampi(j0 + 1, a.H) * a.W};
    const int rk[2] = {clampi(k0, a.W), clampi(k0 + 1, a.W)};
    for (int c = 0; c < a.C; ++c) {
      const float* img = image + (int64_t)c * vvol;
      float x[2][2][2];
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const float t = img[ri[p] + rj[q] + rk[r]];
            x[p][q][r] = (!zeros || (vi[p] && vj[q] && vk[r])) ? t : 0.f;
          }
      const float y00 = x[0][0][0] + f2 * (x[0][0][1] - x[0][0][0]), y01 = x[0][1][0] + f2 * (x[0][1][1] - x[0][1][0]);
      const float y10 = x[1][0][0] + f2 * (x[1][0][1] - x[1][0][0]), y11 = x[1][1][0] + f2 * (x[1][1][1] - x[1][1][0]);
      const float z0 = y00 + f1 * (y01 - y00), z1 = y10 + f1 * (y11 - y10);
      float v = z0 + f0 * (z1 - z0);
      if (defer) { v = v + 0.f; mn = fminf(mn, v); mx = fmaxf(mx, v); }
      else v = aug_finish(v, mul, sm.shift, noisy, sm.noise_mean, sm.noise_std, ks, (int64_t)c * pvol + o);
      dst[(int64_t)c * pvol] = v;
    }
    if (label) {
      const int ni = floor_index(floorf(s0 + 0.5f), a.D), nj = floor_index(floorf(s1 + 0.5f), a.H), nk = floor_index(floorf(s2 + 0.5f), a.W);
      const bool inside = ni >= 0 && ni < a.D && nj >= 0 && nj < a.H && nk >= 0 && nk < a.W;
      const LB t = label[((int64_t)clampi(ni, a.D) * a.H + clampi(nj, a.H)) * a.W + clampi(nk, a.W)];
      olab[(int64_t)n * pvol + o] = (!zeros || inside) ? t : (LB)0;
    }
  }
  if (defer) {                     // (uniform per workgroup: the sample is blockIdx.z)
    __shared__ float red[2][4];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { mn = fminf(mn, __shfl_xor(mn, s, 64)); mx = fmaxf(mx, __shfl_xor(mx, s, 64)); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
      mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
      mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
      if (mn <= mx) {              // the minimum as the maximum of the complemented code: a zeroed scratch is the identity of both
        atomicMax(minmax + 4 * n, ~float_code(mn));
        atomicMax(minmax + 4 * n + 1, float_code(mx));
      }
    }
  }
}

// second launch: the samples with gamma, in place over their [C][rd][rh][rw] block
static __global__ void __launch_bounds__(256) augment_gamma_kernel(float* __restrict__ oimg, uint32_t* __restrict__ minmax, AffArgs a) {
  const int n = blockIdx.z;
  const miseg_aug_affine_sample& sm = a.s[n];
  if (!(sm.gamma > 0.f)) return;
  __shared__ uint32_t code[2];
  if (threadIdx.x == 0) { code[0] = minmax[4 * n]; code[1] = minmax[4 * n + 1]; }
  __syncthreads();
  const float lo = code_float(~code[0]), range = code_float(code[1]) - lo, den = range + 1e-7f;
  const float mul = 1.f + sm.scale;
  const bool noisy = sm.noise_std > 0.f;
  const uint64_t ks = noisy ? noise_sample_key(a.key, n) : 0ull;
  const int64_t total = (int64_t)a.C * a.rd * a.rh * a.rw;
  float* p = oimg + (int64_t)n * total;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const float v = powf((p[e] - lo) / den, sm.gamma) * range + lo;
    p[e] = aug_finish(v, mul, sm.shift, noisy, sm.noise_mean, sm.noise_std, ks, e);
  }
  // every workgroup of the sample has read the codes (before its loop) when it arrives here: the last one hands the scratch back zeroed
  if (threadIdx.x == 0) {
    const uint32_t prev = atomicAdd(minmax + 4 * n + 2, 1u);
    if (prev == gridDim.x - 1) { minmax[4 * n] = 0u; minmax[4 * n + 1] = 0u; minmax[4 * n + 2] = 0u; }
  }
}

}  // namespace miseg

using namespace miseg;

extern "C" int miseg_augment_affine(const miseg_augment_affine_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_augment_affine_params), MISEG_E_BADARG, "augment_affine: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_augment_affine_params));
  MISEG_REQUIRE(p->image && p->out_image && p->samples_host && (!p->label || p->out_label), MISEG_E_BADARG, "augment_affine: null pointer");
  MISEG_REQUIRE(p->n > 0 && p->n <= MISEG_AUG_MAX_SAMPLES, MISEG_E_UNSUPPORTED, "augment_affine: %d samples (1..%d)", p->n, MISEG_AUG_MAX_SAMPLES);
  MISEG_REQUIRE(p->label_bytes == 1 || p->label_bytes == 4 || p->label_bytes == 8, MISEG_E_UNSUPPORTED, "augment_affine: label element of %d bytes (1, 4 or 8)",
                p->label_bytes);
  MISEG_REQUIRE(p->padding_mode == MISEG_AUG_PAD_BORDER || p->padding_mode == MISEG_AUG_PAD_ZEROS, MISEG_E_UNSUPPORTED, "augment_affine: unknown padding_mode %d",
                p->padding_mode);
  MISEG_REQUIRE(p->C > 0 && p->D > 0 && p->H > 0 && p->W > 0 && p->rd > 0 && p->rh > 0 && p->rw > 0, MISEG_E_BADARG,
                "augment_affine: C %d, volume %dx%dx%d, roi %dx%dx%d: a value below 1", p->C, p->D, p->H, p->W, p->rd, p->rh, p->rw);
  // the coordinates are fp32: every index of the volume has to be one exactly
  MISEG_REQUIRE(p->D < (1 << 22) && p->H < (1 << 22) && p->W < (1 << 22), MISEG_E_UNSUPPORTED, "augment_affine: a volume axis of 2^22 or more");
  AffArgs a;
  a.C = p->C; a.D = p->D; a.H = p->H; a.W = p->W; a.rd = p->rd; a.rh = p->rh; a.rw = p->rw; a.n = p->n; a.pad = p->padding_mode;
  a.key = dropout_host_key(p->seed, p->draw);
  bool any_gamma = false;
  for (int i = 0; i < p->n; ++i) {
    const miseg_aug_affine_sample& q = p->samples_host[i];
    // an identity sample gathers by integer index: its crop stays inside the volume (checked for every sample: the crop is drawn inside)
    MISEG_REQUIRE(q.origin[0] >= 0 && q.origin[1] >= 0 && q.origin[2] >= 0 && q.origin[0] + p->rd <= p->D && q.origin[1] + p->rh <= p->H && q.origin[2] + p->rw <= p->W,
                  MISEG_E_BADARG, "augment_affine: sample %d crop (%d,%d,%d)+(%d,%d,%d) leaves the %dx%dx%d volume", i, q.origin[0], q.origin[1], q.origin[2], p->rd,
                  p->rh, p->rw, p->D, p->H, p->W);
    MISEG_REQUIRE(!(q.rot_k & 1) || p->rd == p->rh, MISEG_E_BADARG, "augment_affine: an odd number of quarter turns needs roi_d == roi_h");
    bool finite = isfinite(q.scale) && isfinite(q.shift) && isfinite(q.gamma) && isfinite(q.noise_mean) && isfinite(q.noise_std);
    for (int e = 0; e < 9; ++e) finite = finite && isfinite(q.m[e]);
    for (int e = 0; e < 3; ++e) finite = finite && isfinite(q.t[e]);
    MISEG_REQUIRE(finite, MISEG_E_BADARG, "augment_affine: sample %d has a non-finite m / t / scale / shift / gamma / noise value", i);
    any_gamma = any_gamma || q.gamma > 0.f;
    a.s[i] = q;
  }
  MISEG_REQUIRE(!any_gamma || p->minmax, MISEG_E_BADARG, "augment_affine: a sample has gamma and minmax is null");
  const int64_t pvol = (int64_t)p->rd * p->rh * p->rw;
  int gx = cdiv(pvol, 256 * 4);
  if (gx > 1024) gx = 1024;
  const dim3 grid(gx, 1, p->n);
  if (!p->label || p->label_bytes == 1)
    augment_affine_kernel<uint8_t><<<grid, 256, 0, s>>>(p->image, (const uint8_t*)p->label, p->out_image, (uint8_t*)p->out_label, p->minmax, a);
  else if (p->label_bytes == 4)
    augment_affine_kernel<uint32_t><<<grid, 256, 0, s>>>(p->image, (const uint32_t*)p->label, p->out_image, (uint32_t*)p->out_label, p->minmax, a);
  else
    augment_affine_kernel<uint64_t><<<grid, 256, 0, s>>>(p->image, (const uint64_t*)p->label, p->out_image, (uint64_t*)p->out_label, p->minmax, a);
  MISEG_LAUNCH_CHECK("augment_affine");
  if (any_gamma) {
    int gg = cdiv(pvol * p->C, 256 * 4);
    if (gg > 2048) gg = 2048;
    augment_gamma_kernel<<<dim3(gg, 1, p->n), 256, 0, s>>>(p->out_image, p->minmax, a);
    MISEG_LAUNCH_CHECK("augment_affine (gamma)");
  }
  return MISEG_OK;
}
