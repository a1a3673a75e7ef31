// The soft prediction export (include/miseg_hip.h: miseg_soft_export): class scores are blended trilinearly onto the
// file's grid before the argmax, and the blended scores can be written beside the labels.  The host's per-axis tables (lo, hi, t) carry all
// geometry; the kernels compute no coordinate.
//   lerp(a, b, t) = t == 0 ? a : fl(fl(a * fl(1 - t)) + fl(b * t)), along logits W, then H, then D; every operation is rounded on its own
// (contraction is off for the whole file, as in ensemble.hip), so the numpy restatement of the tests gives the same bits.
//   One workgroup = a 64 (X) x 64 (axis f) output tile at one coordinate of axis g, f being the output axis that indexes logits W unless X
// does (miseg_label_export's tile).  Channel after channel, the source voxels under the tile - the span of the tile's taps along X and f, the
// two planes lo / hi of g - are read into an LDS image with the lanes along logits W, and every output takes its 8 taps from the image:
// neighbouring outputs of an upsampling share them.  The image's rows run along X's source axis with an odd pitch, so the fill is free of
// bank conflicts when the lanes run along f, and the lanes of the blend (along X) read equal or adjacent words.  A tile whose span does not fit
// the image (a strong downsampling, or tables that jump) reads its taps from memory instead.  Stores go out with the lanes along X.
//   Every tap index is clamped into the box on the device, and an image index is a clamped index minus the minimum of the tile's clamped
// indices, so every address lies inside the scores / the image whatever the tables hold.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace miseg {

constexpr int SOFT_TILE = 64;
constexpr int SOFT_IMAGE = 9216;   // floats of the LDS image: 2 planes x 67 x 67 with the odd pitch fit (equal sampling spans 65 x 65)

struct SoftArgs {
  // per tile role 0 = X, 1 = f, 2 = g
  const int32_t* lo[3]; const int32_t* hi[3]; const float* t[3];
  int n[3], b0[3], bn[3], lv[3];   // output side; box origin / extent and number (0 D, 1 H, 2 W) of the role's logits axis
  int64_t st[3], ost[3];           // source / output stride of the role's axis (elements)
  int64_t cstride, ovox;           // channel stride of the source / of prob
  int C, fast_x, out_bytes, prob_bytes;
};

__device__ __forceinline__ float soft_lerp(float a, float b, float t, float u) { return t == 0.f ? a : a * u + b * t; }

__device__ __forceinline__ int soft_clamp(int v, int n) { return min(max(v, 0), n - 1); }

// softmax over the channels of every voxel of the box, into a packed [C][bd][bh][bw] image (lanes along w)
static __global__ void __launch_bounds__(256) soft_softmax_kernel(const float* __restrict__ scores, float* __restrict__ ws, int C, int H, int W, int64_t vox,
                                                                  int d0, int h0, int w0, int bh, int bw, int nbox) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < nbox; e += gridDim.x * 256) {
    const int w = e % bw, h = (e / bw) % bh, d = e / (bw * bh);
    const float* x = scores + ((int64_t)(d0 + d) * H + (h0 + h)) * W + (w0 + w);
    float mx = x[0];
    for (int c = 1; c < C; ++c) {
      const float v = x[(int64_t)c * vox];
      if (v > mx) mx = v;
    }
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum = sum + expf(x[(int64_t)c * vox] - mx);
    for (int c = 0; c < C; ++c) ws[(int64_t)c * nbox + e] = expf(x[(int64_t)c * vox] - mx) / sum;
  }
}

// the blend of one output from its 8 taps v[bx | bf << 1 | bg << 2] (tile roles X, f, g) and the roles' weights t3: along the role RW that
// indexes logits W first, then RH, then the third - the logits' order, whatever the tile's
template <int RW, int RH>
__device__ __forceinline__ float soft_blend8(const float (&v)[8], const float (&t3)[3]) {
  constexpr int RD = 3 - RW - RH;
  const float tW = t3[RW], tH = t3[RH], tD = t3[RD], uW = 1.f - tW, uH = 1.f - tH, uD = 1.f - tD;
  float h[2];
#pragma unroll
  for (int bd = 0; bd < 2; ++bd) {
    float w[2];
#pragma unroll
    for (int bh = 0; bh < 2; ++bh) w[bh] = soft_lerp(v[(bh << RH) | (bd << RD)], v[(1 << RW) | (bh << RH) | (bd << RD)], tW, uW);
    h[bd] = soft_lerp(w[0], w[1], tH, uH);
  }
  return soft_lerp(h[0], h[1], tD, uD);
}

// RW / RH: the tile role (0 = X, 1 = f, 2 = g) that indexes logits W / H
template <int RW, int RH>
static __global__ void __launch_bounds__(256) soft_export_kernel(const float* __restrict__ src, const int32_t* __restrict__ lut, void* __restrict__ out,
                                                                 void* __restrict__ prob, SoftArgs a) {
  __shared__ float image[SOFT_IMAGE];
  __shared__ int lo_s[2][SOFT_TILE], hi_s[2][SOFT_TILE], mn_s[2], span_s[2];
  __shared__ float t_s[2][SOFT_TILE];
  __shared__ uint32_t lut_s[64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int x0 = blockIdx.x * SOFT_TILE, j0 = blockIdx.y * SOFT_TILE, cg = blockIdx.z;
  if (wv < 2) {                    // wave 0: the tile's X coordinates, wave 1: its f coordinates (past the side: the last one again)
    const int c = min((wv == 0 ? x0 : j0) + lane, a.n[wv] - 1);
    const int l = soft_clamp(a.lo[wv][c] - a.b0[wv], a.bn[wv]), h = soft_clamp(a.hi[wv][c] - a.b0[wv], a.bn[wv]);
    int mn = min(l, h), mx = max(l, h);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = min(mn, __shfl_xor(mn, o, 64));
      mx = max(mx, __shfl_xor(mx, o, 64));
    }
    lo_s[wv][lane] = l - mn;
    hi_s[wv][lane] = h - mn;
    t_s[wv][lane] = a.t[wv][c];
    if (lane == 0) { mn_s[wv] = mn; span_s[wv] = mx - mn + 1; }
  } else if (wv == 2) {
    if (out != nullptr && lane < a.C) lut_s[lane] = (uint32_t)lut[lane];
  }
  __syncthreads();
  const float tg = a.t[2][cg];
  const int lg = soft_clamp(a.lo[2][cg] - a.b0[2], a.bn[2]);
  const int hg = tg == 0.f ? lg : soft_clamp(a.hi[2][cg] - a.b0[2], a.bn[2]);     // t == 0: the hi plane is never used, nor read
  const int planes = hg == lg ? 1 : 2;
  const int sx = span_s[0], sf = span_s[1], pitch = sx | 1;
  const bool staged = 2 * sf * pitch <= SOFT_IMAGE;
  // the tile's first source voxel: channel 0, plane lo of g
  const float* base = src + (int64_t)mn_s[0] * a.st[0] + (int64_t)mn_s[1] * a.st[1] + (int64_t)lg * a.st[2];
  const int64_t gstep = (int64_t)(hg - lg) * a.st[2];
  // the fill walks rows of the image's fast source axis (logits W: X's when fast_x, else f's) with 16, 32 or 64 lanes a row
  const int sfast = a.fast_x ? sx : sf, sslow = a.fast_x ? sf : sx;
  const int lsh = sfast <= 16 ? 4 : (sfast <= 32 ? 5 : 6), q0 = tid & ((1 << lsh) - 1), row0 = tid >> lsh, rstep = 256 >> lsh;
  const int i = lane;
  const bool xin = x0 + i < a.n[0];
  const int lx = lo_s[0][i], hx = hi_s[0][i];
  float t3[3] = {t_s[0][i], 0.f, tg};
  float best[SOFT_TILE / 4];
  int arg[SOFT_TILE / 4];
#pragma unroll
  for (int k = 0; k < SOFT_TILE / 4; ++k) { best[k] = 0.f; arg[k] = 0; }
  for (int c = 0; c < a.C; ++c) {
    const float* sc = base + (int64_t)c * a.cstride;
    if (staged) {
      __syncthreads();             // the previous channel's blend has read the image
      for (int row = row0; row < planes * sslow; row += rstep) {
        const int pl = row >= sslow ? 1 : 0, s = row - pl * sslow;
        const float* rp = sc + (int64_t)s * a.st[a.fast_x ? 1 : 0] + (pl ? gstep : 0);
        float* ip = image + pl * sf * pitch + (a.fast_x ? s * pitch : s);
        for (int q = q0; q < sfast; q += 1 << lsh) ip[a.fast_x ? q : q * pitch] = rp[q];      // (the fast source axis has stride 1)
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < SOFT_TILE / 4; ++k) {
      const int j = wv + 4 * k;
      if (j0 + j >= a.n[1]) continue;            // (uniform over the wave)
      t3[1] = t_s[1][j];
      const int lf = lo_s[1][j], hf = hi_s[1][j];
      float v[8];
      if (staged) {
        const int ox[2] = {lx, hx}, of[2] = {lf * pitch, hf * pitch}, og[2] = {0, planes == 2 ? sf * pitch : 0};
#pragma unroll
        for (int b = 0; b < 8; ++b) v[b] = image[ox[b & 1] + of[(b >> 1) & 1] + og[b >> 2]];
      } else {
        const int64_t ox[2] = {lx * a.st[0], hx * a.st[0]}, of[2] = {lf * a.st[1], hf * a.st[1]}, og[2] = {0, gstep};
#pragma unroll
        for (int b = 0; b < 8; ++b) v[b] = sc[ox[b & 1] + of[(b >> 1) & 1] + og[b >> 2]];
      }
      const float r = soft_blend8<RW, RH>(v, t3);
      if (c == 0) best[k] = r;
      else if (r > best[k]) { best[k] = r; arg[k] = c; }       // strict: the FIRST maximum wins; a NaN after channel 0 never does
      if (prob != nullptr && xin) {
        const int64_t o = (int64_t)c * a.ovox + x0 + i + (int64_t)(j0 + j) * a.ost[1] + (int64_t)cg * a.ost[2];
        if (a.prob_bytes == 4) ((float*)prob)[o] = r;
        else ((uint8_t*)prob)[o] = r == r ? (uint8_t)min(255, max(0, (int)floorf(r * 255.f + 0.5f))) : (uint8_t)0;
      }
    }
  }
  if (out == nullptr || !xin) return;
#pragma unroll
  for (int k = 0; k < SOFT_TILE / 4; ++k) {
    const int j = wv + 4 * k;
    if (j0 + j >= a.n[1]) continue;
    const int64_t o = x0 + i + (int64_t)(j0 + j) * a.ost[1] + (int64_t)cg * a.ost[2];
    const uint32_t v = lut_s[arg[k]];
    if (a.out_bytes == 1) ((uint8_t*)out)[o] = (uint8_t)v;
    else if (a.out_bytes == 2) ((uint16_t*)out)[o] = (uint16_t)v;
    else ((uint32_t*)out)[o] = v;
  }
}
}  // namespace miseg
using namespace miseg;

extern "C" size_t miseg_soft_export_workspace_bytes(int C, int box_nd, int box_nh, int box_nw, int softmax) {
  if (!softmax || C <= 0 || box_nd <= 0 || box_nh <= 0 || box_nw <= 0) return 0;
  return (((size_t)C * box_nd * box_nh * box_nw * sizeof(float)) + 255) & ~(size_t)255;
}

extern "C" int miseg_soft_export(const miseg_soft_export_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_soft_export_params), MISEG_E_BADARG, "soft_export: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_soft_export_params));
  MISEG_REQUIRE(p->out || p->prob, MISEG_E_BADARG, "soft_export: both outputs are null (labels, scores or both)");
  MISEG_REQUIRE(p->scores && (p->lut || !p->out), MISEG_E_BADARG, "soft_export: null pointer");
  for (int k = 0; k < 3; ++k)
    MISEG_REQUIRE(p->lo[k] && p->hi[k] && p->t[k] && p->lo_host[k] && p->hi_host[k], MISEG_E_BADARG, "soft_export: null table (axis %c)", "XYZ"[k]);
  MISEG_REQUIRE(p->C >= 1 && p->C <= 64, MISEG_E_BADARG, "soft_export: C %d (1..64)", p->C);
  MISEG_REQUIRE(!p->out || p->out_bytes == 1 || p->out_bytes == 2 || p->out_bytes == 4, MISEG_E_BADARG, "soft_export: out_bytes %d (1, 2 or 4)", p->out_bytes);
  MISEG_REQUIRE(!p->prob || p->prob_bytes == 1 || p->prob_bytes == 4, MISEG_E_BADARG, "soft_export: prob_bytes %d (4: fp32, 1: uint8)", p->prob_bytes);
  MISEG_REQUIRE(!p->prob || p->prob_bytes == 4 || p->softmax || p->unit_range, MISEG_E_UNSUPPORTED,
                "soft_export: uint8 scores need values in [0, 1]: softmax, or unit_range declared by the caller");
  const int dims[3] = {p->D, p->H, p->W}, b0[3] = {p->box_d0, p->box_h0, p->box_w0}, bn[3] = {p->box_nd, p->box_nh, p->box_nw};
  const int n[3] = {p->nx, p->ny, p->nz}, axis[3] = {p->axis_x, p->axis_y, p->axis_z};
  for (int k = 0; k < 3; ++k) {
    MISEG_REQUIRE(dims[k] > 0 && dims[k] <= 65535 && n[k] > 0 && n[k] <= 65535, MISEG_E_BADARG, "soft_export: scores %dx%dx%d, out %dx%dx%d (sides 1..65535)",
                  p->D, p->H, p->W, p->nx, p->ny, p->nz);
    MISEG_REQUIRE(b0[k] >= 0 && bn[k] > 0 && b0[k] + bn[k] <= dims[k], MISEG_E_BADARG, "soft_export: box axis %d [%d, %d + %d) leaves the side %d", k, b0[k],
                  b0[k], bn[k], dims[k]);
    MISEG_REQUIRE(axis[k] >= 0 && axis[k] < 3 && axis[k] != axis[(k + 1) % 3] && axis[k] != axis[(k + 2) % 3], MISEG_E_BADARG,
                  "soft_export: axes (%d, %d, %d) are not a permutation of (0, 1, 2)", axis[0], axis[1], axis[2]);
  }
  const int64_t nbox = (int64_t)bn[0] * bn[1] * bn[2];
  MISEG_REQUIRE(nbox < ((int64_t)1 << 31), MISEG_E_UNSUPPORTED, "soft_export: box of %lld voxels (below 2^31)", (long long)nbox);
  MISEG_REQUIRE(!p->softmax || p->workspace, MISEG_E_BADARG, "soft_export: softmax needs the workspace");
  for (int k = 0; k < 3; ++k) {
    const int first = b0[axis[k]], end = first + bn[axis[k]];
    for (int i = 0; i < n[k]; ++i) {
      const int l = p->lo_host[k][i], h = p->hi_host[k][i];
      MISEG_REQUIRE(l >= first && l < end && h >= first && h < end, MISEG_E_BADARG, "soft_export: table %c[%d] = (%d, %d) leaves the box [%d, %d)", "XYZ"[k], i, l, h,
                    first, end);
      MISEG_REQUIRE(l <= h && h <= l + 1, MISEG_E_BADARG, "soft_export: table %c[%d]: hi %d outside [lo, lo + 1] of lo %d", "XYZ"[k], i, h, l);
    }
  }
  const float* src = p->scores + ((int64_t)b0[0] * p->H + b0[1]) * p->W + b0[2];
  // the softmax pass packs the box; raw scores are read where they lie: the whole volume's strides, from the box's first voxel
  int64_t st[3] = {(int64_t)p->H * p->W, p->W, 1}, cstride = (int64_t)p->D * p->H * p->W;
  if (p->softmax) {
    int g1 = cdiv(nbox, 256 * 4);
    if (g1 > 8192) g1 = 8192;
    soft_softmax_kernel<<<g1, 256, 0, s>>>(p->scores, (float*)p->workspace, p->C, p->H, p->W, cstride, b0[0], b0[1], b0[2], bn[1], bn[2], (int)nbox);
    MISEG_LAUNCH_CHECK("soft_export softmax");
    src = (const float*)p->workspace;
    st[0] = (int64_t)bn[1] * bn[2]; st[1] = bn[2]; cstride = nbox;
  }
  SoftArgs a;
  // the tile's second axis: the one that indexes the scores' fast axis W, unless X does (then Y)
  a.fast_x = axis[0] == 2;
  const int f = a.fast_x ? 1 : (axis[1] == 2 ? 1 : 2), role[3] = {0, f, 3 - f};
  const int64_t ost[3] = {1, (int64_t)n[0], (int64_t)n[0] * n[1]};
  for (int r = 0; r < 3; ++r) {
    const int k = role[r];
    a.lo[r] = p->lo[k]; a.hi[r] = p->hi[k]; a.t[r] = p->t[k];
    a.n[r] = n[k]; a.b0[r] = b0[axis[k]]; a.bn[r] = bn[axis[k]]; a.lv[r] = axis[k];
    a.st[r] = st[axis[k]]; a.ost[r] = ost[k];
  }
  a.cstride = cstride;
  a.ovox = (int64_t)n[0] * n[1] * n[2];
  a.C = p->C;
  a.out_bytes = p->out_bytes;
  a.prob_bytes = p->prob_bytes;
  const dim3 grid(cdiv(a.n[0], SOFT_TILE), cdiv(a.n[1], SOFT_TILE), a.n[2]);
  // the tile role that indexes logits W / H picks the instantiation: the blend runs along W, then H, then D
  int rW = 0, rH = 0;
  for (int r = 0; r < 3; ++r) { if (a.lv[r] == 2) rW = r; if (a.lv[r] == 1) rH = r; }
  const int32_t* lut = p->lut;
  void *out = p->out, *prob = p->prob;
  switch (rW * 3 + rH) {
    case 1: soft_export_kernel<0, 1><<<grid, 256, 0, s>>>(src, lut, out, prob, a); break;
    case 2: soft_export_kernel<0, 2><<<grid, 256, 0, s>>>(src, lut, out, prob, a); break;
    case 3: soft_export_kernel<1, 0><<<grid, 256, 0, s>>>(src, lut, out, prob, a); break;
    case 5: soft_export_kernel<1, 2><<<grid, 256, 0, s>>>(src, lut, out, prob, a); break;
    default: return set_error(MISEG_E_BADARG, "soft_export: logits W is indexed by the tile's plane axis");   // (f indexes W unless X does)
  }
  MISEG_LAUNCH_CHECK("soft_export blend");
  return MISEG_OK;
}
