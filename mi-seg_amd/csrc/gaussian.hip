// Separable Gaussian filter on a batch of patches: the smoothing / sharpening end of the device augmenter (include/miseg_hip.h:
// miseg_gaussian_filter3d).  One workgroup of 512 threads per TD x TH x TW output tile of one channel volume
// (blockIdx.x = the tile, .y = the channel, .z = the sample), the per-sample descriptors in the kernel arguments.
//   The tile's input with its halo is (TD + 2 rd) x (TH + 2 rh) x (TW + 2 rw) values.  It goes through LDS GP planes at a time:
//     stage   global -> registers -> sA [GP * eh][ew]: zeros outside the volume, in groups of four along W (the W halo is rounded up to 4):
//             one 16-byte load a group when every row of the volume is 16-byte aligned (W % 4 == 0: a group is inside its row or outside it),
//             four 4-byte loads otherwise.  The loads of the NEXT chunk are issued before the passes of this one and land in sA behind them.
//     W pass  sA -> sB [GP * eh][TW]
//     H pass  sB -> sR [ed][TH][TW], which keeps the H results of every plane
//   and after the last chunk the D pass reads sR and stores the tile, W fastest, with the sharpen epilogue on the way when the sample asks
//   for it (its centre value is read again from src: a cache hit).  Two barriers a chunk: sA is free once the W pass is behind its barrier,
//   and the next W pass writes sB only behind the next stage barrier.  Lanes run along W in every pass: no LDS bank conflicts.
//   Per element acc = 0; acc = fl(acc + fl(w[k] * v[k])) for k = -r..r, contraction off for the whole file.  The passes are unrolled for the
//   even radii 2, 4, 6, 8 (taps in scalar registers, LDS offsets in the instructions); the host hands an odd radius r over as r + 1 with a
//   zero tap at either end.  That, like a value outside the volume, which is staged as +0, adds fl(0 * v) = +-0 to acc: acc starts at +0 and
//   never becomes -0, so its bits stay as they are - the same as skipping the tap (v is finite).  An axis of radius 0 copies.
//   A tile at a face of the volume, a volume smaller than a tile or than the halo: all the same code, the stores masked.
//   LDS: (GP * 32 * 48 + GP * 32 * 32 + 24 * 16 * 32) * 4 B = 78 KiB at any radius (static): two workgroups a CU.  Measured on a batch of
//   two 96^3 patches (432 workgroups on 256 CUs): 42 us a call at radius 6 and 48 us at radius 8 with GP = 3, 46 us and 63 us with GP = 4
//   (88 KiB, one workgroup a CU); one patch (216 workgroups) takes 28 us and 33 us either way.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace miseg {

static constexpr int GR = MISEG_GAUSS_MAX_RADIUS, TD = MISEG_GAUSS_TILE_D, TH = MISEG_GAUSS_TILE_H, TW = MISEG_GAUSS_TILE_W;
static constexpr int GP = 3;                       // planes a chunk
static constexpr int GT = 512;                     // threads
static constexpr int GED = TD + 2 * GR, GEH = TH + 2 * GR, GEW = TW + 2 * GR;      // the largest staged extents (GR is a multiple of 4)
static constexpr int GSTAGE = (GP * GEH * GEW / 4 + GT - 1) / GT;                  // groups of four a thread stages a chunk, at most
static_assert(TW == 32 && TH == 16 && GT % TW == 0 && GR == 8, "the index arithmetic and the radius dispatch below are written for these");

struct GaussArgs {
  int C, D, H, W, vec;
  miseg_gaussian_filter_sample s[MISEG_AUG_MAX_SAMPLES];      // radii made even (gauss_even)
};
static_assert(sizeof(GaussArgs) + 64 < 4096, "the descriptors travel in the kernel arguments");

// acc = 0; acc = fl(acc + fl(w[k] * v[(k - R) * STRIDE])) for the 2 R + 1 taps around v; R == 0: the value itself
template <int R, int STRIDE>
__device__ __forceinline__ float gauss_taps(const float (&w)[2 * GR + 1], const float* v) {
  if (R == 0) return v[0];
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k <= 2 * R; ++k) acc = acc + w[k] * v[(k - R) * STRIDE];
  return acc;
}

// a uniform switch over the even radii
#define MISEG_GAUSS_RADII(r, CALL) \
  switch (r) {                     \
    case 0: CALL(0); break;        \
    case 2: CALL(2); break;        \
    case 4: CALL(4); break;        \
    case 6: CALL(6); break;        \
    default: CALL(8); break;       \
  }

template <int R>
__device__ __forceinline__ void gauss_w_pass(const float (&w)[2 * GR + 1], const float* sA, float* sB, int rows, int rwa, int tid) {
  for (int i = tid; i < rows * TW; i += GT) sB[i] = gauss_taps<R, 1>(w, &sA[(i >> 5) * GEW + rwa + (i & 31)]);
}

template <int R>
__device__ __forceinline__ void gauss_h_pass(const float (&w)[2 * GR + 1], const float* sB, float* sR, int np, int eh, int tid) {
  for (int i = tid; i < np * TH * TW; i += GT) {
    const int x = i & 31, y = (i >> 5) & 15, z = i >> 9;
    sR[i] = gauss_taps<R, TW>(w, &sB[(z * eh + y + R) * TW + x]);
  }
}

template <int R>
__device__ __forceinline__ void gauss_d_pass(const miseg_gaussian_filter_sample& sm, const GaussArgs& a, const float* sR, const float* __restrict__ s,
                                             float* __restrict__ d, int d0, int h0, int w0, int tid) {
  for (int i = tid; i < TD * TH * TW; i += GT) {
    const int gx = w0 + (i & 31), gy = h0 + ((i >> 5) & 15), gz = d0 + (i >> 9);
    if (gx < a.W && gy < a.H && gz < a.D) {
      const int64_t g = ((int64_t)gz * a.H + gy) * a.W + gx;
      float v = gauss_taps<R, TH * TW>(sm.taps[0], &sR[i + R * TH * TW]);
      if (sm.sharpen) {
        const float c = s[g];
        const float diff = c - v;
        const float scaled = sm.alpha * diff;
        v = c + scaled;
      }
      d[g] = v;
    }
  }
}

static __global__ void __launch_bounds__(GT) gaussian_filter3d_kernel(const float* __restrict__ src, float* __restrict__ dst, GaussArgs a) {
  __shared__ __attribute__((aligned(16))) float sA[GP * GEH * GEW];
  __shared__ float sB[GP * GEH * TW];
  __shared__ float sR[GED * TH * TW];
  const miseg_gaussian_filter_sample& sm = a.s[blockIdx.z];
  const int rd = sm.radius[0], rh = sm.radius[1], rw = sm.radius[2];
  const int tid = threadIdx.x;
  const int ntw = cdiv(a.W, TW), nth = cdiv(a.H, TH);
  const int w0 = (int)(blockIdx.x % ntw) * TW, h0 = (int)((blockIdx.x / ntw) % nth) * TH, d0 = (int)(blockIdx.x / ((unsigned)ntw * nth)) * TD;
  const int64_t base = ((int64_t)blockIdx.z * a.C + blockIdx.y) * ((int64_t)a.D * a.H * a.W);
  const float* s = src + base;
  float* d = dst + base;

  if (rd == 0 && rh == 0 && rw == 0 && !sm.sharpen) {        // (uniform per workgroup) the verbatim copy, as words
    for (int i = tid; i < TD * TH * TW; i += GT) {
      const int gx = w0 + (i & 31), gy = h0 + ((i >> 5) & 15), gz = d0 + (i >> 9);
      if (gx < a.W && gy < a.H && gz < a.D) {
        const int64_t g = ((int64_t)gz * a.H + gy) * a.W + gx;
        reinterpret_cast<uint32_t*>(d)[g] = reinterpret_cast<const uint32_t*>(s)[g];
      }
    }
    return;
  }

  const int ed = TD + 2 * rd, eh = TH + 2 * rh, rwa = (rw + 3) & ~3, ew4 = (TW + 2 * rwa) >> 2;
  f32x4 pre[GSTAGE];
  // group i of the chunk at plane z0 -> its place in sA (-1: none) and, in `pre`, its four values
  auto place = [&](int z0, int i) -> int {
    const int np = ed - z0 < GP ? ed - z0 : GP;
    return i < np * eh * ew4 ? (i / ew4) * GEW + 4 * (i % ew4) : -1;
  };
  auto load_chunk = [&](int z0) {
#pragma unroll
    for (int j = 0; j < GSTAGE; ++j) {
      const int i = tid + j * GT;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (place(z0, i) >= 0) {
        const int row = i / ew4;
        const int gx = w0 - rwa + 4 * (i % ew4), gy = h0 - rh + row % eh, gz = d0 - rd + z0 + row / eh;
        if (gy >= 0 && gy < a.H && gz >= 0 && gz < a.D) {
          const float* r = s + ((int64_t)gz * a.H + gy) * a.W;
          if (a.vec) {
            if (gx >= 0 && gx < a.W) v = *reinterpret_cast<const f32x4*>(r + gx);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (gx + e >= 0 && gx + e < a.W) v[e] = r[gx + e];
          }
        }
      }
      pre[j] = v;
    }
  };

  load_chunk(0);
  for (int z0 = 0; z0 < ed; z0 += GP) {
    const int np = ed - z0 < GP ? ed - z0 : GP;
#pragma unroll
    for (int j = 0; j < GSTAGE; ++j) {
      const int at = place(z0, tid + j * GT);
      if (at >= 0) *reinterpret_cast<f32x4*>(&sA[at]) = pre[j];
    }
    if (z0 + GP < ed) load_chunk(z0 + GP);
    __syncthreads();
#define MISEG_GAUSS_W(R) gauss_w_pass<R>(sm.taps[2], sA, sB, np * eh, rwa, tid)
    MISEG_GAUSS_RADII(rw, MISEG_GAUSS_W)
    __syncthreads();
#define MISEG_GAUSS_H(R) gauss_h_pass<R>(sm.taps[1], sB, sR + z0 * TH * TW, np, eh, tid)
    MISEG_GAUSS_RADII(rh, MISEG_GAUSS_H)
  }
  __syncthreads();
#define MISEG_GAUSS_D(R) gauss_d_pass<R>(sm, a, sR, s, d, d0, h0, w0, tid)
  MISEG_GAUSS_RADII(rd, MISEG_GAUSS_D)
}

// the kernel's form of a descriptor: an odd radius r becomes r + 1 with a zero tap at either end, the taps it does not read are zero
static miseg_gaussian_filter_sample gauss_even(const miseg_gaussian_filter_sample& q) {
  miseg_gaussian_filter_sample e{};
  for (int ax = 0; ax < 3; ++ax) {
    const int r = q.radius[ax], pad = r & 1;
    e.radius[ax] = r + pad;
    for (int k = 0; r > 0 && k <= 2 * r; ++k) e.taps[ax][k + pad] = q.taps[ax][k];
  }
  e.alpha = q.alpha;
  e.sharpen = q.sharpen;
  return e;
}

}  // namespace miseg

using namespace miseg;

extern "C" int miseg_gaussian_filter3d(const miseg_gaussian_filter_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_gaussian_filter_params), MISEG_E_BADARG, "gaussian_filter3d: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_gaussian_filter_params));
  MISEG_REQUIRE(p->src && p->dst && p->samples_host, MISEG_E_BADARG, "gaussian_filter3d: null pointer");
  MISEG_REQUIRE(p->n > 0 && p->n <= MISEG_AUG_MAX_SAMPLES, MISEG_E_BADARG, "gaussian_filter3d: %d samples (1..%d)", p->n, MISEG_AUG_MAX_SAMPLES);
  MISEG_REQUIRE(p->C > 0 && p->D > 0 && p->H > 0 && p->W > 0, MISEG_E_BADARG, "gaussian_filter3d: C %d, volume %dx%dx%d: a value below 1", p->C, p->D, p->H, p->W);
  const uint64_t elems = (uint64_t)p->n * p->C * p->D * p->H * p->W;
  const uintptr_t sb = (uintptr_t)p->src, db = (uintptr_t)p->dst;
  MISEG_REQUIRE(sb + elems * 4 <= db || db + elems * 4 <= sb, MISEG_E_BADARG, "gaussian_filter3d: src and dst overlap (the filter reads neighbours: not in place)");
  MISEG_REQUIRE(p->C <= 65535, MISEG_E_UNSUPPORTED, "gaussian_filter3d: %d channels (at most 65535)", p->C);
  const int64_t tiles = (int64_t)cdiv(p->D, TD) * cdiv(p->H, TH) * cdiv(p->W, TW);
  MISEG_REQUIRE(tiles <= 0x7fffffffll, MISEG_E_UNSUPPORTED, "gaussian_filter3d: %lld tiles in a channel volume", (long long)tiles);
  GaussArgs a;
  a.C = p->C; a.D = p->D; a.H = p->H; a.W = p->W;
  a.vec = (sb & 15) == 0 && (p->W & 3) == 0;
  for (int i = 0; i < MISEG_AUG_MAX_SAMPLES; ++i) a.s[i] = miseg_gaussian_filter_sample{};
  for (int i = 0; i < p->n; ++i) {
    const miseg_gaussian_filter_sample& q = p->samples_host[i];
    for (int ax = 0; ax < 3; ++ax) {
      MISEG_REQUIRE(q.radius[ax] >= 0 && q.radius[ax] <= GR, MISEG_E_BADARG, "gaussian_filter3d: sample %d axis %d: radius %d (0..%d)", i, ax, q.radius[ax], GR);
      for (int k = 0; q.radius[ax] > 0 && k <= 2 * q.radius[ax]; ++k)
        MISEG_REQUIRE(isfinite(q.taps[ax][k]), MISEG_E_BADARG, "gaussian_filter3d: sample %d axis %d: a non-finite tap", i, ax);
    }
    MISEG_REQUIRE(isfinite(q.alpha), MISEG_E_BADARG, "gaussian_filter3d: sample %d: a non-finite alpha", i);
    a.s[i] = gauss_even(q);
  }
  gaussian_filter3d_kernel<<<dim3((unsigned)tiles, p->C, p->n), GT, 0, s>>>(p->src, p->dst, a);
  MISEG_LAUNCH_CHECK("gaussian_filter3d");
  return MISEG_OK;
}
