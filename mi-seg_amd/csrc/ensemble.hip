// Flip test-time augmentation / model ensembling (include/miseg_hip.h: miseg_ensemble_accumulate): one streaming pass
// folds one member's stitched logits, predicted on a flipped copy of the volume, into the running accumulator in the volume's own frame.
//   acc' = fl(fl(acc + fl(w_c * t_c)) * s_c)      t = x | softmax_c(x) | one-hot(first-maximum argmax x);  "+ acc" absent when first, "* s_c"
// absent unless scaled; every operation is rounded on its own (contraction is off for the whole file, as in the weighted stitch of
// training.hip), so kinds 0 and 2 give the bits of the torch restatement (hip/ops.py::ensemble_accumulate_torch).
//   A work item is up to 4 consecutive w of one (b, d, h) row with all C channels: src is read once (16-byte loads when W % 4 == 0 and the base
// is 16-byte aligned, a w flip reverses inside the register quad; scalar loads otherwise), acc is read unless first and written once.  Items
// are walked by a grid-stride loop; every element offset is 64-bit.  Plain vector loads and stores only: no atomics, no LDS.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace miseg {

struct EnsembleArgs {
  int B, C, D, H, W, nq;           // nq = ceil(W / 4) quads a row
  int fd, fh, fw, first, scaled, vsrc, vacc;
  int64_t items;                   // B * D * H * nq, below 2^32
  float weight[64], scale[64];
};

struct Quad { float v[4]; };

// the (up to) 4 values of row `p` that land on w0 .. w0 + n - 1 of the accumulator: mirrored along w when fw
__device__ __forceinline__ Quad load_quad(const float* __restrict__ p, int W, int w0, int n, bool fw, bool vec) {
  Quad q;
  if (vec) {                       // W % 4 == 0: n == 4 and the mirrored quad starts at W - 4 - w0, itself a multiple of 4
    const f32x4 t = *reinterpret_cast<const f32x4*>(p + (fw ? W - 4 - w0 : w0));
    q.v[0] = fw ? t[3] : t[0]; q.v[1] = fw ? t[2] : t[1]; q.v[2] = fw ? t[1] : t[2]; q.v[3] = fw ? t[0] : t[3];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) q.v[j] = j < n ? p[fw ? W - 1 - w0 - j : w0 + j] : 0.f;
  }
  return q;
}

__device__ __forceinline__ void store_quad(float* __restrict__ p, int w0, int n, bool vec, const Quad& q) {
  if (vec) {
    const f32x4 t = {q.v[0], q.v[1], q.v[2], q.v[3]};
    *reinterpret_cast<f32x4*>(p + w0) = t;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (j < n) p[w0 + j] = q.v[j];
  }
}

// item -> row offsets (elements, channel 0 of the item's sample) of the accumulator row and of the source row it mirrors, and the quad
__device__ __forceinline__ void ensemble_item(const EnsembleArgs& a, int64_t i, int64_t& dst_row, int64_t& src_row, int& w0, int& n) {
  // fewer than 2^32 items (the host refuses more): 32-bit divisions; the element offsets below are 64-bit
  const uint32_t u = (uint32_t)i, row = u / (uint32_t)a.nq, t = row / (uint32_t)a.H, bb = t / (uint32_t)a.D;
  const int q = (int)(u - row * (uint32_t)a.nq);
  const int64_t h = row - t * (uint32_t)a.H, d = t - bb * (uint32_t)a.D, b = bb;
  const int64_t sd = a.fd ? a.D - 1 - d : d, sh = a.fh ? a.H - 1 - h : h;
  const int64_t sample = b * a.C * ((int64_t)a.D * a.H * a.W);
  dst_row = sample + (d * a.H + h) * a.W;
  src_row = sample + (sd * a.H + sh) * a.W;
  w0 = q * 4;
  n = a.W - w0 < 4 ? a.W - w0 : 4;
}

// acc' of one element from its term t.  Plain operators under this file's `fp contract(off)`: the __fmul_rn / __fadd_rn of the HIP headers are
// inline functions compiled under the headers' own contraction mode, and their product and sum were fused into an FMA after inlining.
__device__ __forceinline__ float ensemble_fold(float t, float w, float s, float old, bool first, bool scaled) {
  const float term = w * t;
  const float sum = first ? term : old + term;
  return scaled ? sum * s : sum;
}

// MISEG_ENSEMBLE_MEAN_LOGITS: no channel depends on another, every channel streams through
static __global__ void __launch_bounds__(256) ensemble_logits_kernel(const float* __restrict__ src, float* __restrict__ acc, EnsembleArgs a) {
  const int64_t vox = (int64_t)a.D * a.H * a.W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.items; i += (int64_t)gridDim.x * 256) {
    int64_t dr, sr;
    int w0, n;
    ensemble_item(a, i, dr, sr, w0, n);
#pragma unroll 4
    for (int c = 0; c < a.C; ++c) {
      const Quad x = load_quad(src + sr + c * vox, a.W, w0, n, a.fw, a.vsrc);
      Quad o = {};
      if (!a.first) o = load_quad(acc + dr + c * vox, a.W, w0, n, false, a.vacc);
#pragma unroll
      for (int j = 0; j < 4; ++j) o.v[j] = ensemble_fold(x.v[j], a.weight[c], a.scale[c], o.v[j], a.first, a.scaled);
      store_quad(acc + dr + c * vox, w0, n, a.vacc, o);
    }
  }
}

// MISEG_ENSEMBLE_MEAN_PROB / MISEG_ENSEMBLE_VOTE: the term of a channel needs all channels of the voxel.  CMAX > 0: C <= CMAX channels of the
// quad stay in registers (statically indexed) and src is read once; CMAX == 0 (16 < C <= 64): src is read again in every pass over the channels.
template <int KIND, int CMAX>
static __global__ void __launch_bounds__(256) ensemble_cross_kernel(const float* __restrict__ src, float* __restrict__ acc, EnsembleArgs a) {
  constexpr int NX = CMAX > 0 ? CMAX : 1;
  const int64_t vox = (int64_t)a.D * a.H * a.W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.items; i += (int64_t)gridDim.x * 256) {
    int64_t dr, sr;
    int w0, n;
    ensemble_item(a, i, dr, sr, w0, n);
    Quad x[NX];
    if (CMAX > 0) {
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < a.C) x[c] = load_quad(src + sr + c * vox, a.W, w0, n, a.fw, a.vsrc);
        else x[c].v[0] = x[c].v[1] = x[c].v[2] = x[c].v[3] = 0.f;
    }
    // softmax: the maximum by fmaxf from -inf, as softmax_from (training.hip); vote: the strict `>` scan of ops.first_max_argmax from channel 0
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, sum[4] = {0.f, 0.f, 0.f, 0.f};
    int arg[4] = {0, 0, 0, 0};
    if (CMAX > 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) mx[j] = KIND == MISEG_ENSEMBLE_VOTE ? x[0].v[j] : -INFINITY;
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        if (c < a.C) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (KIND == MISEG_ENSEMBLE_VOTE) { if (c > 0 && x[c].v[j] > mx[j]) { mx[j] = x[c].v[j]; arg[j] = c; } }
            else mx[j] = fmaxf(mx[j], x[c].v[j]);
          }
        }
      }
      if (KIND == MISEG_ENSEMBLE_MEAN_PROB) {
#pragma unroll
        for (int c = 0; c < NX; ++c) {
          if (c < a.C) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { x[c].v[j] = expf(x[c].v[j] - mx[j]); sum[j] = sum[j] + x[c].v[j]; }
          }
        }
      }
    } else {
      for (int c = 0; c < a.C; ++c) {
        const Quad t = load_quad(src + sr + c * vox, a.W, w0, n, a.fw, a.vsrc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (KIND == MISEG_ENSEMBLE_VOTE) { if (c == 0) mx[j] = t.v[j]; else if (t.v[j] > mx[j]) { mx[j] = t.v[j]; arg[j] = c; } }
          else mx[j] = c == 0 ? fmaxf(-INFINITY, t.v[j]) : fmaxf(mx[j], t.v[j]);
        }
      }
      if (KIND == MISEG_ENSEMBLE_MEAN_PROB) {
        for (int c = 0; c < a.C; ++c) {
          const Quad t = load_quad(src + sr + c * vox, a.W, w0, n, a.fw, a.vsrc);
#pragma unroll
          for (int j = 0; j < 4; ++j) sum[j] = sum[j] + expf(t.v[j] - mx[j]);
        }
      }
    }
    float inv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) inv[j] = KIND == MISEG_ENSEMBLE_MEAN_PROB ? 1.f / sum[j] : 0.f;
    auto fold = [&](int c, const Quad& e) {
      Quad o = {};
      if (!a.first) o = load_quad(acc + dr + c * vox, a.W, w0, n, false, a.vacc);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = KIND == MISEG_ENSEMBLE_VOTE ? (arg[j] == c ? 1.f : 0.f) : e.v[j] * inv[j];
        o.v[j] = ensemble_fold(t, KIND == MISEG_ENSEMBLE_VOTE ? 1.f : a.weight[c], a.scale[c], o.v[j], a.first, a.scaled);
      }
      store_quad(acc + dr + c * vox, w0, n, a.vacc, o);
    };
    if (CMAX > 0) {
#pragma unroll
      for (int c = 0; c < NX; ++c) if (c < a.C) fold(c, x[c]);
    } else {
      for (int c = 0; c < a.C; ++c) {
        Quad e;
        e.v[0] = e.v[1] = e.v[2] = e.v[3] = 0.f;
        if (KIND == MISEG_ENSEMBLE_MEAN_PROB) {
          e = load_quad(src + sr + c * vox, a.W, w0, n, a.fw, a.vsrc);
#pragma unroll
          for (int j = 0; j < 4; ++j) e.v[j] = expf(e.v[j] - mx[j]);
        }
        fold(c, e);
      }
    }
  }
}

template <int KIND>
static void ensemble_cross_launch(int grid, hipStream_t s, const float* src, float* acc, const EnsembleArgs& a) {
  if (a.C <= 4) ensemble_cross_kernel<KIND, 4><<<grid, 256, 0, s>>>(src, acc, a);
  else if (a.C <= 8) ensemble_cross_kernel<KIND, 8><<<grid, 256, 0, s>>>(src, acc, a);
  else if (a.C <= 16) ensemble_cross_kernel<KIND, 16><<<grid, 256, 0, s>>>(src, acc, a);
  else ensemble_cross_kernel<KIND, 0><<<grid, 256, 0, s>>>(src, acc, a);
}

}  // namespace miseg

using namespace miseg;

extern "C" int miseg_ensemble_accumulate(const miseg_ensemble_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_ensemble_params), MISEG_E_BADARG, "ensemble_accumulate: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_ensemble_params));
  MISEG_REQUIRE(p->src && p->acc, MISEG_E_BADARG, "ensemble_accumulate: null src / acc");
  MISEG_REQUIRE(p->C >= 1 && p->C <= 64, MISEG_E_BADARG, "ensemble_accumulate: %d channels (1..64)", p->C);
  MISEG_REQUIRE(p->B >= 1 && p->D >= 1 && p->H >= 1 && p->W >= 1, MISEG_E_BADARG, "ensemble_accumulate: shape [%d, %d, %d, %d, %d] has a dimension below 1",
                p->B, p->C, p->D, p->H, p->W);
  MISEG_REQUIRE(p->kind == MISEG_ENSEMBLE_MEAN_LOGITS || p->kind == MISEG_ENSEMBLE_MEAN_PROB || p->kind == MISEG_ENSEMBLE_VOTE, MISEG_E_BADARG,
                "ensemble_accumulate: unknown kind %d", p->kind);
  MISEG_REQUIRE(p->flip >= 0 && p->flip <= 7, MISEG_E_BADARG, "ensemble_accumulate: flip %d (bits 0..2)", p->flip);
  for (int c = 0; c < p->C; ++c) {
    MISEG_REQUIRE(isfinite(p->weight[c]) && p->weight[c] >= 0.f, MISEG_E_BADARG, "ensemble_accumulate: weight[%d] = %g is not finite and non-negative", c,
                  (double)p->weight[c]);
    MISEG_REQUIRE(!p->scaled || (isfinite(p->out_scale[c]) && p->out_scale[c] >= 0.f), MISEG_E_BADARG,
                  "ensemble_accumulate: out_scale[%d] = %g is not finite and non-negative", c, (double)p->out_scale[c]);
  }
  const unsigned __int128 elems = (unsigned __int128)p->B * p->C * ((unsigned __int128)p->D * p->H * p->W);
  const unsigned __int128 items = (unsigned __int128)p->B * p->D * ((unsigned __int128)p->H * ((p->W + 3ll) / 4));
  MISEG_REQUIRE(elems <= ((unsigned __int128)1 << 60) && items <= 0xffffffffull, MISEG_E_UNSUPPORTED,
                "ensemble_accumulate: shape [%d, %d, %d, %d, %d] is too large (B * D * H * ceil(W / 4) below 2^32)", p->B, p->C, p->D, p->H, p->W);
  const uintptr_t sb = (uintptr_t)p->src, ab = (uintptr_t)p->acc, bytes = (uintptr_t)elems * 4;
  MISEG_REQUIRE(sb + bytes <= ab || ab + bytes <= sb, MISEG_E_BADARG, "ensemble_accumulate: src and acc overlap (the fold is not in place)");
  MISEG_REQUIRE((sb & 3) == 0 && (ab & 3) == 0, MISEG_E_BADARG, "ensemble_accumulate: src / acc are not 4-byte aligned");
  EnsembleArgs a;
  a.B = p->B; a.C = p->C; a.D = p->D; a.H = p->H; a.W = p->W;
  a.nq = (p->W + 3) / 4;
  a.fd = p->flip & 1; a.fh = (p->flip >> 1) & 1; a.fw = (p->flip >> 2) & 1;
  a.first = p->first != 0; a.scaled = p->scaled != 0;
  a.vsrc = p->W % 4 == 0 && (sb & 15) == 0;
  a.vacc = p->W % 4 == 0 && (ab & 15) == 0;
  a.items = (int64_t)items;
  for (int c = 0; c < 64; ++c) {
    a.weight[c] = c < p->C ? p->weight[c] : 0.f;
    a.scale[c] = c < p->C && a.scaled ? p->out_scale[c] : 1.f;
  }
  // memory bound: at most 2048 workgroups walk the items with a grid stride
  const int grid = balanced_grid((a.items + 255) / 256, 2048);
  if (p->kind == MISEG_ENSEMBLE_MEAN_LOGITS) ensemble_logits_kernel<<<grid, 256, 0, s>>>(p->src, p->acc, a);
  else if (p->kind == MISEG_ENSEMBLE_MEAN_PROB) ensemble_cross_launch<MISEG_ENSEMBLE_MEAN_PROB>(grid, s, p->src, p->acc, a);
  else ensemble_cross_launch<MISEG_ENSEMBLE_VOTE>(grid, s, p->src, p->acc, a);
  MISEG_LAUNCH_CHECK("ensemble_accumulate");
  return MISEG_OK;
}
