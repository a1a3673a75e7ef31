// (Conditional) InstanceNorm and LayerNorm over channels-last rows -- HBM-bound kernels.
// Roofline: bytes only.  stats = 1 read of x; apply = 1 read (+1 residual) + 1 write;
// backward = reduce (dy, y, x reads) + apply (dy, y, x reads, dx [+dres] writes).
// Thread layout: tx owns one 16-byte channel vector for the whole block (its affine/statistics live in
// registers), ty walks rows, so every wave-instruction reads contiguous row segments.
#include <cstdlib>
#include "common.h"

namespace miseg {

#ifdef MISEG_NORM_STAMPS      // debug build (scripts/debug/norm_stamps.py): where a small norm launch spends its time, seen by thread 0 of workgroup 0
__device__ unsigned long long g_norm_stamps[16];
#define NSTAMP(i)                                                                                   \
  do {                                                                                              \
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {                \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                   \
      g_norm_stamps[i] = __builtin_readcyclecounter();                                              \
    }                                                                                               \
  } while (0)
#else
#define NSTAMP(i)
#endif

static constexpr int NORM_THREADS = 256;
static constexpr int NORM_TX_MAX = 32;   // channel vectors per block (wider rows are tiled over blockIdx.z)

template <class T, int VEC> struct RowVec {
  float v[VEC];
  __device__ __forceinline__ void load(const T* p) {
    if constexpr (VEC == 1) {
      v[0] = to_f32(p[0]);
    } else {
      typename Vec16<T>::type t = *reinterpret_cast<const typename Vec16<T>::type*>(p);
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = to_f32(t[i]);
    }
  }
  __device__ __forceinline__ void store(T* p) const {
    if constexpr (VEC == 1) {
      p[0] = from_f32<T>(v[0]);
    } else {
      typename Vec16<T>::type t;
#pragma unroll
      for (int i = 0; i < VEC; ++i) t[i] = from_f32<T>(v[i]);
      *reinterpret_cast<typename Vec16<T>::type*>(p) = t;
    }
  }
  __device__ __forceinline__ float get(int i) const { return v[i]; }
};

// one value's share of a channel's (sum, sum of squares)
__device__ __forceinline__ void stat_term(float v, float& s, float& q) {
  s += v;
  q = fmaf(v, v, q);
}

// Statistics buffers hold NORM_R replicas of the fp64 (sum, sum of squares) pairs: double [NORM_R][B][C][2].  A block adds
// its partial sums to replica (chunk mod NORM_R): with one row, the ~900 blocks of a 96^3 tensor queue on 96 addresses and
// the reduction costs 2x the streaming read (measured 49 us vs 15 us); consumers add the replicas up in their prologue.
static constexpr int NORM_R = 16;

// block-level reduction over ty of two per-thread vectors, then one fp64 atomic per (channel, which) -- no finalize
// kernel, no workspace.
template <int VEC>
__device__ __forceinline__ void block_reduce_to_stat(float* red, const float* s, const float* q, int tx, int ty, int tx_n, int ty_n, int c0, int C,
                                                     double* stat_b) {
  if (ty < ty_n) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      red[(ty * 2 + 0) * tx_n * VEC + tx * VEC + i] = s[i];
      red[(ty * 2 + 1) * tx_n * VEC + tx * VEC + i] = q[i];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * tx_n * VEC; e += NORM_THREADS) {
    const int which = e / (tx_n * VEC), col = e % (tx_n * VEC);
    float acc = 0.f;
    for (int y = 0; y < ty_n; ++y) acc += red[(y * 2 + which) * tx_n * VEC + col];
    const int ch = c0 * VEC + col;
    if (ch < C) atomicAdd(stat_b + 2 * ch + which, (double)acc);
  }
}

// workgroup prologue of the consumers: sums[(col) * 2 + which] = sum over replicas of stat[r][b][c0*VEC + col][which]
__device__ __forceinline__ void gather_stat(double* sums, const double* __restrict__ stat, int64_t rstride, int b, int C, int ch0, int ncols) {
  for (int e = threadIdx.x; e < 2 * ncols; e += NORM_THREADS) {
    const int ch = ch0 + (e >> 1);
    double acc = 0.0;
    if (ch < C) {
      const double* p = stat + ((int64_t)b * C + ch) * 2 + (e & 1);
#pragma unroll
      for (int r = 0; r < NORM_R; ++r) acc += p[r * rstride];
    }
    sums[e] = acc;
  }
  __syncthreads();
}

// mean and 1/sqrt(var + eps) of one channel; the variance is formed in fp64 (cancellation), the root in fp32
__device__ __forceinline__ void mean_rstd(double sum, double sumsq, double invS, float eps, float& m, float& rs) {
  const double mu = sum * invS;
  double var = fma(sumsq, invS, -mu * mu);
  if (var < 0.0) var = 0.0;
  m = (float)mu;
  rs = 1.0f / sqrtf((float)var + eps);
}

// ---------------------------------------------------------------------------------------------------
// The instance-norm arithmetic.  Every forward and backward kernel below is built from these pieces, so the scale / shift, the
// pre-activation and with them the LeakyReLU's sign are the same expressions, in the same order, in the forward and the backward pass.
// ---------------------------------------------------------------------------------------------------
struct StylePtrs {
  const float* gamma[MISEG_MAX_STYLES];
  const float* beta[MISEG_MAX_STYLES];
};
struct StyleGradPtrs {
  float* dgamma[MISEG_MAX_STYLES];
  float* dbeta[MISEG_MAX_STYLES];
};

// A workgroup keeps its tile's per-channel pairs of sums in LDS in one of two layouts:
//   gathered (gather_stat):  [col][2] with col = t * VEC + i                      the streaming kernels, the forward statistics of the fused backward
//   totals (fused_totals):   sum k of element i of channel vector t at [(k * VEC + i) * tx_n + t], sum 0 shared by all norms of the kernel
// LaneSums is one lane's view of either: element i has s[i * step] and q[i * step].
struct LaneSums {
  const double* s;
  const double* q;
  int step;
};
template <int VEC> __device__ __forceinline__ LaneSums gathered_sums(const double* sums, int tx) { return {sums + tx * VEC * 2, sums + tx * VEC * 2 + 1, 2}; }
template <int VEC> __device__ __forceinline__ LaneSums total_sums(const double* tot, int k, int tx, int tx_n) { return {tot + tx, tot + k * VEC * tx_n + tx, tx_n}; }

// per-lane coefficients of one norm: y = fma(x, sc, sh), xhat = (x - m) * rs
template <int VEC> struct NormCoef {
  float m[VEC], rs[VEC], sc[VEC], sh[VEC];
  // first half: request the style's affine values (sc, sh hold gamma, beta until finish()).  The fused kernels issue this before the statistics
  // are gathered, so that it is in flight with the rows.  Dead lanes of a ragged tile read the last channel vector (VEC divides C): one clamp
  // per lane keeps the VEC addresses consecutive.
  __device__ __forceinline__ void affine(const float* g, const float* b, int ch0, int C) {
    const int ch = min(ch0, C - VEC);
#pragma unroll
    for (int i = 0; i < VEC; ++i) sc[i] = g ? g[ch + i] : 1.f;      // (one loop per row: each null test then guards VEC loads, not one)
#pragma unroll
    for (int i = 0; i < VEC; ++i) sh[i] = b ? b[ch + i] : 0.f;
  }
  __device__ __forceinline__ void finish(const LaneSums& st, double invS, float eps) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      mean_rstd(st.s[i * st.step], st.q[i * st.step], invS, eps, m[i], rs[i]);
      sc[i] = rs[i] * sc[i];
      sh[i] = sh[i] - m[i] * sc[i];
    }
  }
  __device__ __forceinline__ void fill(const LaneSums& st, double invS, float eps, const float* g, const float* b, int ch0, int C) {
    affine(g, b, ch0, C);
    finish(st, invS, eps);
  }
  __device__ __forceinline__ void identity() {      // a residual that is added as it is
#pragma unroll
    for (int i = 0; i < VEC; ++i) { m[i] = 0.f; rs[i] = 1.f; sc[i] = 1.f; sh[i] = 0.f; }
  }
};

// what enters the activation: of one norm, and of the residual pair y = LeakyReLU(norm_a(xa) + norm_b(xb))
template <int VEC> __device__ __forceinline__ float preact(const NormCoef<VEC>& c, int i, float x) { return fmaf(x, c.sc[i], c.sh[i]); }
template <int VEC> __device__ __forceinline__ float pair_preact(const NormCoef<VEC>& ca, const NormCoef<VEC>& cb, int i, float xa, float xb) {
  float o = preact(ca, i, xa);
  o += preact(cb, i, xb);
  return o;
}

// the LeakyReLU's backward on one row g of the incoming gradient: out = g where the activation's input was positive, g * slope elsewhere
// (out may be g's own values).  sign(i) is anything with that input's sign: the stored output y (a residual that the kernel does not see
// entered the activation) or the pre-activation recomputed from the inputs - one tensor less to read.  The caller chooses between the two
// per ROW: inside the element loop that test was a scalar branch per element - 40 instructions per element, 3.8 us for 7 rows of a fused launch.
template <int VEC, class GRow, class Sign> __device__ __forceinline__ void leaky_mask(float (&out)[VEC], const GRow& g, Sign sign, float slope) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    const float gi = g.get(i);
    out[i] = sign(i) > 0.f ? gi : gi * slope;
  }
}

// backward sums of one row: q += g * xhat (sum g itself is shared by the norms of a pair and added by the kernel)
template <int VEC, class Row> __device__ __forceinline__ void bwd_sum_term(const NormCoef<VEC>& c, const float (&g)[VEC], const Row& x, float* q) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) q[i] = fmaf(g[i], (x.get(i) - c.m[i]) * c.rs[i], q[i]);
}
// the sample's mean of g, and of g * xhat, from the backward sums (a pair shares the first: both norms see the same g)
template <int VEC> __device__ __forceinline__ void bwd_mean_g(const LaneSums& d, double invS, float (&a)[VEC]) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) a[i] = (float)(d.s[i * d.step] * invS);
}
template <int VEC> __device__ __forceinline__ void bwd_mean_gxhat(const LaneSums& d, double invS, float (&bq)[VEC]) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) bq[i] = (float)(d.q[i * d.step] * invS);
}
template <int VEC> __device__ __forceinline__ float input_grad(const NormCoef<VEC>& c, int i, float g, float x, float a, float bq) {
  return c.sc[i] * (g - a - (x - c.m[i]) * c.rs[i] * bq);
}

// where column e of a workgroup's tile has its channel and its two sums, in the two layouts of LaneSums.  cv0: the tile's first channel vector;
// k: which of the totals holds this norm's g * xhat
template <int VEC> struct GatheredCols {
  int cv0;
  __device__ __forceinline__ void operator()(int e, int& ch, int& is, int& iq) const {
    ch = cv0 * VEC + e;
    is = 2 * e;
    iq = 2 * e + 1;
  }
};
template <int VEC> struct TotalCols {
  int cv0, tx_n, k;
  __device__ __forceinline__ void operator()(int e, int& ch, int& is, int& iq) const {
    const int i = e / tx_n, t = e - i * tx_n;
    ch = (cv0 + t) * VEC + i;
    is = e;
    iq = k * VEC * tx_n + e;
  }
};
// the affine gradients of one (sample, channel tile) of one norm: dgamma += sum g * xhat, dbeta += sum g
template <class Cols> __device__ __forceinline__ void add_affine_grads(const StyleGradPtrs& gp, int st, const double* sums, int ncols, int C, Cols cols) {
  float* dg = gp.dgamma[st];
  float* db = gp.dbeta[st];
  for (int e = threadIdx.x; e < ncols; e += NORM_THREADS) {
    int ch, is, iq;
    cols(e, ch, is, iq);
    if (ch < C) {
      if (dg) atomicAdd(dg + ch, (float)sums[iq]);
      if (db) atomicAdd(db + ch, (float)sums[is]);
    }
  }
}

// the row of a 1x1x1 convolution of a ONE-channel image (the stem block's shortcut), which is never stored: row[c] = round(r1x[row] * r1w[c]),
// formed exactly as the rank-1 GEMM would have rounded it
template <class T, int VEC> struct Rank1Row {
  float w[VEC];
  __device__ __forceinline__ void load(const T* r1w, int ch0, int C) {      // r1w == nullptr: no such shortcut
    const int ch = min(ch0, C - VEC);      // (dead lanes: as NormCoef::affine)
#pragma unroll
    for (int i = 0; i < VEC; ++i) w[i] = r1w ? to_f32(r1w[ch + i]) : 0.f;
  }
  __device__ __forceinline__ void form(float xs, RowVec<T, VEC>& row) const {
#pragma unroll
    for (int i = 0; i < VEC; ++i) row.v[i] = to_f32(from_f32<T>(xs * w[i]));
  }
};

// ---------------------------------------------------------------------------------------------------
// stats: stat[b][c] += (sum x, sum x^2) over this block's rows      grid (chunks, B, ctiles)
// ---------------------------------------------------------------------------------------------------
template <class T, int VEC>
__global__ void __launch_bounds__(NORM_THREADS) instnorm_stats_kernel(const T* __restrict__ x, int64_t ldx, int S, int C, int cv, int tx_n, int ty_n, int rpb,
                                                                      double* __restrict__ stat) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  const int b = blockIdx.y, chunk = blockIdx.x, c0 = blockIdx.z * tx_n;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int r0 = chunk * rpb, r1 = min(S, r0 + rpb);
  const T* xb = x + (int64_t)b * S * ldx;
  const int c = c0 + tx;
  float s[VEC], q[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = q[i] = 0.f;
  if (ty < ty_n && c < cv) {
    int r = r0 + ty;
    for (; r + 3 * ty_n < r1; r += 4 * ty_n) {   // 4 independent row loads in flight per lane
      RowVec<T, VEC> v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u].load(xb + (int64_t)(r + u * ty_n) * ldx + c * VEC);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < VEC; ++i) stat_term(v[u].v[i], s[i], q[i]);
    }
    for (; r < r1; r += ty_n) {
      RowVec<T, VEC> v;
      v.load(xb + (int64_t)r * ldx + c * VEC);
#pragma unroll
      for (int i = 0; i < VEC; ++i) stat_term(v.v[i], s[i], q[i]);
    }
  }
  block_reduce_to_stat<VEC>(red, s, q, tx, ty, tx_n, ty_n, c0, C, stat + ((int64_t)(chunk % NORM_R) * gridDim.y + b) * C * 2);
}

// The second launch of a convolution split over its input chunks (conv3d.hip: the small grids of the deep stages): y = round(sum of the
// fp32 slabs [+ res]) and, in the same pass, the instance-norm statistics of y - the split path used to leave them to a separate
// miseg_instnorm_stats launch over the tensor it had just written (one launch-and-drain latency per convolution of stages >= 3).
// Same thread geometry and replicated fp64 reduction as instnorm_stats_kernel; vector lanes read VEC floats of every slab.
template <class T, int VEC>
__global__ void __launch_bounds__(NORM_THREADS) slabs_to_out_stats_kernel(const float* __restrict__ slabs, int nslabs, int64_t slab_stride, T* __restrict__ y,
                                                                          int64_t ldy, const T* __restrict__ res, int64_t ldres, int S, int C, int cv, int tx_n,
                                                                          int ty_n, int rpb, double* __restrict__ stat) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  const int b = blockIdx.y, chunk = blockIdx.x, c0 = blockIdx.z * tx_n;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int r0 = chunk * rpb, r1 = min(S, r0 + rpb);
  const int c = c0 + tx;
  float s[VEC], q[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = q[i] = 0.f;
  if (ty < ty_n && c < cv) {
    for (int r = r0 + ty; r < r1; r += ty_n) {
      const int64_t row = (int64_t)b * S + r;
      float a[VEC];
      const float* p = slabs + row * C + c * VEC;
#pragma unroll
      for (int i = 0; i < VEC; ++i) a[i] = 0.f;
      if constexpr (VEC % 4 == 0) {
        for (int z0 = 0; z0 < nslabs; z0 += 4) {      // four slabs' loads in flight together (clamped: a repeated slab is not added)
          f32x4 v[4][VEC / 4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int z = min(z0 + u, nslabs - 1);
#pragma unroll
            for (int k = 0; k < VEC / 4; ++k) v[u][k] = *reinterpret_cast<const f32x4*>(p + z * slab_stride + 4 * k);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (z0 + u < nslabs) {
#pragma unroll
              for (int k = 0; k < VEC / 4; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) a[4 * k + e] += v[u][k][e];
            }
          }
        }
      } else {
        for (int z = 0; z < nslabs; ++z)
#pragma unroll
          for (int i = 0; i < VEC; ++i) a[i] += p[z * slab_stride + i];
      }
      RowVec<T, VEC> o;
      if (res) {
        o.load(res + row * ldres + c * VEC);
#pragma unroll
        for (int i = 0; i < VEC; ++i) a[i] += o.v[i];
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        o.v[i] = to_f32(from_f32<T>(a[i]));      // statistics of the stored (rounded) values, as miseg_instnorm_stats would read them
        stat_term(o.v[i], s[i], q[i]);
      }
      o.store(y + row * ldy + c * VEC);
    }
  }
  if (stat) block_reduce_to_stat<VEC>(red, s, q, tx, ty, tx_n, ty_n, c0, C, stat + ((int64_t)(chunk % NORM_R) * gridDim.y + b) * C * 2);
}

template <class T, int VEC>
__global__ void __launch_bounds__(NORM_THREADS) instnorm_apply_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ res, int64_t ldres,
                                                                      T* __restrict__ y, int64_t ldy, int S, int C, int cv, int tx_n, int ty_n, int rpb,
                                                                      const double* __restrict__ stat, float eps, const int32_t* __restrict__ styles,
                                                                      StylePtrs sp, int act, float slope, const double* __restrict__ rstat, StylePtrs rsp,
                                                                      const T* __restrict__ r1x, int64_t ldr1x, const T* __restrict__ r1w) {
  // rstat != nullptr: `res` is the RAW input of a second (shortcut) instance norm with its own statistics / affine rows and is
  // normalised on the fly: y = act(norm(x) + norm_r(res)) in one pass (UnetResBlock with a 1x1x1 shortcut conv, dynunet_block.py:118-124)
  // r1x != nullptr (with rstat, res == nullptr): that raw input is the 1x1x1 convolution of a ONE-channel image (the stem block) and is
  // not stored at all (Rank1Row)
  extern __shared__ __attribute__((aligned(16))) double sums[];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int c = blockIdx.z * tx_n + tx;
  double* rsums = sums + 2 * tx_n * VEC;
  gather_stat(sums, stat, (int64_t)gridDim.y * C * 2, b, C, blockIdx.z * tx_n * VEC, tx_n * VEC);
  if (rstat) gather_stat(rsums, rstat, (int64_t)gridDim.y * C * 2, b, C, blockIdx.z * tx_n * VEC, tx_n * VEC);
  if (ty >= ty_n || c >= cv) return;
  const int r0 = chunk * rpb, r1 = min(S, r0 + rpb);
  const int st = styles ? styles[b] : 0;
  const int64_t boff = (int64_t)b * S;
  const double invS = 1.0 / S;
  NormCoef<VEC> cx, cr;
  cx.fill(gathered_sums<VEC>(sums, tx), invS, eps, sp.gamma[st], sp.beta[st], c * VEC, C);
  if (rstat) cr.fill(gathered_sums<VEC>(rsums, tx), invS, eps, rsp.gamma[st], rsp.beta[st], c * VEC, C);
  else cr.identity();
  Rank1Row<T, VEC> rank1;
  rank1.load(r1x ? r1w : nullptr, c * VEC, C);
#pragma unroll 4
  for (int r = r0 + ty; r < r1; r += ty_n) {
    RowVec<T, VEC> v, o;
    v.load(x + (boff + r) * ldx + c * VEC);
    if (res || r1x) {
      RowVec<T, VEC> rr;
      if (res) rr.load(res + (boff + r) * ldres + c * VEC);
      else rank1.form(to_f32(r1x[(boff + r) * ldr1x]), rr);
#pragma unroll
      for (int i = 0; i < VEC; ++i) o.v[i] = pair_preact(cx, cr, i, v.v[i], rr.v[i]);
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) o.v[i] = preact(cx, i, v.v[i]);
    }
    if (act == MISEG_ACT_LEAKY) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) o.v[i] = o.v[i] > 0.f ? o.v[i] : o.v[i] * slope;
    }
    o.store(y + (boff + r) * ldy + c * VEC);
  }
}

// ---------------------------------------------------------------------------------------------------
// backward: reduce (sum dz, sum dz*xhat) -> dstat (fp64 atomics) ; apply (its chunk-0 workgroups also add the affine gradients)
// ---------------------------------------------------------------------------------------------------
template <class T, int VEC>
__global__ void __launch_bounds__(NORM_THREADS) instnorm_bwd_reduce_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ yact, int64_t ldy,
                                                                           const T* __restrict__ x, int64_t ldx, int S, int C, int cv, int tx_n, int ty_n, int rpb,
                                                                           const double* __restrict__ stat, float eps, int act, float slope,
                                                                           double* __restrict__ dstat, const int32_t* __restrict__ styles, StylePtrs sp) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  double* sums = reinterpret_cast<double*>(red);   // prologue only; the reduction reuses the space after a barrier
  const int b = blockIdx.y, chunk = blockIdx.x, c0 = blockIdx.z * tx_n;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int r0 = chunk * rpb, r1 = min(S, r0 + rpb);
  const int64_t boff = (int64_t)b * S;
  const int c = c0 + tx;
  gather_stat(sums, stat, (int64_t)gridDim.y * C * 2, b, C, c0 * VEC, tx_n * VEC);
  const int st = styles ? styles[b] : 0;
  NormCoef<VEC> cf;      // (its sc / sh: only to recompute the activation's sign)
  cf.fill(gathered_sums<VEC>(sums, tx), 1.0 / S, eps, sp.gamma[st], sp.beta[st], c * VEC, C);
  float s[VEC], q[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = q[i] = 0.f;
  __syncthreads();
  if (ty < ty_n && c < cv) {
#pragma unroll 4
    for (int r = r0 + ty; r < r1; r += ty_n) {
      RowVec<T, VEC> g, xv;
      g.load(dy + (boff + r) * lddy + c * VEC);
      xv.load(x + (boff + r) * ldx + c * VEC);
      if (act == MISEG_ACT_LEAKY) {
        if (yact) {
          RowVec<T, VEC> yv;
          yv.load(yact + (boff + r) * ldy + c * VEC);
          leaky_mask(g.v, g, [&](int i) { return yv.v[i]; }, slope);
        } else {
          leaky_mask(g.v, g, [&](int i) { return preact(cf, i, xv.v[i]); }, slope);
        }
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] += g.v[i];
      bwd_sum_term(cf, g.v, xv, q);
    }
  }
  block_reduce_to_stat<VEC>(red, s, q, tx, ty, tx_n, ty_n, c0, C, dstat + ((int64_t)(chunk % NORM_R) * gridDim.y + b) * C * 2);
}

template <class T, int VEC>
__global__ void __launch_bounds__(NORM_THREADS) instnorm_bwd_apply_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ yact, int64_t ldy,
                                                                          const T* __restrict__ x, int64_t ldx, T* __restrict__ dx, int64_t lddx,
                                                                          T* __restrict__ dres, int64_t lddres, int S, int C, int cv, int tx_n, int ty_n, int rpb,
                                                                          const double* __restrict__ stat, float eps, const int32_t* __restrict__ styles,
                                                                          StylePtrs sp, int act, float slope, const double* __restrict__ dstat, StyleGradPtrs gp,
                                                                          const T* __restrict__ gadd, int64_t ldgadd) {
  extern __shared__ __attribute__((aligned(16))) double sums[];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int c = blockIdx.z * tx_n + tx;
  double* dsums = sums + 2 * tx_n * VEC;
  gather_stat(sums, stat, (int64_t)gridDim.y * C * 2, b, C, blockIdx.z * tx_n * VEC, tx_n * VEC);
  gather_stat(dsums, dstat, (int64_t)gridDim.y * C * 2, b, C, blockIdx.z * tx_n * VEC, tx_n * VEC);
  const int st = styles ? styles[b] : 0;
  if (chunk == 0) add_affine_grads(gp, st, dsums, tx_n * VEC, C, GatheredCols<VEC>{(int)blockIdx.z * tx_n});
  if (ty >= ty_n || c >= cv) return;
  const int r0 = chunk * rpb, r1 = min(S, r0 + rpb);
  const int64_t boff = (int64_t)b * S;
  const double invS = 1.0 / S;
  NormCoef<VEC> cf;
  cf.fill(gathered_sums<VEC>(sums, tx), invS, eps, sp.gamma[st], sp.beta[st], c * VEC, C);
  float a[VEC], bq[VEC];
  bwd_mean_g(gathered_sums<VEC>(dsums, tx), invS, a);
  bwd_mean_gxhat(gathered_sums<VEC>(dsums, tx), invS, bq);
#pragma unroll 4
  for (int r = r0 + ty; r < r1; r += ty_n) {
    RowVec<T, VEC> gv, xv, o;
    gv.load(dy + (boff + r) * lddy + c * VEC);
    xv.load(x + (boff + r) * ldx + c * VEC);
    if (act == MISEG_ACT_LEAKY) {
      if (yact) {
        RowVec<T, VEC> yv;
        yv.load(yact + (boff + r) * ldy + c * VEC);
        leaky_mask(gv.v, gv, [&](int i) { return yv.v[i]; }, slope);
      } else {
        leaky_mask(gv.v, gv, [&](int i) { return preact(cf, i, xv.v[i]); }, slope);
      }
    }
    if (dres) gv.store(dres + (boff + r) * lddres + c * VEC);
#pragma unroll
    for (int i = 0; i < VEC; ++i) o.v[i] = input_grad(cf, i, gv.v[i], xv.v[i], a[i], bq[i]);
    if (gadd) {
      RowVec<T, VEC> ga;
      ga.load(gadd + (boff + r) * ldgadd + c * VEC);
#pragma unroll
      for (int i = 0; i < VEC; ++i) o.v[i] += ga.v[i];
    }
    o.store(dx + (boff + r) * lddx + c * VEC);
  }
}

// ---- backward of y = LeakyReLU(norm_a(xa) + norm_b(xb)) (instnorm_apply_kernel with rstat): both norms see the same activation-
// masked gradient g, so ONE reduction pass yields sum g, sum g*xhat_a, sum g*xhat_b and ONE apply pass writes both input gradients
// (10 passes over the tensor instead of the 13 of two chained norm backwards, no `dres` tensor, two launches instead of four).

template <class T, int VEC>
__global__ void __launch_bounds__(NORM_THREADS) instnorm_pair_bwd_reduce_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ yact, int64_t ldy,
                                                                                const T* __restrict__ xa, int64_t ldxa, const T* __restrict__ xb, int64_t ldxb,
                                                                                int S, int C, int cv, int tx_n, int ty_n, int rpb,
                                                                                const double* __restrict__ stat_a, const double* __restrict__ stat_b, float eps,
                                                                                float slope, double* __restrict__ dstat_a, double* __restrict__ dstat_b,
                                                                                const int32_t* __restrict__ styles, StylePtrs spa, StylePtrs spb,
                                                                                const T* __restrict__ r1x, int64_t ldr1x, const T* __restrict__ r1w) {
  // r1x != nullptr: xb is not stored (Rank1Row)
  // yact == nullptr: the LeakyReLU's sign is recomputed from the two inputs (pair_preact, as the forward formed it) - one tensor less to
  // read in both passes
  extern __shared__ __attribute__((aligned(16))) float red[];
  double* sums_a = reinterpret_cast<double*>(red);   // prologue only; the reductions reuse the space after a barrier
  double* sums_b = sums_a + 2 * tx_n * VEC;
  const int b = blockIdx.y, chunk = blockIdx.x, c0 = blockIdx.z * tx_n;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int r0 = chunk * rpb, r1 = min(S, r0 + rpb);
  const int64_t boff = (int64_t)b * S;
  const int c = c0 + tx;
  gather_stat(sums_a, stat_a, (int64_t)gridDim.y * C * 2, b, C, c0 * VEC, tx_n * VEC);
  gather_stat(sums_b, stat_b, (int64_t)gridDim.y * C * 2, b, C, c0 * VEC, tx_n * VEC);
  const double invS = 1.0 / S;
  const int st = styles ? styles[b] : 0;
  NormCoef<VEC> ca, cb;
  ca.fill(gathered_sums<VEC>(sums_a, tx), invS, eps, spa.gamma[st], spa.beta[st], c * VEC, C);
  cb.fill(gathered_sums<VEC>(sums_b, tx), invS, eps, spb.gamma[st], spb.beta[st], c * VEC, C);
  Rank1Row<T, VEC> rank1;
  rank1.load(r1x ? r1w : nullptr, c * VEC, C);
  float s[VEC], qa[VEC], qb[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = qa[i] = qb[i] = 0.f;
  __syncthreads();
  if (ty < ty_n && c < cv) {
#pragma unroll 4
    for (int r = r0 + ty; r < r1; r += ty_n) {
      RowVec<T, VEC> g, yv, va, vb;
      g.load(dy + (boff + r) * lddy + c * VEC);
      if (yact) yv.load(yact + (boff + r) * ldy + c * VEC);
      va.load(xa + (boff + r) * ldxa + c * VEC);
      if (r1x) rank1.form(to_f32(r1x[(boff + r) * ldr1x]), vb);
      else vb.load(xb + (boff + r) * ldxb + c * VEC);
      // (a select per element, not a branch per row: with the branch the compiler keeps two copies of the unrolled loop's registers - 138
      // against 111 for fp32 lanes, one wave per SIMD less)
      leaky_mask(g.v, g, [&](int i) { return yact ? yv.v[i] : pair_preact(ca, cb, i, va.v[i], vb.v[i]); }, slope);
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] += g.v[i];
      bwd_sum_term(ca, g.v, va, qa);
      bwd_sum_term(cb, g.v, vb, qb);
    }
  }
  block_reduce_to_stat<VEC>(red, s, qa, tx, ty, tx_n, ty_n, c0, C, dstat_a + ((int64_t)(chunk % NORM_R) * gridDim.y + b) * C * 2);
  __syncthreads();
  block_reduce_to_stat<VEC>(red, s, qb, tx, ty, tx_n, ty_n, c0, C, dstat_b + ((int64_t)(chunk % NORM_R) * gridDim.y + b) * C * 2);
}

template <class T, int VEC>
__global__ void __launch_bounds__(NORM_THREADS) instnorm_pair_bwd_apply_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ yact, int64_t ldy,
                                                                               const T* __restrict__ xa, int64_t ldxa, const T* __restrict__ xb, int64_t ldxb,
                                                                               T* __restrict__ dxa, int64_t lddxa, T* __restrict__ dxb, int64_t lddxb, int S, int C,
                                                                               int cv, int tx_n, int ty_n, int rpb, const double* __restrict__ stat_a,
                                                                               const double* __restrict__ stat_b, float eps, const int32_t* __restrict__ styles,
                                                                               StylePtrs spa, StylePtrs spb, float slope, const double* __restrict__ dstat_a,
                                                                               const double* __restrict__ dstat_b, StyleGradPtrs gpa, StyleGradPtrs gpb,
                                                                               const T* __restrict__ r1x, int64_t ldr1x, const T* __restrict__ r1w,
                                                                               float* __restrict__ r1dw) {
  // r1x != nullptr: xb = round(r1x[row] * r1w[c]) is not stored (see instnorm_apply_kernel) and neither is its gradient: the only consumer
  // is the weight gradient of that 1x1x1 convolution, dW[c] += sum over rows of round(dxb[row][c]) * r1x[row], reduced here
  extern __shared__ __attribute__((aligned(16))) double sums[];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int c = blockIdx.z * tx_n + tx;
  const int nc = 2 * tx_n * VEC;
  double* sa = sums;
  double* sb = sums + nc;
  double* da = sums + 2 * nc;
  double* db = sums + 3 * nc;
  gather_stat(sa, stat_a, (int64_t)gridDim.y * C * 2, b, C, blockIdx.z * tx_n * VEC, tx_n * VEC);
  gather_stat(sb, stat_b, (int64_t)gridDim.y * C * 2, b, C, blockIdx.z * tx_n * VEC, tx_n * VEC);
  gather_stat(da, dstat_a, (int64_t)gridDim.y * C * 2, b, C, blockIdx.z * tx_n * VEC, tx_n * VEC);
  gather_stat(db, dstat_b, (int64_t)gridDim.y * C * 2, b, C, blockIdx.z * tx_n * VEC, tx_n * VEC);
  const int st = styles ? styles[b] : 0;
  if (chunk == 0) {
    add_affine_grads(gpa, st, da, tx_n * VEC, C, GatheredCols<VEC>{(int)blockIdx.z * tx_n});
    add_affine_grads(gpb, st, db, tx_n * VEC, C, GatheredCols<VEC>{(int)blockIdx.z * tx_n});
  }
  const bool live = ty < ty_n && c < cv;
  if (!live && !r1x) return;
  // the rank-1 weight gradient all but vanishes (the norm behind the 1x1x1 convolution removes its scale): thousands of terms that cancel a
  // thousandfold.  The per-thread chains and the workgroup's column sums run in float64 (fp32 chains left single elements 1e-4 of the
  // gradient's scale off, differently from run to run); one fp32 atomic per channel and workgroup remains.
  double dwacc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) dwacc[i] = 0.0;
  if (live) {
    const int r0 = chunk * rpb, r1 = min(S, r0 + rpb);
    const int64_t boff = (int64_t)b * S;
    const double invS = 1.0 / S;
    NormCoef<VEC> ca, cb;
    ca.fill(gathered_sums<VEC>(sa, tx), invS, eps, spa.gamma[st], spa.beta[st], c * VEC, C);
    cb.fill(gathered_sums<VEC>(sb, tx), invS, eps, spb.gamma[st], spb.beta[st], c * VEC, C);
    float aa[VEC], bqa[VEC], bqb[VEC];
    bwd_mean_g(gathered_sums<VEC>(da, tx), invS, aa);
    bwd_mean_gxhat(gathered_sums<VEC>(da, tx), invS, bqa);
    bwd_mean_gxhat(gathered_sums<VEC>(db, tx), invS, bqb);
    Rank1Row<T, VEC> rank1;
    rank1.load(r1x ? r1w : nullptr, c * VEC, C);
#pragma unroll 4
    for (int r = r0 + ty; r < r1; r += ty_n) {
      RowVec<T, VEC> g, yv, va, vb, oa, ob;
      g.load(dy + (boff + r) * lddy + c * VEC);
      if (yact) yv.load(yact + (boff + r) * ldy + c * VEC);
      va.load(xa + (boff + r) * ldxa + c * VEC);
      float xs = 0.f;
      if (r1x) {
        xs = to_f32(r1x[(boff + r) * ldr1x]);
        rank1.form(xs, vb);
      } else {
        vb.load(xb + (boff + r) * ldxb + c * VEC);
      }
      leaky_mask(g.v, g, [&](int i) { return yact ? yv.v[i] : pair_preact(ca, cb, i, va.v[i], vb.v[i]); }, slope);      // (as in the reduce kernel)
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        oa.v[i] = input_grad(ca, i, g.v[i], va.v[i], aa[i], bqa[i]);
        ob.v[i] = input_grad(cb, i, g.v[i], vb.v[i], aa[i], bqb[i]);
      }
      oa.store(dxa + (boff + r) * lddxa + c * VEC);
      if (r1x) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) dwacc[i] = fma((double)to_f32(from_f32<T>(ob.v[i])), (double)xs, dwacc[i]);
      } else {
        ob.store(dxb + (boff + r) * lddxb + c * VEC);
      }
    }
  }
  if (r1x) {     // every thread of the workgroup is here: column sums of dwacc over ty, one fp32 atomic per channel and workgroup
    float* redf = reinterpret_cast<float*>(sums);
    __syncthreads();       // the statistics in `sums` have been read by everyone
    if (ty < ty_n) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) redf[(ty * tx_n + tx) * VEC + i] = (float)dwacc[i];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < tx_n * VEC; e += NORM_THREADS) {
      const int ch = blockIdx.z * tx_n * VEC + e;
      double tot = 0.0;
      for (int t = 0; t < ty_n; ++t) tot += (double)redf[t * tx_n * VEC + e];
      if (ch < C) atomicAdd(r1dw + ch, (float)tot);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Register-resident fused kernels (round 3): tensors of up to NORM_FUSED_MAX_ROWS = 2048 rows per sample (the 12^3, 6^3 and 3^3 stages).
// One workgroup per (sample, tile of tx_n channel vectors); thread (tx, ty) owns rows ty, ty + ty_n, ... - at most FUSED_MAXR of them - of
// its channel vector and keeps them IN REGISTERS (packed, 4 registers per 16-byte row): every tensor is read exactly once, all its loads are
// in flight together and are issued BEFORE the statistics are gathered, the reduction over the rows is a cross-lane step + one LDS round
// across the four waves, and the second pass (normalise / the input gradient) runs from the registers.  The round-2 kernels walked the rows
// twice with four loads in flight behind the statistics gather (6.5 - 11 us for 166 KB); the chunked pairs they replace at 12^3 were
// two launches with an fp64-atomic hand-off between them (8 + 8 us).
// ---------------------------------------------------------------------------------------------------
static constexpr int FUSED_MAXR = 8;
static constexpr int NORM_FUSED_MAX_ROWS = FUSED_MAXR * NORM_THREADS;

template <class T, int VEC> struct PRow {       // one row's VEC channels of a lane as loaded (packed: VEC * sizeof(T) bytes, one load)
  typedef T raw_t __attribute__((ext_vector_type(VEC)));
  raw_t raw;
  __device__ __forceinline__ void load(const T* p) { raw = *reinterpret_cast<const raw_t*>(p); }
  __device__ __forceinline__ void store(T* p) const { *reinterpret_cast<raw_t*>(p) = raw; }
  __device__ __forceinline__ float get(int i) const { return to_f32(raw[i]); }
  __device__ __forceinline__ void set(int i, float v) { raw[i] = from_f32<T>(v); }
};
template <class T> struct PRow<T, 1> {
  T raw;
  __device__ __forceinline__ void load(const T* p) { raw = p[0]; }
  __device__ __forceinline__ void store(T* p) const { p[0] = raw; }
  __device__ __forceinline__ float get(int) const { return to_f32(raw); }
  __device__ __forceinline__ void set(int, float v) { raw = from_f32<T>(v); }
};

// totals over the ty rows of the workgroup of NVV per-thread floats.  thread = ty * tx_n + tx with tx_n a power of two <= 16, so the lanes of
// a 16-lane DPP row that share tx are those congruent modulo tx_n: rotations of the row by 8, 4, .. tx_n (plain VALU instructions with a DPP
// operand - the xor shuffles of the first version went through the LDS crossbar, 1.3 - 2.1 us of a 10 us launch) leave every lane with
// its class's row total; the 16 rows of the workgroup then meet in LDS.  tot[k * tx_n + tx] (double) is valid for every thread afterwards.
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int NVV>
__device__ __forceinline__ void fused_totals(float (&v)[NVV], float* red, double* tot, int tx_n) {
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 4;
  if (tx_n <= 8) {
#pragma unroll
    for (int k = 0; k < NVV; ++k) v[k] = dpp_add<0x128>(v[k]);      // row_ror:8
  }
  if (tx_n <= 4) {
#pragma unroll
    for (int k = 0; k < NVV; ++k) v[k] = dpp_add<0x124>(v[k]);      // row_ror:4
  }
  if (tx_n <= 2) {
#pragma unroll
    for (int k = 0; k < NVV; ++k) v[k] = dpp_add<0x122>(v[k]);      // row_ror:2
  }
  if (tx_n <= 1) {
#pragma unroll
    for (int k = 0; k < NVV; ++k) v[k] = dpp_add<0x121>(v[k]);      // row_ror:1
  }
  if ((lane & 15) < tx_n) {
#pragma unroll
    for (int k = 0; k < NVV; ++k) red[(row * NVV + k) * tx_n + (lane & 15)] = v[k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NVV * tx_n; e += NORM_THREADS) {
    double acc = 0.0;
#pragma unroll
    for (int w = 0; w < NORM_THREADS / 16; ++w) acc += (double)red[w * NVV * tx_n + e];
    tot[e] = acc;
  }
  __syncthreads();
}

template <int VEC> __device__ __forceinline__ void add_floats(const float* __restrict__ p, float (&a)[VEC]) {
  if constexpr (VEC % 4 == 0) {
#pragma unroll
    for (int j = 0; j < VEC / 4; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * j);
      a[4 * j] += v[0]; a[4 * j + 1] += v[1]; a[4 * j + 2] += v[2]; a[4 * j + 3] += v[3];
    }
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) a[j] += p[j];
  }
}
// row = round(sum of this lane's elements of `nslabs` fp32 partial slabs): the output of a split convolution, formed by its consumer
template <class T, int VEC> __device__ __forceinline__ void sum_slabs(PRow<T, VEC>& row, const float* __restrict__ p, int nslabs, int64_t slab_stride) {
  float a[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) a[i] = 0.f;
  for (int k = 0; k < nslabs; ++k) add_floats<VEC>(p + k * slab_stride, a);
#pragma unroll
  for (int i = 0; i < VEC; ++i) row.set(i, a[i]);
}

// SLABS: the input is still the `nslabs` fp32 partial slabs [B * S][C] of a split convolution (miseg_conv3_params.defer_slabs): a lane sums
// its elements, rounds them to T - that IS the convolution's output, written to x for the backward pass - and goes on as below.  One launch
// where the split convolution's reduce launch and the norm's apply launch were two (the <= 2048-row layers of the deep stages).
template <class T, int VEC, bool SLABS = false>
__global__ void __launch_bounds__(NORM_THREADS) instnorm_fused_fwd_kernel(T* __restrict__ x, int64_t ldx, const T* __restrict__ res, int64_t ldres,
                                                                          T* __restrict__ y, int64_t ldy, int S, int C, int cv, int tx_n, int ty_n,
                                                                          double* __restrict__ stat, float eps, const int32_t* __restrict__ styles, StylePtrs sp,
                                                                          int act, float slope, const float* __restrict__ slabs = nullptr, int nslabs = 0,
                                                                          int64_t slab_stride = 0) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  double* tot = reinterpret_cast<double*>(red + (NORM_THREADS / 16) * 2 * VEC * tx_n);
  const int b = blockIdx.y;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int c = blockIdx.x * tx_n + tx;
  const bool live = c < cv;
  const int64_t boff = (int64_t)b * S;
  // (style id and affine rows are requested first: they are in flight with the rows)
  const int st = styles ? styles[b] : 0;
  NormCoef<VEC> cf;
  cf.affine(sp.gamma[st], sp.beta[st], c * VEC, C);
  PRow<T, VEC> xr[FUSED_MAXR], rr[FUSED_MAXR];
  if constexpr (SLABS) {
#pragma unroll
    for (int u = 0; u < FUSED_MAXR; ++u) {
      const int r = ty + u * ty_n;
      if (live && r < S) {
        sum_slabs(xr[u], slabs + (boff + r) * (int64_t)C + c * VEC, nslabs, slab_stride);
        xr[u].store(x + (boff + r) * ldx + c * VEC);
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < FUSED_MAXR; ++u) {
      const int r = ty + u * ty_n;
      if (live && r < S) xr[u].load(x + (boff + r) * ldx + c * VEC);
    }
  }
  if (res) {
#pragma unroll
    for (int u = 0; u < FUSED_MAXR; ++u) {
      const int r = ty + u * ty_n;
      if (live && r < S) rr[u].load(res + (boff + r) * ldres + c * VEC);
    }
  }
  float sq[2 * VEC];
#pragma unroll
  for (int i = 0; i < 2 * VEC; ++i) sq[i] = 0.f;
#pragma unroll
  for (int u = 0; u < FUSED_MAXR; ++u) {
    if (live && ty + u * ty_n < S) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) stat_term(xr[u].get(i), sq[i], sq[VEC + i]);
    }
  }
  fused_totals<2 * VEC>(sq, red, tot, tx_n);      // tot[(which * VEC + i) * tx_n + tx]
  // replica 0 of the statistics buffer (the others stay zero): the backward pass reads it like any other
  for (int e = threadIdx.x; e < 2 * VEC * tx_n; e += NORM_THREADS) {
    const int k = e / tx_n, t = e - k * tx_n, which = k / VEC, i = k - which * VEC;
    const int ch = (blockIdx.x * tx_n + t) * VEC + i;
    if (ch < C) stat[((int64_t)b * C + ch) * 2 + which] = tot[e];
  }
  if (!live) return;
  cf.finish(total_sums<VEC>(tot, 1, tx, tx_n), 1.0 / S, eps);
#pragma unroll
  for (int u = 0; u < FUSED_MAXR; ++u) {
    const int r = ty + u * ty_n;
    if (r < S) {
      float v[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = preact(cf, i, xr[u].get(i));
      if (res) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] += rr[u].get(i);
      }
      if (act == MISEG_ACT_LEAKY) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = v[i] > 0.f ? v[i] : v[i] * slope;
      }
      PRow<T, VEC> o;
#pragma unroll
      for (int i = 0; i < VEC; ++i) o.set(i, v[i]);
      o.store(y + (boff + r) * ldy + c * VEC);
    }
  }
}

// SLABS: dy is still the `nslabs` fp32 partial slabs of the split data-gradient convolution in front of this norm (see the forward kernel):
// summed and rounded to T in registers - the incoming gradient is never written to memory at all.
template <class T, int VEC, bool SLABS = false>
__global__ void __launch_bounds__(NORM_THREADS) instnorm_fused_bwd_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ yact, int64_t ldy,
                                                                          const T* __restrict__ x, int64_t ldx, T* __restrict__ dx, int64_t lddx,
                                                                          T* __restrict__ dres, int64_t lddres, int S, int C, int cv, int tx_n, int ty_n,
                                                                          const double* __restrict__ stat, float eps, const int32_t* __restrict__ styles,
                                                                          StylePtrs sp, StyleGradPtrs gp, int act, float slope, const T* __restrict__ gadd,
                                                                          int64_t ldgadd, const float* __restrict__ slabs = nullptr, int nslabs = 0,
                                                                          int64_t slab_stride = 0) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  double* tot = reinterpret_cast<double*>(red + (NORM_THREADS / 16) * 2 * VEC * tx_n);   // totals of (g, g * xhat)
  double* sums = tot + 2 * VEC * tx_n;                                                  // forward statistics [col][2]
  const int b = blockIdx.y;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int c = blockIdx.x * tx_n + tx;
  const bool live = c < cv;
  const int64_t boff = (int64_t)b * S;
  const bool masked = act == MISEG_ACT_LEAKY;
  NSTAMP(0);
  // style id, affine rows and all row loads first: nothing below depends on them until the statistics have arrived as well
  const int st = styles ? styles[b] : 0;
  const bool from_y = masked && yact;      // a residual entered the activation: its sign comes from the stored output
  NormCoef<VEC> cf;
  cf.affine(sp.gamma[st], (masked && !yact) ? sp.beta[st] : nullptr, c * VEC, C);      // (the shift: only to recompute the activation's sign)
  PRow<T, VEC> gr[FUSED_MAXR], xr[FUSED_MAXR], yr[FUSED_MAXR];
#pragma unroll
  for (int u = 0; u < FUSED_MAXR; ++u) {
    const int r = ty + u * ty_n;
    if (live && r < S) {
      if constexpr (SLABS) sum_slabs(gr[u], slabs + (boff + r) * (int64_t)C + c * VEC, nslabs, slab_stride);
      else gr[u].load(dy + (boff + r) * lddy + c * VEC);
      xr[u].load(x + (boff + r) * ldx + c * VEC);
      if (from_y) yr[u].load(yact + (boff + r) * ldy + c * VEC);
    }
  }
  NSTAMP(1);
  gather_stat(sums, stat, (int64_t)gridDim.y * C * 2, b, C, blockIdx.x * tx_n * VEC, tx_n * VEC);
  NSTAMP(2);
  const double invS = 1.0 / S;
  cf.finish(gathered_sums<VEC>(sums, tx), invS, eps);
  // the activation-masked gradient of row u; evaluated in both passes (three instructions per element) rather than stored
  auto gmask = [&](int u, float (&gm)[VEC]) {
    if (from_y) {
      leaky_mask(gm, gr[u], [&](int i) { return yr[u].get(i); }, slope);
    } else if (masked) {
      leaky_mask(gm, gr[u], [&](int i) { return preact(cf, i, xr[u].get(i)); }, slope);
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) gm[i] = gr[u].get(i);
    }
  };
  float sq[2 * VEC];
#pragma unroll
  for (int i = 0; i < 2 * VEC; ++i) sq[i] = 0.f;
#pragma unroll
  for (int u = 0; u < FUSED_MAXR; ++u) {
    if (live && ty + u * ty_n < S) {
      float gm[VEC];
      gmask(u, gm);
#pragma unroll
      for (int i = 0; i < VEC; ++i) sq[i] += gm[i];
      bwd_sum_term(cf, gm, xr[u], sq + VEC);
    }
  }
  NSTAMP(3);
  fused_totals<2 * VEC>(sq, red, tot, tx_n);
  NSTAMP(4);
  add_affine_grads(gp, st, tot, tx_n * VEC, C, TotalCols<VEC>{(int)blockIdx.x * tx_n, tx_n, 1});
  NSTAMP(5);
  if (!live) return;
  float a[VEC], bq[VEC];
  bwd_mean_g(total_sums<VEC>(tot, 1, tx, tx_n), invS, a);
  bwd_mean_gxhat(total_sums<VEC>(tot, 1, tx, tx_n), invS, bq);
#pragma unroll
  for (int u = 0; u < FUSED_MAXR; ++u) {
    const int r = ty + u * ty_n;
    if (r < S) {
      float gm[VEC], v[VEC];
      gmask(u, gm);
      if (dres) {
        PRow<T, VEC> dr;
#pragma unroll
        for (int i = 0; i < VEC; ++i) dr.set(i, gm[i]);
        dr.store(dres + (boff + r) * lddres + c * VEC);
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = input_grad(cf, i, gm[i], xr[u].get(i), a[i], bq[i]);
      if (gadd) {
        PRow<T, VEC> ga;
        ga.load(gadd + (boff + r) * ldgadd + c * VEC);
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] += ga.get(i);
      }
      PRow<T, VEC> o;
#pragma unroll
      for (int i = 0; i < VEC; ++i) o.set(i, v[i]);
      o.store(dx + (boff + r) * lddx + c * VEC);
    }
  }
  NSTAMP(6);
}

// backward of y = LeakyReLU(norm_a(xa) + norm_b(xb)) in ONE launch (see instnorm_pair_bwd_{reduce,apply}_kernel for the arithmetic):
// dy, xa, xb stay in registers, the three sums (g, g * xhat_a, g * xhat_b) meet inside the workgroup.
template <class T, int VEC>
__global__ void __launch_bounds__(NORM_THREADS) instnorm_pair_fused_bwd_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ yact, int64_t ldy,
                                                                               const T* __restrict__ xa, int64_t ldxa, const T* __restrict__ xb, int64_t ldxb,
                                                                               T* __restrict__ dxa, int64_t lddxa, T* __restrict__ dxb, int64_t lddxb, int S, int C,
                                                                               int cv, int tx_n, int ty_n, const double* __restrict__ stat_a,
                                                                               const double* __restrict__ stat_b, float eps, const int32_t* __restrict__ styles,
                                                                               StylePtrs spa, StylePtrs spb, float slope, StyleGradPtrs gpa, StyleGradPtrs gpb) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  double* tot = reinterpret_cast<double*>(red + (NORM_THREADS / 16) * 3 * VEC * tx_n);   // totals of (g, g * xhat_a, g * xhat_b)
  double* sums_a = tot + 3 * VEC * tx_n;
  double* sums_b = sums_a + 2 * VEC * tx_n;
  const int b = blockIdx.y;
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int c = blockIdx.x * tx_n + tx;
  const bool live = c < cv;
  const int64_t boff = (int64_t)b * S;
  // style id + affine rows first (in flight with the rows)
  const int st = styles ? styles[b] : 0;
  NormCoef<VEC> ca, cb;
  ca.affine(spa.gamma[st], spa.beta[st], c * VEC, C);
  cb.affine(spb.gamma[st], spb.beta[st], c * VEC, C);
  PRow<T, VEC> gr[FUSED_MAXR], ar[FUSED_MAXR], br[FUSED_MAXR], yr[FUSED_MAXR];
#pragma unroll
  for (int u = 0; u < FUSED_MAXR; ++u) {
    const int r = ty + u * ty_n;
    if (live && r < S) {
      gr[u].load(dy + (boff + r) * lddy + c * VEC);
      ar[u].load(xa + (boff + r) * ldxa + c * VEC);
      br[u].load(xb + (boff + r) * ldxb + c * VEC);
      if (yact) yr[u].load(yact + (boff + r) * ldy + c * VEC);
    }
  }
  gather_stat(sums_a, stat_a, (int64_t)gridDim.y * C * 2, b, C, blockIdx.x * tx_n * VEC, tx_n * VEC);
  gather_stat(sums_b, stat_b, (int64_t)gridDim.y * C * 2, b, C, blockIdx.x * tx_n * VEC, tx_n * VEC);
  const double invS = 1.0 / S;
  ca.finish(gathered_sums<VEC>(sums_a, tx), invS, eps);
  cb.finish(gathered_sums<VEC>(sums_b, tx), invS, eps);
  auto gmask = [&](int u, float (&gm)[VEC]) {
    if (yact) leaky_mask(gm, gr[u], [&](int i) { return yr[u].get(i); }, slope);
    else leaky_mask(gm, gr[u], [&](int i) { return pair_preact(ca, cb, i, ar[u].get(i), br[u].get(i)); }, slope);
  };
  float sq[3 * VEC];
#pragma unroll
  for (int i = 0; i < 3 * VEC; ++i) sq[i] = 0.f;
#pragma unroll
  for (int u = 0; u < FUSED_MAXR; ++u) {
    if (live && ty + u * ty_n < S) {
      float gm[VEC];
      gmask(u, gm);
#pragma unroll
      for (int i = 0; i < VEC; ++i) sq[i] += gm[i];
      bwd_sum_term(ca, gm, ar[u], sq + VEC);
      bwd_sum_term(cb, gm, br[u], sq + 2 * VEC);
    }
  }
  fused_totals<3 * VEC>(sq, red, tot, tx_n);
  add_affine_grads(gpa, st, tot, tx_n * VEC, C, TotalCols<VEC>{(int)blockIdx.x * tx_n, tx_n, 1});
  add_affine_grads(gpb, st, tot, tx_n * VEC, C, TotalCols<VEC>{(int)blockIdx.x * tx_n, tx_n, 2});
  if (!live) return;
  float aa[VEC], bqa[VEC], bqb[VEC];
  bwd_mean_g(total_sums<VEC>(tot, 1, tx, tx_n), invS, aa);
  bwd_mean_gxhat(total_sums<VEC>(tot, 1, tx, tx_n), invS, bqa);
  bwd_mean_gxhat(total_sums<VEC>(tot, 2, tx, tx_n), invS, bqb);
#pragma unroll
  for (int u = 0; u < FUSED_MAXR; ++u) {
    const int r = ty + u * ty_n;
    if (r < S) {
      PRow<T, VEC> oa, ob;
      float gm[VEC];
      gmask(u, gm);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        oa.set(i, input_grad(ca, i, gm[i], ar[u].get(i), aa[i], bqa[i]));
        ob.set(i, input_grad(cb, i, gm[i], br[u].get(i), aa[i], bqb[i]));
      }
      oa.store(dxa + (boff + r) * lddxa + c * VEC);
      ob.store(dxb + (boff + r) * lddxb + c * VEC);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// The three launch geometries of the family, side by side.  Host only, and called from norm_plan alone (below): a launcher reads the plan.
// ---------------------------------------------------------------------------------------------------
struct NormGeom {
  int vec;      // elements per lane access (Vec16<T>::N or 1)
  int cv;       // channel vectors per row
  int tx, ty;   // thread grid inside a block
  int rpb;      // rows per block
  int chunks;   // row chunks per sample
  int ctiles;   // channel tiles
};

// the streaming kernels
static NormGeom norm_geom(int S, int C, bool vec_ok, int vecN, int target_blocks = 1024) {
  NormGeom g;
  g.vec = (vec_ok && C % vecN == 0) ? vecN : 1;
  g.cv = C / g.vec;
  g.tx = g.cv < NORM_TX_MAX ? g.cv : NORM_TX_MAX;
  g.ty = NORM_THREADS / g.tx;
  g.ctiles = cdiv(g.cv, g.tx);
  // enough workgroups to fill 256 CUs even on the small grids of the deep stages, >= 4 rows per lane
  // ~4 workgroups per CU for the streaming kernels (one per CU ran the 48^3 tensors at half the HBM rate); the statistics kernel
  // asks for 256 (fewer fp64 atomics)
  int rpb = cdiv(S, target_blocks);
  if (rpb < 4 * g.ty) rpb = 4 * g.ty;
  if (rpb > 1024) rpb = 1024;
  g.rpb = rpb;
  g.chunks = cdiv(S, rpb);
  return g;
}

// slabs_to_out_stats_kernel: the tensors of a split convolution are tiny (27 .. 1728 rows): 8 vector columns x 32 rows per workgroup pass, so
// that even the 3^3 volume is a dozen workgroups (norm_geom's >= 4 rows per lane made it three, 15 us for 16 slabs of 83 KB)
static NormGeom slab_sum_geom(int S, int C, bool vec_ok, int vecN) {
  NormGeom g;
  g.vec = (vec_ok && C % vecN == 0) ? vecN : 1;
  g.cv = C / g.vec;
  g.tx = g.cv < 8 ? g.cv : 8;
  g.ty = NORM_THREADS / g.tx;
  g.ctiles = cdiv(g.cv, g.tx);
  int per = cdiv(S, g.ty * 64);
  g.rpb = g.ty * (per < 1 ? 1 : per > 8 ? 8 : per);
  g.chunks = cdiv(S, g.rpb);
  return g;
}

// thread geometry of the register-resident kernels: ty_n = the power of two >= S, between 16 and 256 - as FEW rows per lane as the tensor
// allows, i.e. as many workgroups as it has channel vectors: these launches are bound by the instructions one wave issues (in-kernel stamps:
// 8 rows x 8 channels per lane cost 3.2 us of arithmetic alone), not by bytes - and tx_n = 256 / ty_n <= 16 channel vectors
struct FusedGeom { int vec, cv, tx, ty; };
static FusedGeom fused_geom(int S, int C, bool vec_ok, int vecN) {
  FusedGeom g;
  int ty = 16;
  while (ty < S && ty < NORM_THREADS) ty <<= 1;
  g.ty = ty;
  g.tx = NORM_THREADS / ty;
  const int rows_per_lane = cdiv(S, ty);
  // channels per lane: 16 bytes where a lane has few rows; narrower (8- / 4-byte loads) where it has many, so that a lane handles <= 16
  // elements and the tensor spreads over 2 - 4 x the workgroups - at 1728 rows x 192 channels the 16-byte form was 24 workgroups of 56
  // elements per lane: 17 us of issue-bound arithmetic (one wave per SIMD) for 0.66 MB
  int vec = 1;
  if (vec_ok) {
    vec = vecN;
    while (vec > 1 && C % vec != 0) vec >>= 1;
    while (vec > 2 && rows_per_lane * vec > 16) vec >>= 1;
  }
  g.vec = vec;
  g.cv = C / g.vec;
  return g;
}

// calls f(std::integral_constant<int, vec>) for the lane width the geometry chose, so that every kernel's launch is written once.  HALVINGS:
// the widths of the register-resident kernels (bf16: 8 / 4 / 2 / 1 channels, fp32: 4 / 2 / 1); otherwise V or 1 (the streaming kernels).
template <int V, bool HALVINGS, class F> static void for_lane_width(int vec, F&& f) {
  if constexpr (V == 1) f(std::integral_constant<int, 1>{});
  else if (vec == V) f(std::integral_constant<int, V>{});
  else for_lane_width<HALVINGS ? V / 2 : 1, HALVINGS>(vec, f);
}
// the same for a kernel's bool template parameter
template <class F> static void for_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

// LDS bytes of the three kinds of launch; nstat: how many (sum, sum of squares) sets the prologue gathers
static size_t reduce_smem(const NormGeom& g, int nstat) {      // block_reduce_to_stat's floats, which reuse the prologue's doubles: the larger of the two
  const size_t red = (size_t)g.ty * 2 * g.tx * g.vec * sizeof(float), pro = (size_t)nstat * 2 * g.tx * g.vec * sizeof(double);
  return red > pro ? red : pro;
}
static size_t apply_smem(const NormGeom& g, int nstat, bool rank1 = false) {      // rank1: no smaller than the floats of the weight gradient's reduction
  const size_t pro = (size_t)nstat * 2 * g.tx * g.vec * sizeof(double), r1 = (size_t)NORM_THREADS * g.vec * sizeof(float);
  return (rank1 && pro < r1) ? r1 : pro;
}
static size_t fused_smem(const FusedGeom& g, int nsum, int nstat) {      // red + tot + gathered statistics
  return (size_t)(NORM_THREADS / 16) * nsum * g.vec * g.tx * sizeof(float) + (size_t)nsum * g.vec * g.tx * sizeof(double) +
         (size_t)nstat * 2 * g.vec * g.tx * sizeof(double);
}

template <class P> static void fill_style_rows(P* (&dst)[MISEG_MAX_STYLES], P* const (&src)[MISEG_MAX_STYLES], int num_styles) {
  for (int s = 0; s < MISEG_MAX_STYLES; ++s) dst[s] = s < num_styles ? src[s] : nullptr;
}
static StylePtrs style_ptrs(const float* const (&gamma)[MISEG_MAX_STYLES], const float* const (&beta)[MISEG_MAX_STYLES], int num_styles) {
  StylePtrs sp;
  fill_style_rows(sp.gamma, gamma, num_styles);
  fill_style_rows(sp.beta, beta, num_styles);
  return sp;
}
static StyleGradPtrs style_grad_ptrs(float* const (&dgamma)[MISEG_MAX_STYLES], float* const (&dbeta)[MISEG_MAX_STYLES], int num_styles) {
  StyleGradPtrs gp;
  fill_style_rows(gp.dgamma, dgamma, num_styles);
  fill_style_rows(gp.dbeta, dbeta, num_styles);
  return gp;
}

// ---------------------------------------------------------------------------------------------------
// LayerNorm over C per row: one wave per row (C <= 8192)
// ---------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) layernorm_fwd_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy, int64_t rows, int C,
                                                            float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ mean, float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* xr = x + row * ldx;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += to_f32(xr[c]);
  s = wave_sum(s);
  const float m = s / C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) { const float d = to_f32(xr[c]) - m; q = fmaf(d, d, q); }
  q = wave_sum(q);
  const float rs = 1.0f / sqrtf(q / C + eps);      // correctly rounded (v_rsq_f32 is 1 ulp: the fp32 parity mode wants torch's value)
  if (lane == 0) { mean[row] = m; rstd[row] = rs; }
  T* yr = y + row * ldy;
  for (int c = lane; c < C; c += 64) {
    float v = (to_f32(xr[c]) - m) * rs;
    if (gamma) v = v * gamma[c];
    if (beta) v += beta[c];
    yr[c] = from_f32<T>(v);
  }
}

template <class T>
__global__ void __launch_bounds__(256) layernorm_bwd_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ x, int64_t ldx, T* __restrict__ dx,
                                                            int64_t lddx, int64_t rows, int C, const float* __restrict__ gamma,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* xr = x + row * ldx;
  const T* gr = dy + row * lddy;
  const float m = mean[row], rs = rstd[row];
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float g = to_f32(gr[c]) * (gamma ? gamma[c] : 1.f);
    const float xh = (to_f32(xr[c]) - m) * rs;
    s1 += g;
    s2 = fmaf(g, xh, s2);
  }
  s1 = wave_sum(s1) / C;
  s2 = wave_sum(s2) / C;
  T* dr = dx + row * lddx;
  for (int c = lane; c < C; c += 64) {
    const float g = to_f32(gr[c]) * (gamma ? gamma[c] : 1.f);
    const float xh = (to_f32(xr[c]) - m) * rs;
    dr[c] = from_f32<T>(rs * (g - s1 - xh * s2));
  }
}

// dgamma[c] += sum_r dy*xhat ; dbeta[c] += sum_r dy   (block handles a row slab, atomics at the end)
template <class T>
__global__ void __launch_bounds__(256) layernorm_bwd_param_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ x, int64_t ldx,
                                                                  int64_t rows, int C, const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, int rows_per_block) {
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(rows, r0 + rows_per_block);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float sg = 0.f, sb = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
      const float g = to_f32(dy[r * lddy + c]);
      sg = fmaf(g, (to_f32(x[r * ldx + c]) - mean[r]) * rstd[r], sg);
      sb += g;
    }
    if (dgamma) atomicAdd(dgamma + c, sg);
    if (dbeta) atomicAdd(dbeta + c, sb);
  }
}

}  // namespace miseg

using namespace miseg;

// ---------------------------------------------------------------------------------------------------
// The plan of an instance-norm call: validation, the 16-byte-lane predicate, the choice between the streaming and the
// register-resident generation, geometry and LDS bytes of every launch - decided here, once, on the host.  The launchers below read it.
// ---------------------------------------------------------------------------------------------------
enum NormEntry { ENTRY_STATS, ENTRY_APPLY, ENTRY_FWD, ENTRY_FWD_SLABS, ENTRY_BWD, ENTRY_BWD_APPLY, ENTRY_BWD_SLABS, ENTRY_BWD_REDUCE, ENTRY_PAIR_BWD,
                 ENTRY_SLAB_SUM };      // the last: slabs_to_out_stats (conv3d.hip), which has no public plan
static constexpr int IN_SLAB_SUM = -1;      // miseg_instnorm_launch.kernel of that internal launch

struct SlabSumParams { const void* y; int64_t ldy; const void* res; int64_t ldres; int B, S, C, dtype; };

struct Operand { const void* p; int64_t ld; bool present; };

// what the planner keeps of a validated call, whichever params struct it came in
struct NormCall {
  int B, S, C, V;         // V: elements of a 16-byte lane
  Operand ops[7];         // the operands of the alignment predicate; an absent optional operand constrains nothing
  int nops;
  bool extra;             // the named terms of the entry's predicate that are no operand alignment (below)
  bool rank1;
};

// THE alignment predicate: every present operand starts on a 16-byte boundary and its row stride is a whole number of 16-byte lanes
static bool lanes16(const Operand* ops, int n, int V) {
  for (int i = 0; i < n; ++i)
    if (ops[i].present && (((uintptr_t)ops[i].p % 16) != 0 || ops[i].ld % V != 0)) return false;
  return true;
}
// its named extra terms.  SLABS_AS_OPERAND: fp32 slabs stand in for dy / x - 16-byte aligned, slab_stride % 4 == 0, and their row stride is C
static bool slabs_as_operand(const float* slabs, int64_t slab_stride, int C, int V) {
  return !slabs || (((uintptr_t)slabs % 16) == 0 && slab_stride % 4 == 0 && C % V == 0);
}
// SLAB_SUM_LANES: slabs_to_out_stats reads the slabs in 16-byte fp32 lanes whatever the output's dtype (slab stride B S C: a multiple of 4 with C)
static bool slab_sum_lanes(const float* slabs, int C) { return ((uintptr_t)slabs % 16) == 0 && C % 4 == 0; }
// RANK1_WHOLE_LANES: the rank-1 pair reads r1w in the lanes of the tensors
static bool rank1_whole_lanes(bool rank1, int C, int V) { return !rank1 || C % V == 0; }

// THE generation choice: the register-resident one-launch kernels up to NORM_FUSED_MAX_ROWS rows per sample - for the entries that have one:
// the single halves never (bwd_apply: the producer's sums stand in for the reduction at any size), the rank-1 pair never.  Slabs exist in
// the register-resident kernels alone: a slab call this function sends to the streaming kernels is refused.
static bool takes_fused(NormEntry e, int S, bool rank1) {
  const bool has_fused = e == ENTRY_FWD || e == ENTRY_FWD_SLABS || e == ENTRY_BWD || e == ENTRY_BWD_SLABS || (e == ENTRY_PAIR_BWD && !rank1);
  return has_fused && S <= NORM_FUSED_MAX_ROWS;
}

static int lane_elems(int dtype, int* V) {
  return dispatch_dtype(dtype, [&](auto* tag) -> int {
    *V = Vec16<typename std::remove_pointer<decltype(tag)>::type>::N;
    return MISEG_OK;
  });
}

// Every refusal of the nine entry points, in the parent launchers' order and with their codes and texts.  Kept disagreements:
//   BWD_ACT_IS_BADARG            miseg_instnorm_bwd refuses a bad act with BADARG, miseg_instnorm_fwd / _apply with UNSUPPORTED
//   STREAMING_FWD_SPEAKS_AS_ITS_HALVES   miseg_instnorm_fwd above NORM_FUSED_MAX_ROWS rows refuses with the checks and texts of miseg_instnorm_stats, then
//                                of miseg_instnorm_apply (so: a shape check the fused path has not, and r1x without res_stat refused)
static int apply_refusals(const miseg_instnorm_apply_params* p) {
  MISEG_REQUIRE(p->num_styles >= 1 && p->num_styles <= MISEG_MAX_STYLES, MISEG_E_BADARG, "instnorm_apply: num_styles %d", p->num_styles);
  MISEG_REQUIRE(p->act == MISEG_ACT_NONE || p->act == MISEG_ACT_LEAKY, MISEG_E_UNSUPPORTED, "instnorm_apply: act %d", p->act);
  MISEG_REQUIRE(!p->res_stat || p->res || p->r1x, MISEG_E_BADARG, "instnorm_apply: res_stat without res");
  MISEG_REQUIRE(!p->r1x || (p->res_stat && !p->res && p->r1w), MISEG_E_BADARG, "instnorm_apply: r1x needs res_stat and r1w, and excludes res");
  return MISEG_OK;
}
static int stats_shape_refusal(int B, int S, int C, int64_t ldx) {
  MISEG_REQUIRE(B > 0 && S > 0 && C > 0 && ldx >= C, MISEG_E_BADARG, "instnorm_stats: bad shape B=%d S=%d C=%d ld=%ld", B, S, C, (long)ldx);
  return MISEG_OK;
}
static int slab_refusals(const char* who, NormEntry e, int B, int S, int C, int nslabs, int64_t slab_stride) {
  MISEG_REQUIRE(takes_fused(e, S, false), MISEG_E_UNSUPPORTED, "%s: %d rows per sample (at most %d: miseg_instnorm_fused_max_rows)", who, S, NORM_FUSED_MAX_ROWS);
  MISEG_REQUIRE(nslabs >= 1 && slab_stride >= (int64_t)B * S * C, MISEG_E_BADARG, "%s: nslabs / slab_stride", who);
  return MISEG_OK;
}

static int norm_validate(NormEntry e, const void* params, const float* slabs, int nslabs, int64_t slab_stride, NormCall* c) {
  int rc = MISEG_OK, dtype = -1;
  c->nops = 0;
  c->extra = true;
  c->rank1 = false;
  auto operand = [&](const void* p, int64_t ld, bool present = true) { c->ops[c->nops++] = Operand{p, ld, present}; };
  auto shape = [&](int B, int S, int C, int dt) { c->B = B; c->S = S; c->C = C; dtype = dt; };
  switch (e) {
    case ENTRY_STATS: {
      const auto* p = (const miseg_instnorm_stats_params*)params;
      MISEG_REQUIRE(p && p->x && p->stat, MISEG_E_BADARG, "instnorm_stats: null pointer");
      if ((rc = stats_shape_refusal(p->B, p->S, p->C, p->ldx))) return rc;
      shape(p->B, p->S, p->C, p->dtype);
      operand(p->x, p->ldx);
      break;
    }
    case ENTRY_APPLY: case ENTRY_FWD: case ENTRY_FWD_SLABS: {
      const auto* p = (const miseg_instnorm_apply_params*)params;
      if (e == ENTRY_APPLY) {
        MISEG_REQUIRE(p && p->x && p->y && p->stat, MISEG_E_BADARG, "instnorm_apply: null pointer");
        if ((rc = apply_refusals(p))) return rc;
      } else {
        MISEG_REQUIRE(e == ENTRY_FWD || slabs, MISEG_E_BADARG, "instnorm_fwd_slabs: null slabs");
        MISEG_REQUIRE(p && p->x && p->y && p->stat, MISEG_E_BADARG, "instnorm_fwd: null pointer");
        MISEG_REQUIRE(!p->res_stat, MISEG_E_UNSUPPORTED, "instnorm_fwd: res_stat (shortcut norm on the fly) is a miseg_instnorm_apply feature");
        if (slabs && (rc = slab_refusals("instnorm_fwd_slabs", e, p->B, p->S, p->C, nslabs, slab_stride))) return rc;
        if (!takes_fused(e, p->S, false)) {      // STREAMING_FWD_SPEAKS_AS_ITS_HALVES
          if ((rc = stats_shape_refusal(p->B, p->S, p->C, p->ldx)) || (rc = lane_elems(p->dtype, &c->V)) || (rc = apply_refusals(p))) return rc;
        } else {
          MISEG_REQUIRE(p->num_styles >= 1 && p->num_styles <= MISEG_MAX_STYLES, MISEG_E_BADARG, "instnorm_fwd: num_styles %d", p->num_styles);
          MISEG_REQUIRE(p->act == MISEG_ACT_NONE || p->act == MISEG_ACT_LEAKY, MISEG_E_UNSUPPORTED, "instnorm_fwd: act %d", p->act);
        }
      }
      shape(p->B, p->S, p->C, p->dtype);
      operand(p->x, p->ldx);      // first: the statistics launch of the streaming forward reads this operand alone
      operand(p->y, p->ldy);
      operand(p->res, p->ldres, p->res != nullptr);
      c->rank1 = e == ENTRY_APPLY && p->r1x;
      break;
    }
    case ENTRY_BWD: case ENTRY_BWD_APPLY: case ENTRY_BWD_SLABS: {
      const auto* p = (const miseg_instnorm_bwd_params*)params;
      if (e == ENTRY_BWD_APPLY)
        MISEG_REQUIRE(p && p->act == MISEG_ACT_NONE, MISEG_E_UNSUPPORTED, "instnorm_bwd_apply: no activation (the producer's sums know nothing of one)");
      MISEG_REQUIRE(e != ENTRY_BWD_SLABS || slabs, MISEG_E_BADARG, "instnorm_bwd_slabs: null slabs");
      MISEG_REQUIRE(p && (p->dy || slabs) && p->x && p->dx && p->stat && p->dstat, MISEG_E_BADARG, "instnorm_bwd: null pointer");
      if (slabs && (rc = slab_refusals("instnorm_bwd_slabs", e, p->B, p->S, p->C, nslabs, slab_stride))) return rc;
      MISEG_REQUIRE(p->act == MISEG_ACT_NONE || p->act == MISEG_ACT_LEAKY, MISEG_E_BADARG, "instnorm_bwd: act %d", p->act);      // BWD_ACT_IS_BADARG
      MISEG_REQUIRE(p->num_styles >= 1 && p->num_styles <= MISEG_MAX_STYLES, MISEG_E_BADARG, "instnorm_bwd: num_styles %d", p->num_styles);
      shape(p->B, p->S, p->C, p->dtype);
      operand(p->dy, p->lddy, !slabs);
      operand(p->x, p->ldx);
      operand(p->dx, p->lddx);
      operand(p->y, p->ldy, p->act != MISEG_ACT_NONE);      // y may be NULL with an activation (the sign is recomputed): NULL is aligned
      operand(p->dres, p->lddres, p->dres != nullptr);
      operand(p->gadd, p->ldgadd, p->gadd != nullptr);
      break;
    }
    case ENTRY_BWD_REDUCE: {
      const auto* p = (const miseg_instnorm_bwd_params*)params;
      MISEG_REQUIRE(p && p->dy && p->x && p->stat && p->dstat, MISEG_E_BADARG, "instnorm_bwd_reduce: null pointer");
      MISEG_REQUIRE(p->act == MISEG_ACT_NONE, MISEG_E_UNSUPPORTED, "instnorm_bwd_reduce: no activation (compose it outside)");
      shape(p->B, p->S, p->C, p->dtype);
      operand(p->dy, p->lddy);
      operand(p->x, p->ldx);
      break;
    }
    case ENTRY_PAIR_BWD: {
      const auto* p = (const miseg_instnorm_pair_bwd_params*)params;
      MISEG_REQUIRE(p && p->dy && p->xa && p->dxa && p->stat_a && p->stat_b && p->dstat_a && p->dstat_b, MISEG_E_BADARG, "instnorm_pair_bwd: null pointer");
      MISEG_REQUIRE(p->r1x ? (p->r1w && p->r1dw && !p->xb && !p->dxb && !p->y) : (p->xb && p->dxb), MISEG_E_BADARG,
                    "instnorm_pair_bwd: either xb / dxb, or the rank-1 shortcut (r1x, r1w, r1dw; no y)");
      MISEG_REQUIRE(p->num_styles >= 1 && p->num_styles <= MISEG_MAX_STYLES, MISEG_E_BADARG, "instnorm_pair_bwd: num_styles %d", p->num_styles);
      shape(p->B, p->S, p->C, p->dtype);
      operand(p->dy, p->lddy);
      operand(p->y, p->ldy, p->y != nullptr);
      operand(p->xa, p->ldxa);
      operand(p->xb, p->ldxb, p->xb != nullptr);
      operand(p->dxb, p->lddxb, p->xb != nullptr);
      operand(p->dxa, p->lddxa);
      c->rank1 = p->r1x != nullptr;
      break;
    }
    case ENTRY_SLAB_SUM: {
      const auto* p = (const SlabSumParams*)params;
      shape(p->B, p->S, p->C, p->dtype);
      operand(p->y, p->ldy);
      operand(p->res, p->ldres, p->res != nullptr);
      break;
    }
  }
  if ((rc = lane_elems(dtype, &c->V))) return rc;
  // the one refusal the parent launchers did not have: they divided by C (or launched an empty grid) where an entry point checks no shape
  MISEG_REQUIRE(c->B > 0 && c->S > 0 && c->C > 0, MISEG_E_BADARG, "instnorm: bad shape B=%d S=%d C=%d", c->B, c->S, c->C);
  // the named extra terms.  The rank-1 PAIR asks C % V == 0 in its predicate; the apply entry with the same shortcut does not (kept: c->rank1
  // of an apply call only marks its launch)
  const bool pair_rank1 = e == ENTRY_PAIR_BWD && c->rank1;
  if (e == ENTRY_SLAB_SUM) c->extra = slab_sum_lanes(slabs, c->C);
  else c->extra = slabs_as_operand(slabs, slab_stride, c->C, c->V) && rank1_whole_lanes(pair_rank1, c->C, c->V);
  return MISEG_OK;
}

static void plan_streaming(miseg_instnorm_plan_info* plan, int kernel, const NormGeom& g, const NormCall& c, size_t lds) {
  miseg_instnorm_launch& l = plan->launch[plan->n_launches++];
  l = miseg_instnorm_launch{kernel, g.vec, 0, g.cv, g.tx, g.ty, g.rpb, g.chunks, g.ctiles, g.chunks, c.B, g.ctiles, NORM_THREADS, c.rank1, (int32_t)lds};
}
static void plan_fused(miseg_instnorm_plan_info* plan, int kernel, const FusedGeom& g, const NormCall& c, bool from_slabs, size_t lds) {
  miseg_instnorm_launch& l = plan->launch[plan->n_launches++];
  l = miseg_instnorm_launch{kernel, g.vec, from_slabs, g.cv, g.tx, g.ty, 0, 0, 0, cdiv(g.cv, g.tx), c.B, 1, NORM_THREADS, 0, (int32_t)lds};
}

static int norm_plan(NormEntry e, const void* params, const float* slabs, int nslabs, int64_t slab_stride, miseg_instnorm_plan_info* plan) {
  MISEG_REQUIRE(plan, MISEG_E_BADARG, "instnorm plan: null plan");
  *plan = miseg_instnorm_plan_info{};
  NormCall c;
  if (int rc = norm_validate(e, params, slabs, nslabs, slab_stride, &c)) return rc;
  const bool al = lanes16(c.ops, c.nops, c.V) && c.extra;
  plan->aligned = al;
  if (takes_fused(e, c.S, c.rank1)) {
    const FusedGeom f = fused_geom(c.S, c.C, al, c.V);
    if (e == ENTRY_PAIR_BWD) plan_fused(plan, MISEG_IN_PAIR_FUSED_BWD, f, c, false, fused_smem(f, 3, 2));
    else if (e == ENTRY_BWD || e == ENTRY_BWD_SLABS) plan_fused(plan, MISEG_IN_FUSED_BWD, f, c, slabs != nullptr, fused_smem(f, 2, 1));
    else plan_fused(plan, MISEG_IN_FUSED_FWD, f, c, slabs != nullptr, fused_smem(f, 2, 0));
    return MISEG_OK;
  }
  if (e == ENTRY_SLAB_SUM) {
    const NormGeom g = slab_sum_geom(c.S, c.C, al, c.V);
    plan_streaming(plan, IN_SLAB_SUM, g, c, reduce_smem(g, 0));
    return MISEG_OK;
  }
  if (e == ENTRY_STATS || e == ENTRY_FWD) {
    // the statistics launch: a target of 256 workgroups (fewer fp64 atomics), and - in the streaming forward too - a predicate over x alone
    // (ops[0]), so it keeps its 16-byte lanes where y or res send the apply launch of the same call to the scalar ones
    const NormGeom g = norm_geom(c.S, c.C, lanes16(c.ops, 1, c.V), c.V, 256);
    plan_streaming(plan, MISEG_IN_STATS, g, c, reduce_smem(g, 0));
    if (e == ENTRY_STATS) return MISEG_OK;
  }
  const NormGeom g = norm_geom(c.S, c.C, al, c.V);
  switch (e) {
    case ENTRY_APPLY: case ENTRY_FWD: plan_streaming(plan, MISEG_IN_APPLY, g, c, apply_smem(g, 2)); break;
    case ENTRY_BWD: case ENTRY_BWD_APPLY:
      if (e == ENTRY_BWD) plan_streaming(plan, MISEG_IN_BWD_REDUCE, g, c, reduce_smem(g, 1));
      plan_streaming(plan, MISEG_IN_BWD_APPLY, g, c, apply_smem(g, 2));
      break;
    case ENTRY_BWD_REDUCE: plan_streaming(plan, MISEG_IN_BWD_REDUCE, g, c, reduce_smem(g, 1)); break;
    case ENTRY_PAIR_BWD:
      plan_streaming(plan, MISEG_IN_PAIR_BWD_REDUCE, g, c, reduce_smem(g, 2));
      plan_streaming(plan, MISEG_IN_PAIR_BWD_APPLY, g, c, apply_smem(g, 4, c.rank1));
      break;
    default: break;
  }
  return MISEG_OK;
}

extern "C" int miseg_instnorm_stats_plan(const miseg_instnorm_stats_params* p, miseg_instnorm_plan_info* plan) { return norm_plan(ENTRY_STATS, p, nullptr, 0, 0, plan); }
extern "C" int miseg_instnorm_apply_plan(const miseg_instnorm_apply_params* p, miseg_instnorm_plan_info* plan) { return norm_plan(ENTRY_APPLY, p, nullptr, 0, 0, plan); }
extern "C" int miseg_instnorm_fwd_plan(const miseg_instnorm_apply_params* p, miseg_instnorm_plan_info* plan) { return norm_plan(ENTRY_FWD, p, nullptr, 0, 0, plan); }
extern "C" int miseg_instnorm_fwd_slabs_plan(const miseg_instnorm_apply_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_instnorm_plan_info* plan) {
  return norm_plan(ENTRY_FWD_SLABS, p, slabs, nslabs, slab_stride, plan);
}
extern "C" int miseg_instnorm_bwd_plan(const miseg_instnorm_bwd_params* p, miseg_instnorm_plan_info* plan) { return norm_plan(ENTRY_BWD, p, nullptr, 0, 0, plan); }
extern "C" int miseg_instnorm_bwd_apply_plan(const miseg_instnorm_bwd_params* p, miseg_instnorm_plan_info* plan) { return norm_plan(ENTRY_BWD_APPLY, p, nullptr, 0, 0, plan); }
extern "C" int miseg_instnorm_bwd_slabs_plan(const miseg_instnorm_bwd_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_instnorm_plan_info* plan) {
  return norm_plan(ENTRY_BWD_SLABS, p, slabs, nslabs, slab_stride, plan);
}
extern "C" int miseg_instnorm_bwd_reduce_plan(const miseg_instnorm_bwd_params* p, miseg_instnorm_plan_info* plan) { return norm_plan(ENTRY_BWD_REDUCE, p, nullptr, 0, 0, plan); }
extern "C" int miseg_instnorm_pair_bwd_plan(const miseg_instnorm_pair_bwd_params* p, miseg_instnorm_plan_info* plan) { return norm_plan(ENTRY_PAIR_BWD, p, nullptr, 0, 0, plan); }

// ---------------------------------------------------------------------------------------------------
// The launchers: each reads its plan and issues the launches it names, with the plan's lane width, geometry, grid and LDS bytes
// ---------------------------------------------------------------------------------------------------
static dim3 grid_of(const miseg_instnorm_launch& l) { return dim3(l.grid_x, l.grid_y, l.grid_z); }

template <class T> static void launch_stats(const miseg_instnorm_launch& l, const void* x, int64_t ldx, int S, int C, const void* stat, hipStream_t stream) {
  for_lane_width<Vec16<T>::N, false>(l.vec, [&](auto w) {
    instnorm_stats_kernel<T, decltype(w)::value><<<grid_of(l), l.threads, l.lds_bytes, stream>>>((const T*)x, ldx, S, C, l.cv, l.tx, l.ty, l.rpb, (double*)stat);
  });
}
template <class T> static void launch_apply(const miseg_instnorm_launch& l, const miseg_instnorm_apply_params* p, hipStream_t stream) {
  const StylePtrs sp = style_ptrs(p->gamma, p->beta, p->num_styles);
  const StylePtrs rsp = style_ptrs(p->res_gamma, p->res_beta, p->res_stat ? p->num_styles : 0);
  for_lane_width<Vec16<T>::N, false>(l.vec, [&](auto w) {
    instnorm_apply_kernel<T, decltype(w)::value><<<grid_of(l), l.threads, l.lds_bytes, stream>>>(
        (const T*)p->x, p->ldx, (const T*)p->res, p->ldres, (T*)p->y, p->ldy, p->S, p->C, l.cv, l.tx, l.ty, l.rpb, (const double*)p->stat, p->eps, p->styles, sp,
        p->act, p->slope, (const double*)p->res_stat, rsp, (const T*)p->r1x, p->ldr1x, (const T*)p->r1w);
  });
}

namespace miseg {
// internal (conv3d.hip): y = round(sum of the slabs) (+ res) and its statistics; stat may be null (plain sum + convert)
int slabs_to_out_stats(const float* slabs, int nslabs, void* y, int64_t ldy, const void* res, int64_t ldres, int B, int S, int C, int dtype, double* stat,
                       hipStream_t stream) {
  const SlabSumParams sp{y, ldy, res, ldres, B, S, C, dtype};
  miseg_instnorm_plan_info plan;
  if (int rc = norm_plan(ENTRY_SLAB_SUM, &sp, slabs, nslabs, 0, &plan)) return rc;
  return dispatch_dtype(dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    const miseg_instnorm_launch& l = plan.launch[0];
    const int64_t stride = (int64_t)B * S * C;
    for_lane_width<Vec16<T>::N, false>(l.vec, [&](auto w) {
      slabs_to_out_stats_kernel<T, decltype(w)::value><<<grid_of(l), l.threads, l.lds_bytes, stream>>>(slabs, nslabs, stride, (T*)y, ldy, (const T*)res, ldres, S, C, l.cv,
                                                                                                      l.tx, l.ty, l.rpb, stat);
    });
    MISEG_LAUNCH_CHECK("slabs_to_out_stats");
    return MISEG_OK;
  });
}
}  // namespace miseg

#ifdef MISEG_NORM_STAMPS
extern "C" int miseg_debug_norm_stamps(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(miseg::g_norm_stamps), sizeof(miseg::g_norm_stamps)); }
#endif

extern "C" size_t miseg_instnorm_stat_bytes(int B, int C) { return (size_t)NORM_R * B * C * 2 * sizeof(double); }
extern "C" int miseg_instnorm_fused_max_rows(void) { return NORM_FUSED_MAX_ROWS; }

extern "C" int miseg_instnorm_stats(const miseg_instnorm_stats_params* p, miseg_stream_t stream) {
  miseg_instnorm_plan_info plan;
  if (int rc = norm_plan(ENTRY_STATS, p, nullptr, 0, 0, &plan)) return rc;
  return dispatch_dtype(p->dtype, [&](auto* tag) -> int {
    launch_stats<typename std::remove_pointer<decltype(tag)>::type>(plan.launch[0], p->x, p->ldx, p->S, p->C, p->stat, (hipStream_t)stream);
    MISEG_LAUNCH_CHECK("instnorm_stats");
    return MISEG_OK;
  });
}

extern "C" int miseg_instnorm_apply(const miseg_instnorm_apply_params* p, miseg_stream_t stream) {
  miseg_instnorm_plan_info plan;
  if (int rc = norm_plan(ENTRY_APPLY, p, nullptr, 0, 0, &plan)) return rc;
  return dispatch_dtype(p->dtype, [&](auto* tag) -> int {
    launch_apply<typename std::remove_pointer<decltype(tag)>::type>(plan.launch[0], p, (hipStream_t)stream);
    MISEG_LAUNCH_CHECK("instnorm_apply");
    return MISEG_OK;
  });
}

// statistics + normalisation: the two streaming kernels, or one fused launch for the small tensors of the deep stages
static int instnorm_fwd_impl(NormEntry e, const miseg_instnorm_apply_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  miseg_instnorm_plan_info plan;
  if (int rc = norm_plan(e, p, slabs, nslabs, slab_stride, &plan)) return rc;
  return dispatch_dtype(p->dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    const miseg_instnorm_launch& l = plan.launch[0];
    if (l.kernel == MISEG_IN_STATS) {
      launch_stats<T>(l, p->x, p->ldx, p->S, p->C, p->stat, stream);
      MISEG_LAUNCH_CHECK("instnorm_stats");
      launch_apply<T>(plan.launch[1], p, stream);
      MISEG_LAUNCH_CHECK("instnorm_apply");
      return MISEG_OK;
    }
    const StylePtrs sp = style_ptrs(p->gamma, p->beta, p->num_styles);
    for_lane_width<Vec16<T>::N, true>(l.vec, [&](auto w) {
      for_flag(l.from_slabs, [&](auto from_slabs) {
        instnorm_fused_fwd_kernel<T, decltype(w)::value, decltype(from_slabs)::value><<<grid_of(l), l.threads, l.lds_bytes, stream>>>(
            (T*)p->x, p->ldx, (const T*)p->res, p->ldres, (T*)p->y, p->ldy, p->S, p->C, l.cv, l.tx, l.ty, (double*)p->stat, p->eps, p->styles, sp, p->act, p->slope,
            slabs, nslabs, slab_stride);
      });
    });
    MISEG_LAUNCH_CHECK("instnorm_fwd");
    return MISEG_OK;
  });
}

extern "C" int miseg_instnorm_fwd(const miseg_instnorm_apply_params* p, miseg_stream_t stream) { return instnorm_fwd_impl(ENTRY_FWD, p, nullptr, 0, 0, stream); }
extern "C" int miseg_instnorm_fwd_slabs(const miseg_instnorm_apply_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_stream_t stream) {
  return instnorm_fwd_impl(ENTRY_FWD_SLABS, p, slabs, nslabs, slab_stride, stream);
}

// ENTRY_BWD_APPLY: p->dstat already holds the backward sums (the epilogue of the GEMM that produced dy added them: miseg_gemm_params.stat_mode 2,
// miseg_mlp_params.bs_dstat) - the plan names no reduction launch and tensors of any size take the streaming apply kernel
static int instnorm_bwd_impl(NormEntry e, const miseg_instnorm_bwd_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  miseg_instnorm_plan_info plan;
  if (int rc = norm_plan(e, p, slabs, nslabs, slab_stride, &plan)) return rc;
  return dispatch_dtype(p->dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    constexpr int V = Vec16<T>::N;
    const StylePtrs sp = style_ptrs(p->gamma, p->beta, p->num_styles);
    const StyleGradPtrs gp = style_grad_ptrs(p->dgamma, p->dbeta, p->num_styles);
    const double* stat = (const double*)p->stat;
    double* dstat = (double*)p->dstat;
    for (int i = 0; i < plan.n_launches; ++i) {
      const miseg_instnorm_launch& l = plan.launch[i];
      if (l.kernel == MISEG_IN_FUSED_BWD)
        for_lane_width<V, true>(l.vec, [&](auto w) {
          for_flag(l.from_slabs, [&](auto from_slabs) {
            instnorm_fused_bwd_kernel<T, decltype(w)::value, decltype(from_slabs)::value><<<grid_of(l), l.threads, l.lds_bytes, stream>>>(
                (const T*)p->dy, p->lddy, (const T*)p->y, p->ldy, (const T*)p->x, p->ldx, (T*)p->dx, p->lddx, (T*)p->dres, p->lddres, p->S, p->C, l.cv, l.tx, l.ty, stat,
                p->eps, p->styles, sp, gp, p->act, p->slope, (const T*)p->gadd, p->ldgadd, slabs, nslabs, slab_stride);
          });
        });
      else
        for_lane_width<V, false>(l.vec, [&](auto w) {
          constexpr int W = decltype(w)::value;
          if (l.kernel == MISEG_IN_BWD_REDUCE)
            instnorm_bwd_reduce_kernel<T, W><<<grid_of(l), l.threads, l.lds_bytes, stream>>>((const T*)p->dy, p->lddy, (const T*)p->y, p->ldy, (const T*)p->x, p->ldx, p->S,
                                                                                           p->C, l.cv, l.tx, l.ty, l.rpb, stat, p->eps, p->act, p->slope, dstat, p->styles, sp);
          else
            instnorm_bwd_apply_kernel<T, W><<<grid_of(l), l.threads, l.lds_bytes, stream>>>((const T*)p->dy, p->lddy, (const T*)p->y, p->ldy, (const T*)p->x, p->ldx,
                                                                                          (T*)p->dx, p->lddx, (T*)p->dres, p->lddres, p->S, p->C, l.cv, l.tx, l.ty, l.rpb, stat,
                                                                                          p->eps, p->styles, sp, p->act, p->slope, dstat, gp, (const T*)p->gadd, p->ldgadd);
        });
    }
    MISEG_LAUNCH_CHECK("instnorm_bwd");
    return MISEG_OK;
  });
}

extern "C" int miseg_instnorm_bwd(const miseg_instnorm_bwd_params* p, miseg_stream_t stream) { return instnorm_bwd_impl(ENTRY_BWD, p, nullptr, 0, 0, stream); }
extern "C" int miseg_instnorm_bwd_apply(const miseg_instnorm_bwd_params* p, miseg_stream_t stream) { return instnorm_bwd_impl(ENTRY_BWD_APPLY, p, nullptr, 0, 0, stream); }
extern "C" int miseg_instnorm_bwd_slabs(const miseg_instnorm_bwd_params* p, const float* slabs, int nslabs, int64_t slab_stride, miseg_stream_t stream) {
  return instnorm_bwd_impl(ENTRY_BWD_SLABS, p, slabs, nslabs, slab_stride, stream);
}

extern "C" int miseg_instnorm_bwd_reduce(const miseg_instnorm_bwd_params* p, miseg_stream_t stream) {
  miseg_instnorm_plan_info plan;
  if (int rc = norm_plan(ENTRY_BWD_REDUCE, p, nullptr, 0, 0, &plan)) return rc;
  return dispatch_dtype(p->dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    const miseg_instnorm_launch& l = plan.launch[0];
    const StylePtrs sp = style_ptrs(p->gamma, p->beta, 0);      // no activation: nothing reads the affine rows
    for_lane_width<Vec16<T>::N, false>(l.vec, [&](auto w) {
      instnorm_bwd_reduce_kernel<T, decltype(w)::value><<<grid_of(l), l.threads, l.lds_bytes, (hipStream_t)stream>>>(
          (const T*)p->dy, p->lddy, nullptr, 0, (const T*)p->x, p->ldx, p->S, p->C, l.cv, l.tx, l.ty, l.rpb, (const double*)p->stat, p->eps, MISEG_ACT_NONE, 0.f,
          (double*)p->dstat, nullptr, sp);
    });
    MISEG_LAUNCH_CHECK("instnorm_bwd_reduce");
    return MISEG_OK;
  });
}

extern "C" int miseg_instnorm_pair_bwd(const miseg_instnorm_pair_bwd_params* p, miseg_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  miseg_instnorm_plan_info plan;
  if (int rc = norm_plan(ENTRY_PAIR_BWD, p, nullptr, 0, 0, &plan)) return rc;
  return dispatch_dtype(p->dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    constexpr int V = Vec16<T>::N;
    const StylePtrs spa = style_ptrs(p->gamma_a, p->beta_a, p->num_styles), spb = style_ptrs(p->gamma_b, p->beta_b, p->num_styles);      // betas: only read when y is absent
    const StyleGradPtrs gpa = style_grad_ptrs(p->dgamma_a, p->dbeta_a, p->num_styles), gpb = style_grad_ptrs(p->dgamma_b, p->dbeta_b, p->num_styles);
    for (int i = 0; i < plan.n_launches; ++i) {
      const miseg_instnorm_launch& l = plan.launch[i];
      if (l.kernel == MISEG_IN_PAIR_FUSED_BWD)      // small tensors: one register-resident launch
        for_lane_width<V, true>(l.vec, [&](auto w) {
          instnorm_pair_fused_bwd_kernel<T, decltype(w)::value><<<grid_of(l), l.threads, l.lds_bytes, stream>>>(
              (const T*)p->dy, p->lddy, (const T*)p->y, p->ldy, (const T*)p->xa, p->ldxa, (const T*)p->xb, p->ldxb, (T*)p->dxa, p->lddxa, (T*)p->dxb, p->lddxb, p->S, p->C,
              l.cv, l.tx, l.ty, (const double*)p->stat_a, (const double*)p->stat_b, p->eps, p->styles, spa, spb, p->slope, gpa, gpb);
        });
      else
        for_lane_width<V, false>(l.vec, [&](auto w) {
          constexpr int W = decltype(w)::value;
          if (l.kernel == MISEG_IN_PAIR_BWD_REDUCE)
            instnorm_pair_bwd_reduce_kernel<T, W><<<grid_of(l), l.threads, l.lds_bytes, stream>>>(
                (const T*)p->dy, p->lddy, (const T*)p->y, p->ldy, (const T*)p->xa, p->ldxa, (const T*)p->xb, p->ldxb, p->S, p->C, l.cv, l.tx, l.ty, l.rpb,
                (const double*)p->stat_a, (const double*)p->stat_b, p->eps, p->slope, (double*)p->dstat_a, (double*)p->dstat_b, p->styles, spa, spb, (const T*)p->r1x,
                p->ldr1x, (const T*)p->r1w);
          else
            instnorm_pair_bwd_apply_kernel<T, W><<<grid_of(l), l.threads, l.lds_bytes, stream>>>(
                (const T*)p->dy, p->lddy, (const T*)p->y, p->ldy, (const T*)p->xa, p->ldxa, (const T*)p->xb, p->ldxb, (T*)p->dxa, p->lddxa, (T*)p->dxb, p->lddxb, p->S, p->C,
                l.cv, l.tx, l.ty, l.rpb, (const double*)p->stat_a, (const double*)p->stat_b, p->eps, p->styles, spa, spb, p->slope, (const double*)p->dstat_a,
                (const double*)p->dstat_b, gpa, gpb, (const T*)p->r1x, p->ldr1x, (const T*)p->r1w, p->r1dw);
        });
    }
    MISEG_LAUNCH_CHECK("instnorm_pair_bwd");
    return MISEG_OK;
  });
}

extern "C" int miseg_layernorm_fwd(const miseg_layernorm_fwd_params* p, miseg_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  MISEG_REQUIRE(p && p->x && p->y && p->mean && p->rstd && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "layernorm_fwd: bad args");
  return dispatch_dtype(p->dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    layernorm_fwd_kernel<T><<<cdiv(p->rows, 4), 256, 0, stream>>>((const T*)p->x, p->ldx, (T*)p->y, p->ldy, p->rows, p->C, p->eps, p->gamma, p->beta, p->mean, p->rstd);
    MISEG_LAUNCH_CHECK("layernorm_fwd");
    return MISEG_OK;
  });
}

extern "C" int miseg_layernorm_bwd(const miseg_layernorm_bwd_params* p, miseg_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  MISEG_REQUIRE(p && p->dy && p->x && p->dx && p->mean && p->rstd && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "layernorm_bwd: bad args");
  return dispatch_dtype(p->dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    layernorm_bwd_kernel<T><<<cdiv(p->rows, 4), 256, 0, stream>>>((const T*)p->dy, p->lddy, (const T*)p->x, p->ldx, (T*)p->dx, p->lddx, p->rows, p->C, p->gamma,
                                                                  p->mean, p->rstd);
    if (p->dgamma || p->dbeta) {
      const int rpb = 256;
      layernorm_bwd_param_kernel<T><<<cdiv(p->rows, rpb), 256, 0, stream>>>((const T*)p->dy, p->lddy, (const T*)p->x, p->ldx, p->rows, p->C, p->mean, p->rstd,
                                                                           p->dgamma, p->dbeta, rpb);
    }
    MISEG_LAUNCH_CHECK("layernorm_bwd");
    return MISEG_OK;
  });
}
