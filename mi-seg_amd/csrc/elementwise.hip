// Plain row operations and data movers (all HBM-bound): add, copy/cast, GELU, row bias, PReLU, affine2, 2x2x2 space<->channel, im2col for tiny
// grids, column sums, resample2, upsample_cat, layout kernels, batched parameter cast, word fills.  The network-end kernels: net_end.hip.
#include "rowwise.h"

namespace miseg {

// ----------------------------------------------------------------------------- the row operations: one loop, one body each
// op(r, c) handles the VEC elements of row r that start at channel c
template <int VEC, class Op>
__global__ void __launch_bounds__(256) rowwise_kernel(int64_t rows, int cv, Op op) {
  const int64_t total = rows * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cv;
    const int c = (int)(i % cv) * VEC;
    op(r, c);
  }
}

// Op<T, VEC>{args...} over rows x C, VEC by `vec` (rowwise.h: vec16_ok), on at most `cap` workgroups
template <template <class, int> class Op, class T, class... A>
static inline void rowwise_launch(bool vec, int64_t rows, int C, int cap, hipStream_t s, A... args) {
  vec_pick<T>(vec, C, [&](auto vc, int cv) {
    constexpr int VEC = decltype(vc)::value;
    rowwise_kernel<VEC><<<ew_grid(rows * cv, cap), 256, 0, s>>>(rows, cv, Op<T, VEC>{args...});
  });
}

template <class T, int VEC> struct AddOp {
  const T* a; int64_t lda; const T* b; int64_t ldb; T* y; int64_t ldy;
  __device__ __forceinline__ void operator()(int64_t r, int c) const {
    V<T, VEC> va, vb;
    va.load(a + r * lda + c);
    vb.load(b + r * ldb + c);
#pragma unroll
    for (int k = 0; k < VEC; ++k) va.v[k] += vb.v[k];
    va.store(y + r * ldy + c);
  }
};

template <class T, int VEC> struct GeluFwdOp {
  const T* x; int64_t ldx; T* y; int64_t ldy;
  __device__ __forceinline__ void operator()(int64_t r, int c) const {
    V<T, VEC> xv;
    xv.load(x + r * ldx + c);
#pragma unroll
    for (int k = 0; k < VEC; ++k) xv.v[k] = 0.5f * xv.v[k] * (1.f + erff(xv.v[k] * 0.70710678118654752f));
    xv.store(y + r * ldy + c);
  }
};

template <class T, int VEC> struct GeluBwdOp {
  const T* dy; int64_t lddy; const T* x; int64_t ldx; T* dx; int64_t lddx;
  __device__ __forceinline__ void operator()(int64_t r, int c) const {
    V<T, VEC> g, xv;
    g.load(dy + r * lddy + c);
    xv.load(x + r * ldx + c);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float t = xv.v[k];
      const float cdf = 0.5f * (1.f + erff(t * 0.70710678118654752f));
      const float pdf = 0.39894228040143268f * (sizeof(T) == 4 ? expf(-0.5f * t * t) : __expf(-0.5f * t * t));
      g.v[k] *= cdf + t * pdf;
    }
    g.store(dx + r * lddx + c);
  }
};

// (the next three: y overlaps no input, which lets the compiler run the loads of several items ahead of the stores in the by-element forms)
template <class T, int VEC> struct RowBiasOp {
  const T* x; int64_t ldx; const float* bias; T* y; int64_t ldy;
  __device__ __forceinline__ void operator()(int64_t r, int c) const {
    __builtin_assume_separate_storage(x, y); __builtin_assume_separate_storage(bias, y);
    V<T, VEC> v;
    v.load(x + r * ldx + c);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v.v[k] += bias[c + k];
    v.store(y + r * ldy + c);
  }
};

template <class T, int VEC> struct PreluFwdOp {
  const T* x; int64_t ldx; const float* slope; T* y; int64_t ldy;
  __device__ __forceinline__ void operator()(int64_t r, int c) const {
    __builtin_assume_separate_storage(x, y); __builtin_assume_separate_storage(slope, y);
    const float a = slope[0];
    V<T, VEC> v;
    v.load(x + r * ldx + c);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v.v[k] = v.v[k] > 0.f ? v.v[k] : a * v.v[k];
    v.store(y + r * ldy + c);
  }
};

// y = k0 * a + k1 * x + k2 with the three coefficients per (batch, channel): coef[b][c][3], rows = B * S
template <class T, int VEC> struct Affine2Op {
  const T* a; int64_t lda; const T* x; int64_t ldx; T* y; int64_t ldy; const float* coef; int S; int C;
  __device__ __forceinline__ void operator()(int64_t r, int c) const {
    __builtin_assume_separate_storage(a, y); __builtin_assume_separate_storage(x, y); __builtin_assume_separate_storage(coef, y);
    const int b = (int)(r / S);
    V<T, VEC> av, xv;
    av.load(a + r * lda + c);
    xv.load(x + r * ldx + c);
    const float* k = coef + ((int64_t)b * C + c) * 3;
#pragma unroll
    for (int e = 0; e < VEC; ++e) av.v[e] = fmaf(k[3 * e], av.v[e], fmaf(k[3 * e + 1], xv.v[e], k[3 * e + 2]));
    av.store(y + r * ldy + c);
  }
};

// ----------------------------------------------------------------------------- copy2d with conversion
template <class TS, class TD>
__global__ void __launch_bounds__(256) copy2d_kernel(const TS* s, int64_t lds, TD* d, int64_t ldd, int64_t rows, int C) {
  const int64_t total = rows * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / C;
    const int c = (int)(i % C);
    d[r * ldd + c] = from_f32<TD>(to_f32(s[r * lds + c]));
  }
}

// ----------------------------------------------------------------------------- cast (+transpose) fp32 matrix
template <class T>
__global__ void __launch_bounds__(256) cast_kernel(const float* s, T* d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = from_f32<T>(s[i]);
}
template <class T>
__global__ void __launch_bounds__(256) cast_transpose_kernel(const float* s, T* d, int R, int C) {
  __shared__ float tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8)
    if (by + j < R && bx + tx < C) tile[j][tx] = s[(int64_t)(by + j) * C + bx + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (bx + j < C && by + tx < R) d[(int64_t)(bx + j) * R + by + tx] = from_f32<T>(tile[tx][j]);
}

// ----------------------------------------------------------------------------- 2x2x2 space <-> channel
struct Off8 { int8_t o[24]; };

// IDX: the item index type.  64-bit division is a ~100-instruction software routine on the GPU and these kernels do 4-5 of them per
// 16-byte item: with fewer than 2^31 items (every shape of the reference configs) the launchers pick the 32-bit instantiation.
template <class T, int VEC, class IDX = int64_t>
__global__ void __launch_bounds__(256) s2c_kernel(const T* src, int64_t lds, T* dst, int64_t ldd, int B, int D, int H, int W, int C, Off8 off) {
  const int D2 = (D + 1) / 2, H2 = (H + 1) / 2, W2 = (W + 1) / 2, cv = C / VEC;
  const IDX total = (IDX)((int64_t)B * D2 * H2 * W2 * 8 * cv);
  for (IDX i = (IDX)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (IDX)gridDim.x * blockDim.x) {
    const int c = (int)(i % cv) * VEC;
    IDX t = i / cv;
    const int j = (int)(t % 8); t /= 8;
    const int w2 = (int)(t % W2); t /= W2;
    const int h2 = (int)(t % H2); t /= H2;
    const int d2 = (int)(t % D2);
    const int b = (int)(t / D2);
    const int d = 2 * d2 + off.o[3 * j], h = 2 * h2 + off.o[3 * j + 1], w = 2 * w2 + off.o[3 * j + 2];
    V<T, VEC> v;
    if (d < D && h < H && w < W) v.load(src + ((((int64_t)b * D + d) * H + h) * W + w) * lds + c);
    else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) v.v[k] = 0.f;
    }
    v.store(dst + ((((int64_t)b * D2 + d2) * H2 + h2) * W2 + w2) * ldd + (int64_t)j * C + c);
  }
}

template <class T, int VEC, class IDX = int64_t>
__global__ void __launch_bounds__(256) c2s_kernel(const T* src, int64_t lds, T* dst, int64_t ldd, int B, int D, int H, int W, int C, Off8 off) {
  const int D2 = (D + 1) / 2, H2 = (H + 1) / 2, W2 = (W + 1) / 2, cv = C / VEC;
  const IDX total = (IDX)((int64_t)B * D * H * W * cv);
  for (IDX i = (IDX)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (IDX)gridDim.x * blockDim.x) {
    const int c = (int)(i % cv) * VEC;
    IDX t = i / cv;
    const int w = (int)(t % W); t /= W;
    const int h = (int)(t % H); t /= H;
    const int d = (int)(t % D);
    const int b = (int)(t / D);
    const int pd = d & 1, ph = h & 1, pw = w & 1;
    const T* srow = src + ((((int64_t)b * D2 + (d >> 1)) * H2 + (h >> 1)) * W2 + (w >> 1)) * lds + c;
    V<T, VEC> acc;
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc.v[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (off.o[3 * j] == pd && off.o[3 * j + 1] == ph && off.o[3 * j + 2] == pw) {
        V<T, VEC> v;
        v.load(srow + (int64_t)j * C);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] += v.v[k];
      }
    }
    acc.store(dst + ((((int64_t)b * D + d) * H + h) * W + w) * ldd + c);
  }
}

// ----------------------------------------------------------------------------- im2col / col2im (3x3x3 pad 1)
template <class T, int VEC>
__global__ void __launch_bounds__(256) im2col3_kernel(const T* src, int64_t lds, T* dst, int64_t ldd, int B, int D, int H, int W, int C) {
  const int cv = C / VEC;
  const int64_t total = (int64_t)B * D * H * W * 27 * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % cv) * VEC;
    int64_t t = i / cv;
    const int tap = (int)(t % 27); t /= 27;
    const int64_t v = t;
    const int w = (int)(t % W); t /= W;
    const int h = (int)(t % H); t /= H;
    const int d = (int)(t % D);
    const int b = (int)(t / D);
    const int dd = d + tap / 9 - 1, hh = h + (tap / 3) % 3 - 1, ww = w + tap % 3 - 1;
    V<T, VEC> val;
    if (dd >= 0 && dd < D && hh >= 0 && hh < H && ww >= 0 && ww < W) val.load(src + ((((int64_t)b * D + dd) * H + hh) * W + ww) * lds + c);
    else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) val.v[k] = 0.f;
    }
    val.store(dst + v * ldd + (int64_t)tap * C + c);
  }
}

template <class T, int VEC>
__global__ void __launch_bounds__(256) col2im3_kernel(const T* col, int64_t ldc, T* dst, int64_t ldd, int B, int D, int H, int W, int C) {
  const int cv = C / VEC;
  const int64_t total = (int64_t)B * D * H * W * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % cv) * VEC;
    int64_t t = i / cv;
    const int64_t v = t;
    const int w = (int)(t % W); t /= W;
    const int h = (int)(t % H); t /= H;
    const int d = (int)(t % D);
    const int b = (int)(t / D);
    V<T, VEC> acc;
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc.v[k] = 0.f;
    for (int tap = 0; tap < 27; ++tap) {
      // col[u][tap] holds src[u + off(tap)]  =>  dst[v] += col[v - off(tap)][tap]
      const int dd = d - (tap / 9 - 1), hh = h - ((tap / 3) % 3 - 1), ww = w - (tap % 3 - 1);
      if (dd >= 0 && dd < D && hh >= 0 && hh < H && ww >= 0 && ww < W) {
        V<T, VEC> val;
        val.load(col + ((((int64_t)b * D + dd) * H + hh) * W + ww) * ldc + (int64_t)tap * C + c);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] += val.v[k];
      }
    }
    acc.store(dst + v * ldd + c);
  }
}

// ----------------------------------------------------------------------------- column sums
// grid (row chunks, channel tiles); tx = 16-byte channel vector, ty walks rows; LDS reduce; one atomic per channel.
template <class T, int VEC>
__global__ void __launch_bounds__(256) colsum_kernel(const T* __restrict__ x, int64_t ldx, int64_t rows, int C, int cv, int tx_n, int ty_n,
                                                     float* __restrict__ out, int rows_per_block) {
  extern __shared__ float red[];
  const int tx = threadIdx.x % tx_n, ty = threadIdx.x / tx_n;
  const int c0 = blockIdx.y * tx_n, c = c0 + tx;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  float s[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = 0.f;
  if (ty < ty_n && c < cv) {
    for (int64_t r = r0 + ty; r < r1; r += ty_n) {
      V<T, VEC> v;
      v.load(x + r * ldx + c * VEC);
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] += v.v[i];
    }
  }
  if (ty < ty_n) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) red[ty * tx_n * VEC + tx * VEC + i] = s[i];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < tx_n * VEC; e += 256) {
    float acc = 0.f;
    for (int y = 0; y < ty_n; ++y) acc += red[y * tx_n * VEC + e];
    const int ch = c0 * VEC + e;
    if (ch < C) atomicAdd(out + ch, acc);
  }
}

struct ColsumBatch { miseg_colsum_desc d[MISEG_COLSUM_BATCH]; int n; };

// one launch for a list of accumulate-mode column sums: workgroup -> (descriptor, 512-row chunk, tile of 64 channels);
// a lane reads one 16-byte channel vector per row (vec descriptors) or single elements (any C / alignment)
static constexpr int CSB_ROWS = 512, CSB_CH = 64;

template <class T>
__global__ void __launch_bounds__(256) colsum_batch_kernel(ColsumBatch b) {
  typedef typename Vec16<T>::type VT;
  constexpr int N = Vec16<T>::N;
  __shared__ float red[32][CSB_CH + 1];
  int k = 0;
  while (k + 1 < b.n && b.d[k + 1].block0 <= (int)blockIdx.x) ++k;
  const miseg_colsum_desc d = b.d[k];
  const int ctiles = (d.C + CSB_CH - 1) / CSB_CH;
  const int local = blockIdx.x - d.block0;
  const int c0 = (local % ctiles) * CSB_CH;
  const int64_t r0 = (int64_t)(local / ctiles) * CSB_ROWS, r1 = min(d.rows, r0 + CSB_ROWS);
  const T* x = reinterpret_cast<const T*>(d.x);
  const bool vec = d.C % N == 0 && d.ldx % N == 0 && ((uintptr_t)d.x % 16 == 0);
  for (int i = threadIdx.x; i < 32 * (CSB_CH + 1); i += 256) (&red[0][0])[i] = 0.f;
  __syncthreads();
  if (vec) {
    constexpr int TX = CSB_CH / N, TY = 256 / TX;     // bf16: 8 x 32, fp32: 16 x 16
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int c = c0 + tx * N;
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
    if (c < d.C) {
      // eight rows in flight per lane (round 4: one dependent load per iteration streamed at 2.4 TB/s; rows beyond the chunk re-read its
      // last row and are not added)
      constexpr int U = 8;
      for (int64_t r = r0 + ty; r < r1; r += U * TY) {
        VT v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t ru = r + (int64_t)u * TY;
          v[u] = *reinterpret_cast<const VT*>(x + (ru < r1 ? ru : r1 - 1) * d.ldx + c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float keep = (r + (int64_t)u * TY) < r1 ? 1.f : 0.f;
#pragma unroll
          for (int e = 0; e < N; ++e) acc[e] = fmaf(keep, to_f32(v[u][e]), acc[e]);
        }
      }
    }
    // TY <= 32: one row of `red` per ty
#pragma unroll
    for (int e = 0; e < N; ++e) red[ty][tx * N + e] = acc[e];
  } else {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 channels x 4 row lanes
    const int c = c0 + tx;
    float acc = 0.f;
    if (c < d.C)
      for (int64_t r = r0 + ty; r < r1; r += 4) acc += to_f32(x[r * d.ldx + c]);
    red[ty][tx] = acc;
  }
  __syncthreads();
  if (threadIdx.x < CSB_CH && c0 + (int)threadIdx.x < d.C) {
    float t = 0.f;
#pragma unroll
    for (int y = 0; y < 32; ++y) t += red[y][threadIdx.x];
    atomicAdd(d.out + c0 + threadIdx.x, t);
  }
}

}  // namespace miseg

using namespace miseg;

extern "C" int miseg_affine2(const miseg_affine2_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_affine2_params), MISEG_E_BADARG, "affine2: struct_size");
  MISEG_REQUIRE(p->a && p->x && p->y && p->coef && p->B > 0 && p->S > 0 && p->C > 0, MISEG_E_BADARG, "affine2: bad args");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->lda, p->ldx, p->ldy}, {p->a, p->x, p->y});
    rowwise_launch<Affine2Op, T>(vec, (int64_t)p->B * p->S, p->C, 4096, s, (const T*)p->a, p->lda, (const T*)p->x, p->ldx, (T*)p->y, p->ldy, p->coef, p->S, p->C);
    MISEG_LAUNCH_CHECK("affine2");
  });
}

extern "C" int miseg_add(const miseg_add_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->a && p->b && p->y && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "add: bad args");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->lda, p->ldb, p->ldy}, {p->a, p->b, p->y});
    rowwise_launch<AddOp, T>(vec, p->rows, p->C, EW_GRID_CAP, s, (const T*)p->a, p->lda, (const T*)p->b, p->ldb, (T*)p->y, p->ldy);
    MISEG_LAUNCH_CHECK("add");
  });
}

extern "C" int miseg_copy2d(const miseg_copy2d_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->src && p->dst && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "copy2d: bad args");
  const int g = ew_grid(p->rows * p->C);
  if (p->sdtype == MISEG_F32 && p->ddtype == MISEG_F32) copy2d_kernel<float, float><<<g, 256, 0, s>>>((const float*)p->src, p->lds, (float*)p->dst, p->ldd, p->rows, p->C);
  else if (p->sdtype == MISEG_F32 && p->ddtype == MISEG_BF16) copy2d_kernel<float, bf16><<<g, 256, 0, s>>>((const float*)p->src, p->lds, (bf16*)p->dst, p->ldd, p->rows, p->C);
  else if (p->sdtype == MISEG_BF16 && p->ddtype == MISEG_F32) copy2d_kernel<bf16, float><<<g, 256, 0, s>>>((const bf16*)p->src, p->lds, (float*)p->dst, p->ldd, p->rows, p->C);
  else if (p->sdtype == MISEG_BF16 && p->ddtype == MISEG_BF16) copy2d_kernel<bf16, bf16><<<g, 256, 0, s>>>((const bf16*)p->src, p->lds, (bf16*)p->dst, p->ldd, p->rows, p->C);
  else return set_error(MISEG_E_BADARG, "copy2d: dtypes %d -> %d", p->sdtype, p->ddtype);
  MISEG_LAUNCH_CHECK("copy2d");
  return MISEG_OK;
}

extern "C" int miseg_cast_matrix(const miseg_cast_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->src && p->dst && p->R > 0 && p->C > 0, MISEG_E_BADARG, "cast_matrix: bad args");
  DT(p, {
    if (p->transpose) cast_transpose_kernel<T><<<dim3(cdiv(p->C, 32), cdiv(p->R, 32)), 256, 0, s>>>(p->src, (T*)p->dst, p->R, p->C);
    else cast_kernel<T><<<ew_grid((int64_t)p->R * p->C), 256, 0, s>>>(p->src, (T*)p->dst, (int64_t)p->R * p->C);
    MISEG_LAUNCH_CHECK("cast_matrix");
  });
}

extern "C" int miseg_gelu_bwd(const miseg_gelu_bwd_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->dy && p->x && p->dx && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "gelu_bwd: bad args");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->lddy, p->ldx, p->lddx}, {p->dy, p->x, p->dx});
    rowwise_launch<GeluBwdOp, T>(vec, p->rows, p->C, EW_GRID_CAP, s, (const T*)p->dy, p->lddy, (const T*)p->x, p->ldx, (T*)p->dx, p->lddx);
    MISEG_LAUNCH_CHECK("gelu_bwd");
  });
}

extern "C" int miseg_gelu_fwd(const miseg_gelu_fwd_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->x && p->y && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "gelu_fwd: bad args");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->ldx, p->ldy}, {p->x, p->y});
    rowwise_launch<GeluFwdOp, T>(vec, p->rows, p->C, EW_GRID_CAP, s, (const T*)p->x, p->ldx, (T*)p->y, p->ldy);
    MISEG_LAUNCH_CHECK("gelu_fwd");
  });
}

static int s2c_common(const miseg_s2c_params* p, hipStream_t s, bool gather) {
  MISEG_REQUIRE(p && p->src && p->dst && p->B > 0 && p->D > 0 && p->H > 0 && p->W > 0 && p->C > 0, MISEG_E_BADARG, "space/channel: bad args");
  Off8 off;
  for (int i = 0; i < 24; ++i) {
    off.o[i] = p->offsets[i];
    MISEG_REQUIRE(off.o[i] == 0 || off.o[i] == 1, MISEG_E_BADARG, "space/channel: offsets must be 0/1");
  }
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->lds, p->ldd}, {p->src, p->dst});
    const int64_t tot = gather ? (int64_t)p->B * ((p->D + 1) / 2) * ((p->H + 1) / 2) * ((p->W + 1) / 2) * 8 : (int64_t)p->B * p->D * p->H * p->W;
    vec_pick<T>(vec, p->C, [&](auto vc, int cv) {
      constexpr int VEC = decltype(vc)::value;
      auto launch = [&](auto* kernel) { kernel<<<ew_grid(tot * cv), 256, 0, s>>>((const T*)p->src, p->lds, (T*)p->dst, p->ldd, p->B, p->D, p->H, p->W, p->C, off); };
      if constexpr (VEC > 1)      // the 16-byte form has a 32-bit instantiation (see s2c_kernel)
        if (tot * cv < (1LL << 30)) return launch(gather ? s2c_kernel<T, VEC, unsigned> : c2s_kernel<T, VEC, unsigned>);
      launch(gather ? s2c_kernel<T, VEC> : c2s_kernel<T, VEC>);
    });
    MISEG_LAUNCH_CHECK("space/channel");
  });
}
extern "C" int miseg_space_to_channel(const miseg_s2c_params* p, miseg_stream_t s) { return s2c_common(p, (hipStream_t)s, true); }
extern "C" int miseg_channel_to_space(const miseg_s2c_params* p, miseg_stream_t s) { return s2c_common(p, (hipStream_t)s, false); }

static int im2col_common(const miseg_im2col3_params* p, hipStream_t s, bool fwd) {
  MISEG_REQUIRE(p && p->src && p->dst && p->B > 0 && p->C > 0, MISEG_E_BADARG, "im2col3: bad args");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->lds, p->ldd}, {p->src, p->dst});
    const int64_t nv = (int64_t)p->B * p->D * p->H * p->W;
    vec_pick<T>(vec, p->C, [&](auto vc, int cv) {
      constexpr int VEC = decltype(vc)::value;
      if (fwd) im2col3_kernel<T, VEC><<<ew_grid(nv * 27 * cv), 256, 0, s>>>((const T*)p->src, p->lds, (T*)p->dst, p->ldd, p->B, p->D, p->H, p->W, p->C);
      else col2im3_kernel<T, VEC><<<ew_grid(nv * cv), 256, 0, s>>>((const T*)p->src, p->lds, (T*)p->dst, p->ldd, p->B, p->D, p->H, p->W, p->C);
    });
    MISEG_LAUNCH_CHECK("im2col3");
  });
}
extern "C" int miseg_im2col3(const miseg_im2col3_params* p, miseg_stream_t s) { return im2col_common(p, (hipStream_t)s, true); }
extern "C" int miseg_col2im3(const miseg_im2col3_params* p, miseg_stream_t s) { return im2col_common(p, (hipStream_t)s, false); }

extern "C" int miseg_colsum(const miseg_colsum_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->x && p->out && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "colsum: bad args");
  MISEG_REQUIRE(p->dtype == MISEG_F32 || p->dtype == MISEG_BF16, MISEG_E_BADARG, "colsum: unknown dtype %d", p->dtype);      // before the fill
  if (!p->accumulate) {
    hipError_t e = miseg::fill_words_async(p->out, 0, (size_t)p->C, s);
    MISEG_REQUIRE(e == hipSuccess, MISEG_E_LAUNCH, "colsum: memset failed");
  }
  DT(p, {
    constexpr int N = Vec16<T>::N;
    const bool vec = vec16_ok(N, {p->C, p->ldx}, {p->x});
    const int cv = vec ? p->C / N : p->C;
    const int tx = cv < 32 ? cv : 32, ty = 256 / tx;
    const int rpb = p->rows >= 65536 ? 512 : 128;
    dim3 grid(cdiv(p->rows, rpb), cdiv(cv, tx));
    const size_t sh = (size_t)ty * tx * (vec ? N : 1) * sizeof(float);
    if (vec) colsum_kernel<T, N><<<grid, 256, sh, s>>>((const T*)p->x, p->ldx, p->rows, p->C, cv, tx, ty, p->out, rpb);
    else colsum_kernel<T, 1><<<grid, 256, sh, s>>>((const T*)p->x, p->ldx, p->rows, p->C, cv, tx, ty, p->out, rpb);
    MISEG_LAUNCH_CHECK("colsum");
  });
}

namespace miseg {
template <class T>
__global__ void __launch_bounds__(256) ncdhw_to_rows_kernel(const float* __restrict__ x, T* __restrict__ y, int Cin, int64_t S, int64_t total) {
  typedef typename Vec16<T>::type VT;
  constexpr int N = Vec16<T>::N;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / S, v = i - b * S;
    VT o;
#pragma unroll
    for (int c = 0; c < N; ++c) o[c] = from_f32<T>(c < Cin ? x[(b * Cin + c) * S + v] : 0.f);
    *reinterpret_cast<VT*>(y + i * N) = o;
  }
}
}  // namespace miseg

extern "C" int miseg_ncdhw_to_rows(const float* x, void* y, int B, int Cin, int64_t S, int CP, int dtype, miseg_stream_t s_) {
  MISEG_REQUIRE(x && y && B > 0 && S > 0 && Cin > 0, MISEG_E_BADARG, "ncdhw_to_rows: bad arguments");
  return dispatch_dtype(dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    MISEG_REQUIRE(CP == Vec16<T>::N && Cin <= CP, MISEG_E_UNSUPPORTED, "ncdhw_to_rows: CP must be %d and Cin <= CP", Vec16<T>::N);
    MISEG_REQUIRE((uintptr_t)y % 16 == 0, MISEG_E_BADARG, "ncdhw_to_rows: y must be 16-byte aligned");
    const int64_t total = (int64_t)B * S;
    miseg::ncdhw_to_rows_kernel<T><<<ew_grid(total), 256, 0, (hipStream_t)s_>>>(x, (T*)y, Cin, S, total);
    MISEG_LAUNCH_CHECK("ncdhw_to_rows");
    return MISEG_OK;
  });
}

namespace miseg {
template <class T>
__global__ void __launch_bounds__(256) param_cast_batch_kernel(const miseg_cast_desc* __restrict__ descs, int ndesc, int total_tiles,
                                                               const int64_t* __restrict__ params_version, int64_t* __restrict__ state) {
  __shared__ float tile[32][33];
  constexpr int NS = 512;
  __shared__ int s_tile0[NS];      // the descriptors' first tiles: the per-tile search reads LDS, not a chain of dependent global loads (round 4)
  // versioned refresh (miseg_hip.h): nothing to do when the copies were made from the current parameters
  const int64_t pv = params_version ? *params_version : 0;
  if (params_version && state[0] == pv) return;
  const bool in_lds = ndesc <= NS;
  if (in_lds) {
    for (int i = threadIdx.x; i < ndesc; i += 256) s_tile0[i] = descs[i].tile0;
    __syncthreads();
  }
  for (int tl = blockIdx.x; tl < total_tiles; tl += gridDim.x) {
    // binary search: last descriptor with tile0 <= tl
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((in_lds ? s_tile0[mid] : descs[mid].tile0) <= tl) lo = mid; else hi = mid - 1;
    }
    const miseg_cast_desc d = descs[lo];
    const int t = tl - d.tile0, tc = (d.C + 31) / 32;
    const int by = (t / tc) * 32, bx = (t % tc) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    T* dst = (T*)d.dst;
    // whole 32 x 32 tiles of 16-byte aligned rows (round 4): one float4 load per thread; the plain cast stores 4 converted values per thread
    // straight from registers, the transposed one 4 consecutive rows of a column from the LDS tile - element-wise 4-byte loads and 2-byte
    // stores streamed at 1.7 TB/s (120 us per live refresh of C-Swin-UNETR's 25 M non-conv weights)
    const bool whole = by + 32 <= d.R && bx + 32 <= d.C && (d.C & 3) == 0;
    if (whole) {
      const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
      const f32x4 v = *reinterpret_cast<const f32x4*>(d.src + (int64_t)(by + r) * d.C + bx + c4);
      if (!d.transpose && d.inner == 1) {
        T o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(v[e]);
        T* q = dst + (int64_t)(by + r) * d.C + bx + c4;
        if (sizeof(T) == 2 && (reinterpret_cast<uintptr_t>(q) & 7) == 0) *reinterpret_cast<uint2*>(q) = *reinterpret_cast<const uint2*>(o);
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) q[e] = o[e];
        }
        continue;
      }
      __syncthreads();                                       // the tile buffer of the previous iteration has been read
      tile[r][c4] = v[0]; tile[r][c4 + 1] = v[1]; tile[r][c4 + 2] = v[2]; tile[r][c4 + 3] = v[3];
      __syncthreads();
      if (d.transpose && (d.R & 3) == 0) {
        const int j = threadIdx.x >> 3, r4 = (threadIdx.x & 7) * 4, c = bx + j;      // column c, rows by + r4 .. + 3
        T o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(tile[r4 + e][j]);
        T* q = dst + (int64_t)((c % d.inner) * d.outer + c / d.inner) * d.R + by + r4;
        if (sizeof(T) == 2 && (reinterpret_cast<uintptr_t>(q) & 7) == 0) *reinterpret_cast<uint2*>(q) = *reinterpret_cast<const uint2*>(o);
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) q[e] = o[e];
        }
        continue;
      }
    } else {
      __syncthreads();                                       // the tile buffer of the previous iteration has been read
      for (int j = ty; j < 32; j += 8)
        if (by + j < d.R && bx + tx < d.C) tile[j][tx] = d.src[(int64_t)(by + j) * d.C + bx + tx];
      __syncthreads();
    }
    if (d.transpose) {
      for (int j = ty; j < 32; j += 8) {
        const int c = bx + j;
        if (c < d.C && by + tx < d.R) dst[(int64_t)((c % d.inner) * d.outer + c / d.inner) * d.R + by + tx] = from_f32<T>(tile[tx][j]);
      }
    } else {
      for (int j = ty; j < 32; j += 8) {
        const int c = bx + tx;
        if (by + j < d.R && c < d.C) dst[(int64_t)(by + j) * d.C + (c % d.inner) * d.outer + c / d.inner] = from_f32<T>(tile[j][tx]);
      }
    }
  }
  refresh_done(params_version, state, pv);
}
}  // namespace miseg

extern "C" int miseg_param_cast_batch(const miseg_cast_desc* descs, int ndesc, int total_tiles, int dtype, const int64_t* params_version, int64_t* state,
                                      miseg_stream_t s_) {
  MISEG_REQUIRE(descs && ndesc > 0 && total_tiles > 0, MISEG_E_BADARG, "param_cast_batch: bad arguments");
  MISEG_REQUIRE((params_version == nullptr) == (state == nullptr), MISEG_E_BADARG, "param_cast_batch: params_version and state go together");
  return dispatch_dtype(dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    static const int cap = miseg::refresh_max_wg("MISEG_CAST_WG", miseg::REFRESH_CAST_WG);
    miseg::param_cast_batch_kernel<T><<<total_tiles < cap ? total_tiles : cap, 256, 0, (hipStream_t)s_>>>(descs, ndesc, total_tiles, params_version, state);
    MISEG_LAUNCH_CHECK("param_cast_batch");
    return MISEG_OK;
  });
}

namespace miseg {
// dir 0: y[coarse] = x[2 * coarse]; dir 1: y[fine] = (all coordinates even) ? x[fine / 2] : 0.   One thread per output element vector.
template <class T, int VEC>
__global__ void __launch_bounds__(256) resample2_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy, int B, int D, int H, int W, int cv,
                                                        int dir) {
  const int D2 = (D + 1) / 2, H2 = (H + 1) / 2, W2 = (W + 1) / 2;
  const int od = dir ? D : D2, oh = dir ? H : H2, ow = dir ? W : W2;
  const int64_t total = (int64_t)B * od * oh * ow * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cv) * VEC;
    int64_t t = i / cv;
    const int w = (int)(t % ow); t /= ow;
    const int h = (int)(t % oh); t /= oh;
    const int d = (int)(t % od);
    const int b = (int)(t / od);
    const int64_t orow = ((((int64_t)b * od + d) * oh + h) * ow + w);
    V<T, VEC> v;
#pragma unroll
    for (int k = 0; k < VEC; ++k) v.v[k] = 0.f;
    if (!dir) v.load(x + ((((int64_t)b * D + 2 * d) * H + 2 * h) * W + 2 * w) * ldx + c);
    else if (!((d | h | w) & 1)) v.load(x + ((((int64_t)b * D2 + d / 2) * H2 + h / 2) * W2 + w / 2) * ldx + c);
    v.store(y + orow * ldy + c);
  }
}

template <class T, int VEC>
__global__ void __launch_bounds__(256) prelu_bwd_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ x, int64_t ldx, const float* __restrict__ slope,
                                                        T* __restrict__ dx, int64_t lddx, float* __restrict__ dslope, int64_t rows, int cv,
                                                        double* __restrict__ scratch) {
  __shared__ float red[4];
  const float a = slope[0];
  const int64_t total = rows * cv;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cv;
    const int c = (int)(i % cv) * VEC;
    V<T, VEC> g, xv;
    g.load(dy + r * lddy + c);
    xv.load(x + r * ldx + c);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (!(xv.v[k] > 0.f)) { acc = fmaf(g.v[k], xv.v[k], acc); g.v[k] *= a; }
    }
    g.store(dx + r * lddx + c);
  }
  if (dslope) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      // the slope gradient is ONE number, a sum over every voxel with heavy cancellation: the workgroup partials meet in float64 (fp32 atomics
      // in arrival order were off by up to 60 % on the 64^3 UNet and not reproducible), the last workgroup to arrive hands the total over.
      // The add returns its old value and the wave waits for it (s_waitcnt: the add has been performed) before it takes its arrival
      // ticket - a dependency written in C++ ("cond ? 1 : 1") is folded away and the ticket could overtake the add.
      const double part = ((double)red[0] + (double)red[1]) + ((double)red[2] + (double)red[3]);
      const double before = atomicAdd(scratch, part);
      asm volatile("s_waitcnt vmcnt(0)" : : "v"(before) : "memory");
      unsigned long long* ticket = reinterpret_cast<unsigned long long*>(scratch + 1);
      const unsigned long long arrived = atomicAdd(ticket, 1ull);
      if (arrived == (unsigned long long)gridDim.x - 1) atomicAdd(dslope, (float)atomicAdd(scratch, 0.0));
    }
  }
}

// rows [B][S][C] <-> NCDHW fp32; the tile transpose keeps both sides coalesced
template <class T>
__global__ void __launch_bounds__(256) layout_ncdhw_kernel(const T* __restrict__ rows_in, T* __restrict__ rows_out, int64_t ld, const float* __restrict__ nc_in,
                                                           float* __restrict__ nc_out, int C, int64_t S, int dir) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int64_t s0 = (int64_t)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  if (!dir) {
    for (int j = ty; j < 32; j += 8)
      if (s0 + j < S && c0 + tx < C) tile[j][tx] = to_f32(rows_in[((int64_t)b * S + s0 + j) * ld + c0 + tx]);
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
      if (c0 + j < C && s0 + tx < S) nc_out[((int64_t)b * C + c0 + j) * S + s0 + tx] = tile[tx][j];
  } else {
    for (int j = ty; j < 32; j += 8)
      if (c0 + j < C && s0 + tx < S) tile[j][tx] = nc_in[((int64_t)b * C + c0 + j) * S + s0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
      if (s0 + j < S && c0 + tx < C) rows_out[((int64_t)b * S + s0 + j) * ld + c0 + tx] = from_f32<T>(tile[tx][j]);
  }
}
}  // namespace miseg

extern "C" int miseg_resample2(const miseg_resample2_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->x && p->y && p->B > 0 && p->D > 0 && p->H > 0 && p->W > 0 && p->C > 0, MISEG_E_BADARG, "resample2: bad args");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->ldx, p->ldy}, {p->x, p->y});
    const int64_t vox = p->dir ? (int64_t)p->B * p->D * p->H * p->W : (int64_t)p->B * ((p->D + 1) / 2) * ((p->H + 1) / 2) * ((p->W + 1) / 2);
    vec_pick<T>(vec, p->C, [&](auto vc, int cv) {
      resample2_kernel<T, decltype(vc)::value><<<ew_grid(vox * cv), 256, 0, s>>>((const T*)p->x, p->ldx, (T*)p->y, p->ldy, p->B, p->D, p->H, p->W, cv, p->dir);
    });
    MISEG_LAUNCH_CHECK("resample2");
  });
}

namespace miseg {
// nearest upsample by f (1 or 2) of x into the right half of a channel concat: out[fine row] = [skip[fine row] | x[fine row / f]].  One
// workgroup per fine (b, z, y) line; its lanes walk the line's W * (cvs + cvu) 16-byte vectors (or elements when VEC == 1) in order, so every
// wave-instruction touches consecutive bytes of out and, per half, of one input row run.  The line's coarse row is scalar arithmetic.
template <class T, int VEC>
__global__ void __launch_bounds__(256) upsample_cat_kernel(const T* __restrict__ skip, int64_t ldskip, const T* __restrict__ x, int64_t ldx, T* __restrict__ out,
                                                           int64_t ldout, int D, int H, int W, int cvs, int cvu, int f) {
  const int line = blockIdx.x;                       // (b * D + z) * H + y
  const int y = line % H, bz = line / H;
  const int z = bz % D, b = bz / D;
  const int Dc = D / f, Hc = H / f, Wc = W / f;
  const int64_t row0 = (int64_t)line * W;
  const int64_t crow0 = (((int64_t)b * Dc + z / f) * Hc + y / f) * Wc;
  const int cvt = cvs + cvu;
  const int n = W * cvt;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int w = i / cvt;
    const int c = i - w * cvt;
    const int64_t r = row0 + w;
    V<T, VEC> v;
    if (c < cvs) v.load(skip + r * ldskip + c * VEC);
    else v.load(x + (crow0 + w / f) * ldx + (c - cvs) * VEC);
    v.store(out + r * ldout + c * VEC);
  }
}

// adjoint of the right half: dx[coarse row] = sum over the f^3 children (dz, dy, dx in that order) of dcat[child row], fp32, rounded once.
// One workgroup per `lpb` consecutive coarse (b, z', y') lines (the host picks lpb so that the lanes divide the work evenly: a 48-voxel line of
// 8 vectors is 384 items, two lines are three full rounds of 256 lanes).  No atomics, so the result does not depend on scheduling.
template <class T, int VEC>
__global__ void __launch_bounds__(256) upsample_cat_bwd_kernel(const T* __restrict__ dcat, int64_t lddcat, T* __restrict__ dx, int64_t lddx, int D, int H, int W,
                                                               int cv, int f, int lines, int lpb) {
  const int Dc = D / f, Hc = H / f, Wc = W / f;
  const int n1 = Wc * cv;
  const int n = lpb * n1;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int l = i / n1;
    const int line = blockIdx.x * lpb + l;           // (b * Dc + z') * Hc + y'
    if (line >= lines) break;
    const int y = line % Hc, bz = line / Hc;
    const int z = bz % Dc, b = bz / Dc;
    const int j = i - l * n1;
    const int w = j / cv;
    const int c = (j - w * cv) * VEC;
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    for (int dz = 0; dz < f; ++dz)
      for (int dy = 0; dy < f; ++dy) {
        const int64_t frow = (((int64_t)b * D + z * f + dz) * H + y * f + dy) * W + (int64_t)w * f;
        for (int dw = 0; dw < f; ++dw) {
          V<T, VEC> g;
          g.load(dcat + (frow + dw) * lddcat + c);
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] += g.v[k];
        }
      }
    V<T, VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
    o.store(dx + ((int64_t)line * Wc + w) * lddx + c);
  }
}
}  // namespace miseg

extern "C" int miseg_upsample_cat(const miseg_upsample_cat_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->skip && p->x && p->out && p->B > 0 && p->D > 0 && p->H > 0 && p->W > 0 && p->Cs > 0 && p->Cu > 0, MISEG_E_BADARG,
                "upsample_cat: bad args");
  MISEG_REQUIRE(p->factor == 1 || p->factor == 2, MISEG_E_BADARG, "upsample_cat: factor %d (1 or 2)", p->factor);
  MISEG_REQUIRE(p->D % p->factor == 0 && p->H % p->factor == 0 && p->W % p->factor == 0, MISEG_E_BADARG,
                "upsample_cat: fine grid %dx%dx%d is not %d x a coarse grid", p->D, p->H, p->W, p->factor);
  MISEG_REQUIRE(p->ldskip >= p->Cs && p->ldx >= p->Cu && p->ldout >= p->Cs + p->Cu, MISEG_E_BADARG, "upsample_cat: a leading dimension is below its channel count");
  const int64_t lines = (int64_t)p->B * p->D * p->H;
  MISEG_REQUIRE(lines < (1ll << 31) && (int64_t)p->W * (p->Cs + p->Cu) < (1ll << 31), MISEG_E_BADARG, "upsample_cat: grid too large");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->Cs, p->Cu, p->ldskip, p->ldx, p->ldout}, {p->skip, p->x, p->out});
    vec_pick<T>(vec, p->Cs, [&](auto vc, int cvs) {
      constexpr int VEC = decltype(vc)::value;
      upsample_cat_kernel<T, VEC><<<(unsigned)lines, 256, 0, s>>>((const T*)p->skip, p->ldskip, (const T*)p->x, p->ldx, (T*)p->out, p->ldout, p->D, p->H, p->W, cvs,
                                                                 p->Cu / VEC, p->factor);
    });
    MISEG_LAUNCH_CHECK("upsample_cat");
  });
}

extern "C" int miseg_upsample_cat_bwd(const miseg_upsample_cat_bwd_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->dcat && p->dx && p->B > 0 && p->D > 0 && p->H > 0 && p->W > 0 && p->C > 0, MISEG_E_BADARG, "upsample_cat_bwd: bad args");
  MISEG_REQUIRE(p->factor == 1 || p->factor == 2, MISEG_E_BADARG, "upsample_cat_bwd: factor %d (1 or 2)", p->factor);
  MISEG_REQUIRE(p->D % p->factor == 0 && p->H % p->factor == 0 && p->W % p->factor == 0, MISEG_E_BADARG,
                "upsample_cat_bwd: fine grid %dx%dx%d is not %d x a coarse grid", p->D, p->H, p->W, p->factor);
  MISEG_REQUIRE(p->lddcat >= p->C && p->lddx >= p->C, MISEG_E_BADARG, "upsample_cat_bwd: a leading dimension is below the channel count");
  const int64_t lines = (int64_t)p->B * (p->D / p->factor) * (p->H / p->factor);
  MISEG_REQUIRE(lines < (1ll << 31) && 4ll * p->W * p->C < (1ll << 31), MISEG_E_BADARG, "upsample_cat_bwd: grid too large");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->lddcat, p->lddx}, {p->dcat, p->dx});
    vec_pick<T>(vec, p->C, [&](auto vc, int cv) {
      const int64_t n1 = (int64_t)(p->W / p->factor) * cv;
      int lpb = 1;                                     // lines per workgroup: the best lane utilisation over 1..4 lines, the fewer lines on a tie
      double best = 0.0;
      for (int k = 1; k <= 4 && k * n1 < (1ll << 31); ++k) {
        const double u = (double)(k * n1) / (256.0 * (double)((k * n1 + 255) / 256));
        if (u > best + 1e-9) { best = u; lpb = k; }
      }
      const unsigned grid = (unsigned)((lines + lpb - 1) / lpb);
      upsample_cat_bwd_kernel<T, decltype(vc)::value><<<grid, 256, 0, s>>>((const T*)p->dcat, p->lddcat, (T*)p->dx, p->lddx, p->D, p->H, p->W, cv, p->factor, (int)lines, lpb);
    });
    MISEG_LAUNCH_CHECK("upsample_cat_bwd");
  });
}

extern "C" int miseg_rowbias_add(const miseg_rowbias_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->x && p->y && p->bias && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "rowbias_add: bad args");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->ldx, p->ldy}, {p->x, p->y});
    rowwise_launch<RowBiasOp, T>(vec, p->rows, p->C, EW_GRID_CAP, s, (const T*)p->x, p->ldx, p->bias, (T*)p->y, p->ldy);
    MISEG_LAUNCH_CHECK("rowbias_add");
  });
}

extern "C" int miseg_prelu_fwd(const miseg_prelu_fwd_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->x && p->y && p->slope && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "prelu_fwd: bad args");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->ldx, p->ldy}, {p->x, p->y});
    rowwise_launch<PreluFwdOp, T>(vec, p->rows, p->C, EW_GRID_CAP, s, (const T*)p->x, p->ldx, p->slope, (T*)p->y, p->ldy);
    MISEG_LAUNCH_CHECK("prelu_fwd");
  });
}

extern "C" int miseg_prelu_bwd(const miseg_prelu_bwd_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->dy && p->x && p->dx && p->slope && p->rows > 0 && p->C > 0, MISEG_E_BADARG, "prelu_bwd: bad args");
  MISEG_REQUIRE(!p->dslope || p->scratch, MISEG_E_BADARG, "prelu_bwd: dslope needs the zeroed double[2] scratch");
  DT(p, {
    const bool vec = vec16_ok(Vec16<T>::N, {p->C, p->lddy, p->ldx, p->lddx}, {p->dy, p->x, p->dx});
    vec_pick<T>(vec, p->C, [&](auto vc, int cv) {
      const int grid = ew_grid(p->rows * cv, 1024);      // one atomic per workgroup on the single slope gradient
      prelu_bwd_kernel<T, decltype(vc)::value><<<grid, 256, 0, s>>>((const T*)p->dy, p->lddy, (const T*)p->x, p->ldx, p->slope, (T*)p->dx, p->lddx, p->dslope, p->rows, cv, p->scratch);
    });
    MISEG_LAUNCH_CHECK("prelu_bwd");
  });
}

extern "C" int miseg_layout_ncdhw(const void* rows_, int64_t ld, float* ncdhw, int B, int C, int64_t S, int dtype, int dir, miseg_stream_t s_) {
  MISEG_REQUIRE(rows_ && ncdhw && B > 0 && C > 0 && S > 0 && ld >= C, MISEG_E_BADARG, "layout_ncdhw: bad args");
  return dispatch_dtype(dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    dim3 grid((unsigned)((S + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
    miseg::layout_ncdhw_kernel<T><<<grid, 256, 0, (hipStream_t)s_>>>((const T*)rows_, (T*)const_cast<void*>(rows_), ld, ncdhw, ncdhw, C, S, dir);
    MISEG_LAUNCH_CHECK("layout_ncdhw");
    return MISEG_OK;
  });
}

extern "C" int miseg_colsum_batch(const miseg_colsum_desc* descs, int n, int dtype, miseg_stream_t s_) {
  MISEG_REQUIRE(descs && n > 0 && n <= MISEG_COLSUM_BATCH, MISEG_E_BADARG, "colsum_batch: 1..%d descriptors", MISEG_COLSUM_BATCH);
  miseg::ColsumBatch b;
  int blocks = 0;
  for (int i = 0; i < n; ++i) {
    MISEG_REQUIRE(descs[i].x && descs[i].out && descs[i].rows > 0 && descs[i].C > 0, MISEG_E_BADARG, "colsum_batch: descriptor %d", i);
    b.d[i] = descs[i];
    b.d[i].block0 = blocks;
    blocks += (int)((descs[i].rows + miseg::CSB_ROWS - 1) / miseg::CSB_ROWS) * ((descs[i].C + miseg::CSB_CH - 1) / miseg::CSB_CH);
  }
  b.n = n;
  return dispatch_dtype(dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    miseg::colsum_batch_kernel<T><<<blocks, 256, 0, (hipStream_t)s_>>>(b);
    MISEG_LAUNCH_CHECK("colsum_batch");
    return MISEG_OK;
  });
}

// up to MISEG_FILL_RANGES word ranges of one buffer in ONE launch (the gradient arena minus the slots a kernel will overwrite whole, round 5):
// ranges are 16-byte aligned (arena slots are) and a multiple of 4 words long except possibly the last
namespace miseg {
struct FillRanges { uint64_t off[MISEG_FILL_RANGES], len[MISEG_FILL_RANGES], start[MISEG_FILL_RANGES + 1]; int n; };
static __global__ void __launch_bounds__(256) fill_ranges_kernel(uint32_t* __restrict__ dst, uint32_t v, FillRanges r) {
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  const u32x4 vv = {v, v, v, v};
  const uint64_t total4 = r.start[r.n];                       // in 16-byte units over all ranges (each range rounded up)
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (uint64_t)gridDim.x * 256) {
    int k = 0;
    while (k + 1 < r.n && r.start[k + 1] <= i) ++k;
    const uint64_t w = (i - r.start[k]) * 4;                  // word offset inside range k
    uint32_t* p = dst + r.off[k] + w;
    if (w + 4 <= r.len[k]) *reinterpret_cast<u32x4*>(p) = vv;
    else for (uint64_t e = w; e < r.len[k]; ++e) dst[r.off[k] + e] = v;
  }
}
}  // namespace miseg

extern "C" int miseg_fill32_ranges(void* dst, uint32_t value, const uint64_t* ranges_host, int n, miseg_stream_t s_) {
  MISEG_REQUIRE(dst && ranges_host && n >= 1 && n <= MISEG_FILL_RANGES, MISEG_E_BADARG, "fill32_ranges: 1..%d ranges", MISEG_FILL_RANGES);
  MISEG_REQUIRE(((uintptr_t)dst % 16) == 0, MISEG_E_BADARG, "fill32_ranges: the buffer must be 16-byte aligned");
  miseg::FillRanges r;
  r.n = n;
  uint64_t acc = 0;
  for (int i = 0; i < n; ++i) {
    r.off[i] = ranges_host[2 * i];
    r.len[i] = ranges_host[2 * i + 1];
    MISEG_REQUIRE(r.off[i] % 4 == 0 && r.len[i] > 0, MISEG_E_BADARG, "fill32_ranges: range %d (offset %llu words, %llu words): offsets are multiples of 4 words", i,
                  (unsigned long long)r.off[i], (unsigned long long)r.len[i]);
    r.start[i] = acc;
    acc += (r.len[i] + 3) / 4;
  }
  r.start[n] = acc;
  miseg::fill_ranges_kernel<<<ew_grid((int64_t)acc, 4096), 256, 0, (hipStream_t)s_>>>((uint32_t*)dst, value, r);
  MISEG_LAUNCH_CHECK("fill32_ranges");
  return MISEG_OK;
}

extern "C" int miseg_fill32(void* dst, uint32_t value, size_t n, miseg_stream_t s_) {
  MISEG_REQUIRE(dst || n == 0, MISEG_E_BADARG, "fill32: null pointer");
  if (n == 0) return MISEG_OK;
  hipError_t e = miseg::fill_words_async(dst, value, n, (hipStream_t)s_);
  MISEG_REQUIRE(e == hipSuccess, MISEG_E_LAUNCH, "fill32: %s", hipGetErrorString(e));
  return MISEG_OK;
}
