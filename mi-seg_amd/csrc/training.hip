// What runs right after the hot path every training / validation step, all HBM-bound:
//   * DiceFocal / DiceCE / GeneralizedDiceFocal loss: one pass for the per-(b,c) sums + loss, one for d(loss)/d(logits)    (lightning_monai.py:46-67,
//                                                                                                               utils/training_utils.py:26-33)
//   * Dice metric after argmax / one-hot                                                                     (lightning_monai.py:68-79,190-195)
//   * AdamW / Adam / SGD-nesterov step of EVERY parameter in one launch over the gradient arena              (lightning_monai.py:255-278)
//   * sliding-window stitching as one gather over resident window logits                                     (lightning_monai.py:86-93,187)
//   * the prediction export: argmax + inverse pad / spacing / orientation + class remap as one gather           (predict_whs.py:92-114)
// MONAI 1.1.0 arithmetic restated from its public API (parity unpinned by any reference test).
#include "common.h"
#include "opt_math.h"
#include "../../include/miseg_hip_debug.h"
#include <math.h>

namespace miseg {

constexpr int LOSS_MAXC = 16;          // channels kept in registers per voxel
#ifndef MISEG_LOSS_VEC
#define MISEG_LOSS_VEC 4               // voxels per thread of the vector instantiations (4: one 16-byte load per channel)
#endif
constexpr int LOSS_VEC = MISEG_LOSS_VEC;
constexpr int LOSS_VPB = 256 * LOSS_VEC;         // voxels per workgroup (256 threads x 1 float4 group; round 5: 2048 left 1.7 workgroups per CU - a chain of
                                       // transcendentals per voxel with nobody to hide it: 50 / 59 us forward / backward on the 96^3 x 6 logits)

template <class L> __device__ __forceinline__ int label_at(const L* lab, int64_t i) { return (int)lab[i]; }

struct LossGeom {
  int B, C, kind, c0, sq, wt;
  int64_t S;
  float gamma;
};

// value of the per-element focal term and its derivative w.r.t. x (MONAI 1.1.0 FocalLoss, sigmoid form on raw logits):
//   ce = x - x t + softplus(-x);   w = exp(gamma * logsigmoid(-x z)), z = 2 t - 1;   f = w ce
// The target is one-hot (t is 0 or 1), so with u = x z, e = exp(-|x|) = exp(-|u|) and L = log1p(e) everything comes from ONE exponential and
// ONE logarithm:  softplus(+-u) = max(+-u, 0) + L;   ce = softplus(-u);   logsigmoid(-u) = -softplus(u);   sigmoid(u) = u >= 0 ? r : e r and
// sigmoid(-u) = u >= 0 ? e r : r with r = 1 / (1 + e);   sigmoid(x) - t = -z sigmoid(-u).  (Round 5: the literal form evaluated two
// softplus and two sigmoids per channel - 5 exp, 2 log1p, 2 divisions - a dependent chain of ~250 instructions per element and the reason
// the two loss kernels took 48 / 56 us on 21 MB of logits; it also lost ce to cancellation for t = 0, x << 0, where this form is exact.)
template <bool GRAD>
__device__ __forceinline__ void focal_term(float x, float t, float gamma, float& f, float& df) {
  const bool pos = t != 0.f;
  const float u = pos ? x : -x;
  const float e = expf(-fabsf(x));
  const float L = log1pf(e);
  const float ce = fmaxf(-u, 0.f) + L;                  // softplus(-u)
  const float w = expf(-gamma * (fmaxf(u, 0.f) + L));   // exp(gamma logsigmoid(-u))
  f = w * ce;
  if (GRAD) {
    const float r = __builtin_amdgcn_rcpf(1.f + e);
    const float su = u >= 0.f ? r : e * r, snu = u >= 0.f ? e * r : r;      // sigmoid(u), sigmoid(-u)
    const float d = w * (gamma * su * ce + snu);        // df/du
    df = pos ? -d : d;                                   // du/dx = z, and the bracket carries -z
  }
}

// softmax over channels [c0s, C) of x -> p (p[c < c0s] = 0); returns log-sum-exp
template <int MAXC> __device__ __forceinline__ float softmax_from(const float (&x)[MAXC], float (&p)[MAXC], int c0s, int C) {
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) if (c >= c0s && c < C) mx = fmaxf(mx, x[c]);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    p[c] = (c >= c0s && c < C) ? expf(x[c] - mx) : 0.f;
    sum += p[c];
  }
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) p[c] *= inv;
  return mx + logf(sum);
}

// GeneralizedDiceLoss / compute_generalized_dice class weights (MONAI 1.1.0; utils/training_utils.py:26-33, tune.py:124-129):
// 1/G^2 | 1/G | 1 of the label count G; an infinite weight (class absent from the sample) becomes the largest finite one of the sample's kept
// classes, 0 when there is none.  q: the sample's [C][3] sums or counts with G at q[3 c + 2].
__device__ __forceinline__ double gdice_raw_weight(double G, int wt) {
  return wt == MISEG_GDICE_W_UNIFORM ? 1.0 : wt == MISEG_GDICE_W_SIMPLE ? 1.0 / G : 1.0 / (G * G);
}
template <class T> __device__ __forceinline__ double gdice_max_weight(const T* q, int c0, int C, int wt) {
  double m = 0.0;
  for (int c = c0; c < C; ++c) {
    const double w = gdice_raw_weight((double)q[3 * c + 2], wt);
    if (w <= 1.7976931348623157e308 && w > m) m = w;
  }
  return m;
}
__device__ __forceinline__ double gdice_weight(double G, int wt, double wmax) {
  const double w = gdice_raw_weight(G, wt);
  return w <= 1.7976931348623157e308 ? w : wmax;
}

// grid (blocks per sample, B).  part: double [B][nblk][3 C + 1]
template <class L, int MAXC, int VEC>
__global__ void __launch_bounds__(256) seg_loss_fwd_kernel(const float* __restrict__ logits, const L* __restrict__ label, LossGeom g, double* __restrict__ part) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int c0d = g.c0, c0s = g.kind == MISEG_LOSS_DICE_FOCAL ? g.c0 : 0;   // dice_ce / gdice_focal: softmax over all channels, channel 0 dropped after
  const float* xb = logits + (int64_t)b * g.C * g.S;
  const L* lb = label + (int64_t)b * g.S;
  float aI[MAXC], aP[MAXC], aT[MAXC], aO = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) aI[c] = aP[c] = aT[c] = 0.f;
  const int64_t base = (int64_t)blockIdx.x * LOSS_VPB;
  for (int it = 0; it < LOSS_VPB / (256 * VEC); ++it) {
    const int64_t s0 = base + ((int64_t)it * 256 + tid) * VEC;
    if (s0 >= g.S) break;
    float xv[MAXC][VEC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < g.C) {
        if constexpr (VEC == 4) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(xb + (int64_t)c * g.S + s0);
#pragma unroll
          for (int v = 0; v < 4; ++v) xv[c][v] = t[v];
        } else if constexpr (VEC == 2) {
          const float2 t = *reinterpret_cast<const float2*>(xb + (int64_t)c * g.S + s0);
          xv[c][0] = t.x; xv[c][1] = t.y;
        } else xv[c][0] = xb[(int64_t)c * g.S + s0];
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) xv[c][v] = 0.f;
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      if (s0 + v >= g.S) break;
      const int lab = label_at(lb, s0 + v);
      float x[MAXC], p[MAXC];
#pragma unroll
      for (int c = 0; c < MAXC; ++c) x[c] = xv[c][v];
      const float lse = softmax_from<MAXC>(x, p, c0s, g.C);
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        if (c >= c0d && c < g.C) {
          const float t = (lab == c) ? 1.f : 0.f;
          aI[c] += p[c] * t;
          aP[c] += g.sq ? p[c] * p[c] : p[c];
          aT[c] += t;
          if (g.kind != MISEG_LOSS_DICE_CE) {
            float f, df;
            focal_term<false>(x[c], t, g.gamma, f, df);
            aO += f;
          }
        }
      }
      if (g.kind == MISEG_LOSS_DICE_CE) {
        float xl = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) if (c == lab) xl = x[c];
        aO += lse - xl;
      }
    }
  }
  __shared__ float red[4][3 * MAXC + 1];
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    if (c < g.C) {       // uniform branch
      const float i = wave_sum(aI[c]), pp = wave_sum(aP[c]), t = wave_sum(aT[c]);
      if (lane == 0) { red[wave][3 * c] = i; red[wave][3 * c + 1] = pp; red[wave][3 * c + 2] = t; }
    }
  }
  const float o = wave_sum(aO);
  if (lane == 0) red[wave][3 * MAXC] = o;
  __syncthreads();
  const int nv = 3 * g.C + 1;
  if (tid < nv) {
    const int src = tid < 3 * g.C ? tid : 3 * MAXC;
    const double v = ((double)red[0][src] + (double)red[1][src]) + ((double)red[2][src] + (double)red[3][src]);
    part[((int64_t)b * gridDim.x + blockIdx.x) * nv + tid] = v;
  }
}

// one workgroup: sums[b][c][k] = sum over blocks (fixed order), sums[3 B C] = total of the focal / CE term, loss scalar.
// One WAVE per (sample, value): a lane adds every 64th block partial, the 64 lane sums meet in a shuffle tree (round 5: the 256-thread LDS
// tree took 8 barriers per value, 19 values per sample one after the other - 23 us for what is 7 additions per lane).
static __global__ void __launch_bounds__(1024) seg_loss_finalize_kernel(const double* __restrict__ part, int nblk, LossGeom g, float nr, float dr, float ld, float lo,
                                                                     double* __restrict__ sums, float* __restrict__ loss) {
  const int nv = 3 * g.C + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = blockDim.x >> 6;
  __shared__ double other[64];
  for (int job = wave; job < g.B * nv; job += nwave) {
    const int b = job / nv, v = job - b * nv;
    double a = 0.0;
    for (int k = lane; k < nblk; k += 64) a += part[((int64_t)b * nblk + k) * nv + v];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) {
      if (v < 3 * g.C) sums[(int64_t)b * 3 * g.C + v] = a;
      else other[b] = a;
    }
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    double tot_o = 0.0, dice = 0.0;
    for (int b = 0; b < g.B; ++b) {
      tot_o += other[b];
      for (int c = g.c0; c < g.C; ++c) {
        const double* q = sums + ((int64_t)b * g.C + c) * 3;
        dice += 1.0 - (2.0 * q[0] + nr) / (q[2] + q[1] + dr);
      }
    }
    const int cn = g.C - g.c0;
    sums[(int64_t)3 * g.B * g.C] = tot_o;
    const double o_mean = g.kind != MISEG_LOSS_DICE_CE ? tot_o / ((double)g.B * cn * g.S) : tot_o / ((double)g.B * g.S);
    if (g.kind == MISEG_LOSS_GDICE_FOCAL) {      // one term per SAMPLE: the classes meet in the weighted numerator / denominator
      double gd = 0.0;
      for (int b = 0; b < g.B; ++b) {
        const double* q = sums + (int64_t)b * g.C * 3;
        const double wmax = gdice_max_weight(q, g.c0, g.C, g.wt);
        double num = 0.0, den = 0.0;
        for (int c = g.c0; c < g.C; ++c) {
          const double w = gdice_weight(q[3 * c + 2], g.wt, wmax);
          num += w * q[3 * c];
          den += w * (q[3 * c + 2] + q[3 * c + 1]);
        }
        gd += 1.0 - (2.0 * num + nr) / (den + dr);
      }
      *loss = (float)(ld * gd / (double)g.B + lo * o_mean);
      return;
    }
    *loss = (float)(ld * dice / ((double)g.B * cn) + lo * o_mean);
  }
}

// GD: the gdice_focal kind.  A template parameter, not a run-time test: the fp64 coefficient prologue below cost the MAXC = 16 instantiation of
// the other kinds 117 VGPRs and two thirds of its occupancy when it sat behind `g.kind`.
template <class L, int MAXC, int VEC, bool GD>
__global__ void __launch_bounds__(256) seg_loss_bwd_kernel(const float* __restrict__ logits, const L* __restrict__ label, LossGeom g, float nr, float dr, float ld, float lo,
                                                           const double* __restrict__ sums, const float* __restrict__ gscale, float* __restrict__ dlogits) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int c0d = g.c0, c0s = (GD || g.kind == MISEG_LOSS_DICE_CE) ? 0 : g.c0;
  const int cn = g.C - g.c0;
  const float gs = gscale ? *gscale : 1.f;
  // per-channel Dice coefficients: dD/dp = ca t + cb p (squared) | ca t + cb (plain)
  float ca[MAXC], cb[MAXC];
  if constexpr (GD) {
    // dL/dp = ca t + cb with ca = -2 k w / den_b, cb = k num_b w / den_b^2, k = lambda gscale / B; num_b, den_b couple the classes of the
    // sample.  w reaches 1e-12 (1 / G^2, G up to 96^3), so thread c forms the quotients of class c in fp64 and rounds them once; the
    // others pick them up from LDS.
    __shared__ float coef[2 * MAXC];
    if (tid < MAXC) {
      float a = 0.f, bb = 0.f;
      if (tid >= c0d && tid < g.C) {
        const double* q = sums + (int64_t)b * g.C * 3;
        const double wmax = gdice_max_weight(q, c0d, g.C, g.wt);
        double num = 0.0, den = 0.0;
        for (int c = c0d; c < g.C; ++c) {
          const double w = gdice_weight(q[3 * c + 2], g.wt, wmax);
          num += w * q[3 * c];
          den += w * (q[3 * c + 2] + q[3 * c + 1]);
        }
        const double numb = 2.0 * num + nr, denb = den + dr, k = (double)ld * gs / (double)g.B;
        const double w = gdice_weight(q[3 * tid + 2], g.wt, wmax);
        a = (float)(-2.0 * k * w / denb);
        bb = (float)(k * numb * w / (denb * denb));
      }
      coef[2 * tid] = a; coef[2 * tid + 1] = bb;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { ca[c] = coef[2 * c]; cb[c] = coef[2 * c + 1]; }
  } else {
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      ca[c] = cb[c] = 0.f;
      if (c >= c0d && c < g.C) {
        const double* q = sums + ((int64_t)b * g.C + c) * 3;
        const double den = q[2] + q[1] + dr, num = 2.0 * q[0] + nr, k = (double)ld * gs / ((double)g.B * cn);
        ca[c] = (float)(-2.0 * k / den);
        cb[c] = (float)((g.sq ? 2.0 : 1.0) * k * num / (den * den));
      }
    }
  }
  const float ko = (GD || g.kind == MISEG_LOSS_DICE_FOCAL) ? lo * gs / ((float)g.B * cn * (float)g.S) : lo * gs / ((float)g.B * (float)g.S);
  const float* xb = logits + (int64_t)b * g.C * g.S;
  float* db = dlogits + (int64_t)b * g.C * g.S;
  const L* lb = label + (int64_t)b * g.S;
  const int64_t base = (int64_t)blockIdx.x * LOSS_VPB;
  for (int it = 0; it < LOSS_VPB / (256 * VEC); ++it) {
    const int64_t s0 = base + ((int64_t)it * 256 + tid) * VEC;
    if (s0 >= g.S) break;
    float xv[MAXC][VEC], dv[MAXC][VEC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < g.C) {
        if constexpr (VEC == 4) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(xb + (int64_t)c * g.S + s0);
#pragma unroll
          for (int v = 0; v < 4; ++v) xv[c][v] = t[v];
        } else if constexpr (VEC == 2) {
          const float2 t = *reinterpret_cast<const float2*>(xb + (int64_t)c * g.S + s0);
          xv[c][0] = t.x; xv[c][1] = t.y;
        } else xv[c][0] = xb[(int64_t)c * g.S + s0];
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) xv[c][v] = 0.f;
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int lab = (s0 + v < g.S) ? label_at(lb, s0 + v) : 0;
      float x[MAXC], p[MAXC], G[MAXC];
#pragma unroll
      for (int c = 0; c < MAXC; ++c) x[c] = xv[c][v];
      softmax_from<MAXC>(x, p, c0s, g.C);
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        const float t = (lab == c) ? 1.f : 0.f;
        G[c] = ca[c] * t + (!GD && g.sq ? cb[c] * p[c] : cb[c]);       // zero outside the Dice channels (ca = cb = 0)
        dot += G[c] * p[c];
      }
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        const float t = (lab == c) ? 1.f : 0.f;
        float d = p[c] * (G[c] - dot);                            // softmax Jacobian; p = 0 outside the softmax support
        if (GD || g.kind == MISEG_LOSS_DICE_FOCAL) {
          if (c >= c0d && c < g.C) {
            float f, df;
            focal_term<true>(x[c], t, g.gamma, f, df);
            d += ko * df;
          }
        } else if (c < g.C) d += ko * (p[c] - t);                 // CE: softmax over all channels is p itself (c0s = 0)
        dv[c][v] = d;
      }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < g.C) {
        if constexpr (VEC == 4) {
          f32x4 t;
#pragma unroll
          for (int v = 0; v < 4; ++v) t[v] = dv[c][v];
          *reinterpret_cast<f32x4*>(db + (int64_t)c * g.S + s0) = t;
        } else if constexpr (VEC == 2) {
          *reinterpret_cast<float2*>(db + (int64_t)c * g.S + s0) = float2{dv[c][0], dv[c][1]};
        } else db[(int64_t)c * g.S + s0] = dv[c][0];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ Dice metric
template <class L, int MAXC>
__global__ void __launch_bounds__(256) dice_count_kernel(const float* __restrict__ logits, const L* __restrict__ label, int C, int64_t S, unsigned long long* __restrict__ counts) {
  __shared__ int cnt[3 * MAXC];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid < 3 * MAXC) cnt[tid] = 0;
  __syncthreads();
  const float* xb = logits + (int64_t)b * C * S;
  const L* lb = label + (int64_t)b * S;
  for (int64_t s = (int64_t)blockIdx.x * 256 + tid; s < S; s += (int64_t)gridDim.x * 256) {
    int arg = 0;
    float mx = xb[s];
    for (int c = 1; c < C; ++c) {
      const float v = xb[(int64_t)c * S + s];
      if (v > mx) { mx = v; arg = c; }            // strict: the FIRST maximum wins (torch.argmax)
    }
    const int lab = label_at(lb, s);
    atomicAdd(&cnt[3 * arg + 1], 1);
    if (lab >= 0 && lab < C) {
      atomicAdd(&cnt[3 * lab + 2], 1);
      if (lab == arg) atomicAdd(&cnt[3 * arg], 1);
    }
  }
  __syncthreads();
  if (tid < 3 * C && cnt[tid]) atomicAdd(&counts[(int64_t)b * 3 * C + tid], (unsigned long long)cnt[tid]);
}

// gdice (optional): GeneralizedDiceScore from the same counts, by the thread of each sample's class 0, in double (DESIGN.md section 7.4 rules 6-7)
static __global__ void dice_finalize_kernel(const unsigned long long* __restrict__ counts, int n, float* __restrict__ dice, int C, int c0, int wt,
                                            float* __restrict__ gdice) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double inter = (double)counts[3 * i], np = (double)counts[3 * i + 1], nl = (double)counts[3 * i + 2];
  dice[i] = nl > 0 ? (float)(2.0 * inter / (np + nl)) : __int_as_float(0x7fc00000);
  if (!gdice || i % C) return;
  const unsigned long long* q = counts + (int64_t)3 * i;      // the sample's [C][3]
  const double wmax = gdice_max_weight(q, c0, C, wt);
  double num = 0.0, den = 0.0;
  unsigned long long npred = 0;
  for (int c = c0; c < C; ++c) {
    const double w = gdice_weight((double)q[3 * c + 2], wt, wmax);
    num += w * (double)q[3 * c];
    den += w * ((double)q[3 * c + 2] + (double)q[3 * c + 1]);
    npred += q[3 * c + 1];
  }
  gdice[i / C] = den == 0.0 ? (npred == 0 ? 1.f : 0.f) : (float)(2.0 * num / den);
}

// ------------------------------------------------------------------------------------------------ optimiser
constexpr int OPT_BLOCK = 4096;     // elements per workgroup (256 threads x 4 float4)

// CLIP (miseg_opt_step_clipped): the update runs on opt_clip(gradient) and a skipped step (rec->skip) returns before any store; the plain
// instantiation never looks at rec / clip_mode / clip_value
template <bool CLIP>
__global__ void __launch_bounds__(256) opt_step_kernel(const miseg_opt_desc* __restrict__ descs, int ndesc, int kind, const float* __restrict__ grad, float* __restrict__ s1,
                                                     float* __restrict__ s2, const int32_t* __restrict__ used, int32_t* __restrict__ steps, float lr, float b1, float b2,
                                                     float eps, float wd, float mom, const float* __restrict__ lr_dev, const int32_t* __restrict__ index,
                                                     const miseg_grad_clip_record* __restrict__ rec, int clip_mode, float clip_value) {
  float clip_c = clip_value;      // the bound of value mode, the record's coefficient of norm mode
  if constexpr (CLIP) {
    if (rec && rec->skip) return;
    if (clip_mode == MISEG_CLIP_NORM) clip_c = rec->coef;
  }
  // descriptor of this workgroup: the last one with block0 <= blockIdx.x
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const miseg_opt_desc d = descs[lo];
  const int pi = index ? index[lo] : lo;             // the parameter's row in used / steps (a table may hold a subset of the parameters)
  if (used && !used[pi]) return;
  if (lr_dev) lr = *lr_dev;
  const int blk = blockIdx.x - d.block0;
  // (steps[pi]: read by every workgroup of the tensor; written back by a separate tiny launch)
  const OptHyper hy = opt_hyper(kind, steps[pi] + 1, lr, b1, b2, eps, wd, mom);
  float* p = d.param;
  const float* gp = grad + d.off;
  float* m = s1 + d.off;
  float* v = s2 ? s2 + d.off : nullptr;
  const int e0 = blk * OPT_BLOCK;
  const bool vec = (((uintptr_t)p) & 15) == 0;      // arena slots are 16-byte aligned; a parameter view may not be
  for (int it = 0; it < 4; ++it) {
    const int e = e0 + (it * 256 + threadIdx.x) * 4;
    if (e >= d.n) break;
    const int cnt = d.n - e < 4 ? d.n - e : 4;
    float pv[4], gv[4], mv[4], vv[4];
    if (vec && cnt == 4) {
      const f32x4 tp = *reinterpret_cast<const f32x4*>(p + e), tg = *reinterpret_cast<const f32x4*>(gp + e), tm = *reinterpret_cast<const f32x4*>(m + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) { pv[k] = tp[k]; gv[k] = tg[k]; mv[k] = tm[k]; }
      if (v) {
        const f32x4 tv = *reinterpret_cast<const f32x4*>(v + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) vv[k] = tv[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = k < cnt;
        pv[k] = ok ? p[e + k] : 0.f; gv[k] = ok ? gp[e + k] : 0.f; mv[k] = ok ? m[e + k] : 0.f; vv[k] = (ok && v) ? v[e + k] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) opt_update(hy, pv[k], CLIP ? opt_clip(clip_mode, clip_c, gv[k]) : gv[k], mv[k], vv[k]);
    if (vec && cnt == 4) {
      f32x4 tp, tm, tv;
#pragma unroll
      for (int k = 0; k < 4; ++k) { tp[k] = pv[k]; tm[k] = mv[k]; tv[k] = vv[k]; }
      *reinterpret_cast<f32x4*>(p + e) = tp;
      *reinterpret_cast<f32x4*>(m + e) = tm;
      if (v) *reinterpret_cast<f32x4*>(v + e) = tv;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) { p[e + k] = pv[k]; m[e + k] = mv[k]; if (v) v[e + k] = vv[k]; }
    }
  }
}

static __global__ void opt_count_kernel(const int32_t* __restrict__ used, int32_t* __restrict__ steps, int n, int64_t* __restrict__ params_version,
                                        int64_t* __restrict__ pack_state, const miseg_grad_clip_record* __restrict__ rec) {
  if (rec && rec->skip) return;      // a skipped step (non-finite gradient) is no update: no count, no version
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!used || used[i])) steps[i] += 1;
  if (i == 0 && params_version) {
    *params_version += 1;      // the parameters changed: the versioned refresh kernels re-lay-out their copies
    if (pack_state) pack_state[0] = *params_version;      // ... except the packs the fused launch in front of this one has just written (opt_math.h)
  }
}

// ------------------------------------------------------------------------------------------------ gradient norm (miseg_grad_norm)
// fixed shuffle tree over the 64 lanes of a wave (offsets 32, 16, .., 1): lane 0 holds the sum
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Launch 1: opt_step_kernel's geometry (one workgroup per 4096-element block of the table) over the gradient arena alone.  Squares and sums
// in double: a thread's 16 elements in ascending order, the shuffle tree, the four waves in order through LDS; one plain store per block.
static __global__ void __launch_bounds__(256) grad_sqsum_kernel(const miseg_opt_desc* __restrict__ descs, int ndesc, const float* __restrict__ grad,
                                                              const int32_t* __restrict__ used, double* __restrict__ part) {
  __shared__ double s_wave[4];
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {      // the last descriptor with block0 <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  if (used && !used[lo]) {      // `grad is None`: the slot is not read (it may hold anything) and adds nothing
    if (threadIdx.x == 0) part[blockIdx.x] = 0.0;
    return;
  }
  const miseg_opt_desc d = descs[lo];
  const float* gp = grad + d.off;
  const int e0 = ((int)blockIdx.x - d.block0) * OPT_BLOCK;
  const bool vec = (((uintptr_t)gp) & 15) == 0;
  f32x4 g[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {      // (all four loads in flight before the first add)
    const int e = e0 + (it * 256 + threadIdx.x) * 4;
    const int cnt = d.n - e;
    if (vec && cnt >= 4) {
      g[it] = *reinterpret_cast<const f32x4*>(gp + e);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) g[it][k] = k < cnt ? gp[e + k] : 0.f;
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += (double)g[it][k] * (double)g[it][k];
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// Launch 2, one workgroup of 16 waves (the order is written out in miseg_hip.h): per-tensor sums into dsum, then their sum, then the record.
constexpr int GN_THREADS = 1024, GN_WAVES = GN_THREADS / 64, GN_UNROLL = 4, GN_DEPTH = 16;
constexpr int GN_LDS_DESCS = 2048;      // block0 of this many descriptors is staged in LDS (one coalesced read instead of two dependent loads per tensor)

static __global__ void __launch_bounds__(GN_THREADS) grad_norm_finish_kernel(const miseg_opt_desc* __restrict__ descs, int ndesc, int total_blocks,
                                                                           const double* __restrict__ part, double* __restrict__ dsum, int mode, float max_norm,
                                                                           int skip_nonfinite, miseg_grad_clip_record* __restrict__ rec, float* __restrict__ per_param) {
  __shared__ int s_block0[GN_LDS_DESCS + 1];
  __shared__ double s_wave[GN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool in_lds = ndesc <= GN_LDS_DESCS;
  if (in_lds) {
    for (int i = tid; i <= ndesc; i += GN_THREADS) s_block0[i] = i < ndesc ? descs[i].block0 : total_blocks;
    __syncthreads();
  }
  // A wave takes GN_UNROLL tensors at a time and has the first partial of each in flight before it adds anything: one tensor per round was a
  // chain of 17 dependent memory round trips per wave on the headline net's 265 tensors (29.7 us for 120 KB of partials).  Which wave adds a
  // tensor does not change its sum: lane l adds the tensor's partials l, l + 64, ... in ascending order, then the shuffle tree.
  for (int i0 = wave * GN_UNROLL; i0 < ndesc; i0 += GN_WAVES * GN_UNROLL) {
    int b0[GN_UNROLL], b1[GN_UNROLL];
    double acc[GN_UNROLL];
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u) {
      const int i = i0 + u;
      b0[u] = b1[u] = 0;
      if (i < ndesc) {
        b0[u] = in_lds ? s_block0[i] : descs[i].block0;
        b1[u] = in_lds ? s_block0[i + 1] : (i + 1 < ndesc ? descs[i + 1].block0 : total_blocks);
        b1[u] = b1[u] < total_blocks ? b1[u] : total_blocks;      // (a table that disagrees with total_blocks reads no partial outside the workspace)
      }
      acc[u] = b0[u] + lane < b1[u] ? part[b0[u] + lane] : 0.0;
    }
    // the rest of a large tensor (the headline net's largest has 3888 partials, 61 a lane): GN_DEPTH loads in flight, added in ascending
    // order (a partial is >= 0, so the + 0.0 of a lane that ran out changes no bit)
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u)
      for (int b = b0[u] + lane + 64; b < b1[u]; b += 64 * GN_DEPTH) {
        double v[GN_DEPTH];
#pragma unroll
        for (int k = 0; k < GN_DEPTH; ++k) v[k] = b + 64 * k < b1[u] ? part[b + 64 * k] : 0.0;
#pragma unroll
        for (int k = 0; k < GN_DEPTH; ++k) acc[u] += v[k];
      }
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u) acc[u] = wave_sum_f64(acc[u]);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < GN_UNROLL; ++u)
        if (i0 + u < ndesc) {
          dsum[i0 + u] = acc[u];
          if (per_param) per_param[i0 + u] = (float)sqrt(acc[u]);
        }
    }
  }
  __syncthreads();      // (dsum was written by this workgroup: visible to it after the barrier)
  double acc = 0.0;
  for (int i = tid; i < ndesc; i += GN_THREADS) acc += dsum[i];
  acc = wave_sum_f64(acc);
  if (lane == 0) s_wave[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    double S = 0.0;
    for (int w = 0; w < GN_WAVES; ++w) S += s_wave[w];
    const float norm = (float)sqrt(S);
    const float coef = mode == MISEG_CLIP_NORM ? fminf(1.f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f))) : 1.f;
    const int finite = isfinite(norm) ? 1 : 0, skip = (skip_nonfinite && !finite) ? 1 : 0;
    rec->norm = norm;
    rec->coef = coef;
    rec->finite = finite;
    rec->skip = skip;
    rec->seen += 1u;
    rec->clipped += coef < 1.f ? 1u : 0u;
    rec->skipped += skip ? 1u : 0u;
    rec->reserved = 0u;
  }
}

// ------------------------------------------------------------------------------------------------ gradient accumulation (miseg_grad_fold)
// opt_step_kernel's geometry over the gradient arena and the window's accumulator `acc` (laid out like the arena).  ops[i] of parameter i:
// bit 0 (u) = it has a gradient in this micro-batch, bit 1 (a) = it had one earlier in the window, bit 2 (F) = this micro-batch closes the
// window.  v = u && a ? fl(acc + g) : u ? g : acc;  F: arena = fl(v * scale), else acc = v - and nothing at all without u unless F && a.  A
// buffer's slot is loaded only where the table in miseg_hip.h says it is read (the branches are uniform over the workgroup), and the sum and
// the product are rounded on their own.  A pure stream: all of a thread's loads are in flight before its first add; no LDS, no atomics.
// The loads are non-temporal (`global_load_dwordx4 .. nt`), the stores plain: both buffers are read once per launch and each is about as large as
// the Infinity Cache for the headline net.  Measured on the headline arena (3 x 249 MB per launch): 118 us with nt loads against 139 - 144 us with plain loads
// and 131 us with nt loads AND nt stores.
__device__ __forceinline__ f32x4 fold_ld(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
static __global__ void __launch_bounds__(256) grad_fold_kernel(const miseg_opt_desc* __restrict__ descs, int ndesc, float* __restrict__ grad,
                                                             float* __restrict__ acc, const int32_t* __restrict__ ops, float scale) {
#pragma clang fp contract(off)
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {      // the last descriptor with block0 <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int op = ops[lo];
  const bool u = (op & 1) != 0, a = (op & 2) != 0, fin = (op & 4) != 0;
  if (!u && !(fin && a)) return;      // ops 0, 2, 4: neither buffer's slot is read or written
  const miseg_opt_desc d = descs[lo];
  float* gp = grad + d.off;
  float* ap = acc + d.off;
  float* out = fin ? gp : ap;
  const int e0 = ((int)blockIdx.x - d.block0) * OPT_BLOCK;
  const bool vec = ((((uintptr_t)gp) | ((uintptr_t)ap)) & 15) == 0;
  f32x4 g[4], s[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = e0 + (it * 256 + threadIdx.x) * 4;
    const int cnt = d.n - e;
    if (vec && cnt >= 4) {
      g[it] = u ? fold_ld(gp + e) : f32x4{0.f, 0.f, 0.f, 0.f};
      s[it] = a ? fold_ld(ap + e) : f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g[it][k] = (u && k < cnt) ? gp[e + k] : 0.f;
        s[it][k] = (a && k < cnt) ? ap[e + k] : 0.f;
      }
    }
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = e0 + (it * 256 + threadIdx.x) * 4;
    const int cnt = d.n - e;
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float sum = s[it][k] + g[it][k];
      const float t = (u && a) ? sum : (u ? g[it][k] : s[it][k]);
      v[k] = fin ? t * scale : t;
    }
    if (vec && cnt >= 4) {
      *reinterpret_cast<f32x4*>(out + e) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) out[e + k] = v[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight averaging (miseg_weight_average, miseg_weight_swap)
// The tick: ONE thread turns the record's counters into this call's decision (apply, first, coef - the rules are written out in miseg_hip.h).
// A launch of its own, so that no workgroup of the streaming launch behind it reads a word another workgroup of its launch writes.
static __global__ void weight_average_tick_kernel(miseg_weight_average_record* __restrict__ rec, const miseg_grad_clip_record* __restrict__ clip, int mode,
                                                  float decay, int warmup, int start, int every) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (clip && clip->skip) return;      // the step wrote no weight: not a call
  const uint32_t t = rec->calls, n = rec->n_averaged;
  const int64_t since = (int64_t)t - (int64_t)start;
  const int apply = (since >= 0 && since % (int64_t)every == 0) ? 1 : 0;
  rec->calls = t + 1u;
  rec->apply = apply;
  rec->first = n == 0u ? 1 : 0;
  if (apply) {
    const float fn = (float)n;
    float c;
    if (mode == MISEG_AVG_MEAN) {
      c = __fdiv_rn(1.0f, (float)(n + 1u));
    } else {
      const float dn = warmup ? fminf(decay, __fdiv_rn(__fadd_rn(1.0f, fn), __fadd_rn(10.0f, fn))) : decay;
      c = __fsub_rn(1.0f, dn);
    }
    rec->coef = c;
    rec->n_averaged = n + 1u;
  }
}

// The stream: opt_step_kernel's geometry over the parameters (read) and `avg` (read unless first, written).  All of a thread's loads are in
// flight before its first subtract; no LDS, no atomics; the difference, the product and the sum are rounded on their own.
// Both sides are loaded non-temporally (fold_ld: `global_load_dwordx4 .. nt`), the stores are plain.
// Measured on the headline arena (3 x 249 MB per launch; miseg_grad_fold op 3 in the same process: 117 us), kernel alone / what averaging
// every step adds to the captured train step:  nt both 118.7 us / +179 us;  nt weights only 113.5 us / +207 us;  nt average only
// 135.7 us / +213 us;  plain both 145.8 us / +201 us.  The weights were written by the launch just before, but 249 MB of them and as much of
// their moments passed through a 256 MiB Infinity Cache since: neither side is found there, and both are read once.  Kept: nt on both - the
// smallest median inside the step, where it counts, and level with the fold alone; nt on the weights only is 5 us faster alone, but its step
// median is 17 us slower, over a range (6.486 .. 6.554 ms) that contains the other's (6.491 .. 6.518 ms): not a difference to build on.
static __global__ void __launch_bounds__(256) weight_average_kernel(const miseg_opt_desc* __restrict__ descs, int ndesc, float* __restrict__ avg,
                                                                  const miseg_weight_average_record* __restrict__ rec,
                                                                  const miseg_grad_clip_record* __restrict__ clip) {
#pragma clang fp contract(off)
  if (clip && clip->skip) return;      // (the tick left the record alone: it still holds the call before)
  if (!rec->apply) return;
  const bool first = rec->first != 0;
  const float c = rec->coef;
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {      // the last descriptor with block0 <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const miseg_opt_desc d = descs[lo];
  const float* wp = d.param;
  float* ap = avg + d.off;
  const int e0 = ((int)blockIdx.x - d.block0) * OPT_BLOCK;
  const bool vec = ((((uintptr_t)wp) | ((uintptr_t)ap)) & 15) == 0;      // arena slots are 16-byte aligned; a parameter view may not be
  f32x4 w[4], a[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = e0 + (it * 256 + threadIdx.x) * 4;
    const int cnt = d.n - e;
    if (vec && cnt >= 4) {
      w[it] = fold_ld(wp + e);
      a[it] = first ? f32x4{0.f, 0.f, 0.f, 0.f} : fold_ld(ap + e);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[it][k] = k < cnt ? wp[e + k] : 0.f;
        a[it][k] = (!first && k < cnt) ? ap[e + k] : 0.f;
      }
    }
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = e0 + (it * 256 + threadIdx.x) * 4;
    const int cnt = d.n - e;
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float diff = w[it][k] - a[it][k];
      const float step = c * diff;
      v[k] = first ? w[it][k] : a[it][k] + step;
    }
    if (vec && cnt >= 4) {
      *reinterpret_cast<f32x4*>(ap + e) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) ap[e + k] = v[k];
    }
  }
}

// The exchange param <-> avg in the same geometry: every element is read from both sides and stored to the other (loads non-temporal: each
// word is read once; stores plain).  Thread 0 of workgroup 0 bumps the parameter version - a word no other workgroup of the launch looks at.
static __global__ void __launch_bounds__(256) weight_swap_kernel(const miseg_opt_desc* __restrict__ descs, int ndesc, float* __restrict__ avg,
                                                               int64_t* __restrict__ params_version) {
#pragma clang fp contract(off)
  if (params_version && blockIdx.x == 0 && threadIdx.x == 0) *params_version += 1;      // the parameters change: the versioned refresh re-lays-out its copies
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {      // the last descriptor with block0 <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const miseg_opt_desc d = descs[lo];
  float* wp = d.param;
  float* ap = avg + d.off;
  const int e0 = ((int)blockIdx.x - d.block0) * OPT_BLOCK;
  const bool vec = ((((uintptr_t)wp) | ((uintptr_t)ap)) & 15) == 0;
  f32x4 w[4], a[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = e0 + (it * 256 + threadIdx.x) * 4;
    const int cnt = d.n - e;
    if (vec && cnt >= 4) {
      w[it] = fold_ld(wp + e);
      a[it] = fold_ld(ap + e);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[it][k] = k < cnt ? wp[e + k] : 0.f;
        a[it][k] = k < cnt ? ap[e + k] : 0.f;
      }
    }
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = e0 + (it * 256 + threadIdx.x) * 4;
    const int cnt = d.n - e;
    if (vec && cnt >= 4) {
      *reinterpret_cast<f32x4*>(wp + e) = a[it];
      *reinterpret_cast<f32x4*>(ap + e) = w[it];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) { wp[e + k] = a[it][k]; ap[e + k] = w[it][k]; }
    }
  }
}

// ------------------------------------------------------------------------------------------------ stitching
struct StitchArgs {
  int C, D, H, W, rd, rh, rw, nd, nh, nw, d0;
  int sd[MISEG_STITCH_MAX_WINDOWS], sh[MISEG_STITCH_MAX_WINDOWS], sw[MISEG_STITCH_MAX_WINDOWS];
};

// windows of one axis covering coordinate x: starts are non-decreasing, so they form a contiguous index range [lo, hi]
__device__ __forceinline__ void cover(const int* st, int n, int r, int x, int& lo, int& hi) {
  lo = n; hi = -1;
  for (int i = 0; i < n; ++i)
    if (st[i] <= x && x < st[i] + r) { if (lo == n) lo = i; hi = i; }
}

// grid (ceil(W/64 / 4)..., H, D): thread = one voxel; channels looped (C small).  Reads of a window row are contiguous along w.
static __global__ void __launch_bounds__(256) stitch_kernel(const float* __restrict__ win, float* __restrict__ out, uint16_t* __restrict__ count, StitchArgs a) {
  const int w = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y, d = a.d0 + blockIdx.z;
  if (w >= a.W) return;
  int dl, dh_, hl, hh, wl, wh;
  cover(a.sd, a.nd, a.rd, d, dl, dh_);
  cover(a.sh, a.nh, a.rh, h, hl, hh);
  cover(a.sw, a.nw, a.rw, w, wl, wh);
  const int n = (dh_ - dl + 1) * (hh - hl + 1) * (wh - wl + 1);
  const int64_t rvol = (int64_t)a.rd * a.rh * a.rw, vox = (int64_t)a.D * a.H * a.W;
  const int64_t o = ((int64_t)d * a.H + h) * a.W + w;
  if (count) count[o] = (uint16_t)n;
  for (int c = 0; c < a.C; ++c) {
    float acc = 0.f;
    for (int id = dl; id <= dh_; ++id)
      for (int ih = hl; ih <= hh; ++ih)
        for (int iw = wl; iw <= wh; ++iw) {
          const int64_t wi = ((int64_t)id * a.nh + ih) * a.nw + iw;
          acc += win[(wi * a.C + c) * rvol + ((int64_t)(d - a.sd[id]) * a.rh + (h - a.sh[ih])) * a.rw + (w - a.sw[iw])];
        }
    out[(int64_t)c * vox + o] = acc / (float)n;         // MONAI: output_image / count_map (a true division: bit-identical)
  }
}

// Weighted blend (MONAI mode="gaussian" / roi_weight_map): the same one-pass gather with a dense importance map wmap[rd][rh][rw].
//   out = (0 + fl(m_1 * p_1) + fl(m_2 * p_2) ...) / (0 + m_1 + m_2 ...)   over the covering windows in window-index order
// product and add are rounded SEPARATELY (contraction is switched off below: an FMA would differ from MONAI's `out[win] += map * pred` in the
// last bit).  The weights and the window offsets of a voxel do not depend on the channel: with a cover of <= STITCH_COVER_REGS windows (8 at
// overlap 0.5) they are read / computed once per voxel into registers (statically indexed: no scratch) and every channel only streams its
// window values, 8 independent loads in flight per lane; a larger cover (up to 64 at overlap 0.75) re-reads the map, which lives in L2 (96^3 fp32 = 3.5 MB), per channel.
#define STITCH_COVER_REGS 8
static __global__ void __launch_bounds__(256) stitch_weighted_kernel(const float* __restrict__ win, const float* __restrict__ wmap, float* __restrict__ out,
                                                                     uint16_t* __restrict__ count, float* __restrict__ wsum, StitchArgs a) {
#pragma clang fp contract(off)
  const int w = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y, d = a.d0 + blockIdx.z;
  if (w >= a.W) return;
  int dl, dh_, hl, hh, wl, wh;
  cover(a.sd, a.nd, a.rd, d, dl, dh_);
  cover(a.sh, a.nh, a.rh, h, hl, hh);
  cover(a.sw, a.nw, a.rw, w, wl, wh);
  const int n = (dh_ - dl + 1) * (hh - hl + 1) * (wh - wl + 1);
  const int64_t rvol = (int64_t)a.rd * a.rh * a.rw, vox = (int64_t)a.D * a.H * a.W;
  const int64_t o = ((int64_t)d * a.H + h) * a.W + w;
  if (count) count[o] = (uint16_t)n;
  if (n <= STITCH_COVER_REGS) {
    float m[STITCH_COVER_REGS];
    int64_t off[STITCH_COVER_REGS];
    int id = dl, ih = hl, iw = wl;
    float ws = 0.f;
#pragma unroll
    for (int k = 0; k < STITCH_COVER_REGS; ++k) {
      m[k] = 0.f; off[k] = 0;
      if (k < n) {
        const int rel = ((d - a.sd[id]) * a.rh + (h - a.sh[ih])) * a.rw + (w - a.sw[iw]);
        m[k] = wmap[rel];
        off[k] = (((int64_t)id * a.nh + ih) * a.nw + iw) * a.C * rvol + rel;
        ws = ws + m[k];
        if (++iw > wh) { iw = wl; if (++ih > hh) { ih = hl; ++id; } }       // the next window in index order
      }
    }
    if (wsum) wsum[o] = ws;
    for (int c = 0; c < a.C; ++c) {
      const float* __restrict__ src = win + (int64_t)c * rvol;
      // all loads of a channel are issued before the first add (a load under `k < n` waits for the one before it: the gather is latency
      // bound); a slot beyond the cover reads window 0's first voxel (off = 0: a valid address) and its value is dropped by the select
      float v[STITCH_COVER_REGS];
#pragma unroll
      for (int k = 0; k < STITCH_COVER_REGS; ++k) v[k] = src[off[k]];
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < STITCH_COVER_REGS; ++k) {
        const float t = m[k] * v[k];
        const float sum = acc + t;
        acc = k < n ? sum : acc;
      }
      out[(int64_t)c * vox + o] = acc / ws;
    }
    return;
  }
  float ws = 0.f;
  for (int id = dl; id <= dh_; ++id)
    for (int ih = hl; ih <= hh; ++ih)
      for (int iw = wl; iw <= wh; ++iw)
        ws = ws + wmap[((d - a.sd[id]) * a.rh + (h - a.sh[ih])) * a.rw + (w - a.sw[iw])];
  if (wsum) wsum[o] = ws;
  for (int c = 0; c < a.C; ++c) {
    float acc = 0.f;
    for (int id = dl; id <= dh_; ++id)
      for (int ih = hl; ih <= hh; ++ih)
        for (int iw = wl; iw <= wh; ++iw) {
          const int64_t wi = ((int64_t)id * a.nh + ih) * a.nw + iw;
          const int rel = ((d - a.sd[id]) * a.rh + (h - a.sh[ih])) * a.rw + (w - a.sw[iw]);
          const float t = wmap[rel] * win[(wi * a.C + c) * rvol + rel];
          acc = acc + t;
        }
    out[(int64_t)c * vox + o] = acc / ws;
  }
}

// ------------------------------------------------------------------------------------------------ augmentation
struct AugArgs {
  int C, D, H, W, rd, rh, rw, n, lb;
  miseg_aug_sample s[MISEG_AUG_MAX_SAMPLES];
};

// (aug_source - patch coordinate -> coordinate inside the un-augmented crop - lives in common.h: augment.hip gathers through it too)
template <class LB>
__global__ void __launch_bounds__(256) augment_kernel(const float* __restrict__ image, const LB* __restrict__ label, float* __restrict__ oimg, LB* __restrict__ olab, AugArgs a) {
  const int n = blockIdx.z;
  const miseg_aug_sample& sm = a.s[n];
  const int64_t pvol = (int64_t)a.rd * a.rh * a.rw, vvol = (int64_t)a.D * a.H * a.W;
  const float mul = 1.f + sm.scale;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < pvol; o += (int64_t)gridDim.x * 256) {
    const int k = (int)(o % a.rw), j = (int)((o / a.rw) % a.rh), i = (int)(o / ((int64_t)a.rw * a.rh));
    int si, sj, sk;
    aug_source(sm, a.rd, a.rh, a.rw, i, j, k, si, sj, sk);
    const int64_t src = ((int64_t)(sm.origin[0] + si) * a.H + (sm.origin[1] + sj)) * a.W + (sm.origin[2] + sk);
    for (int c = 0; c < a.C; ++c) oimg[((int64_t)n * a.C + c) * pvol + o] = image[(int64_t)c * vvol + src] * mul + sm.shift;
    if (label) olab[(int64_t)n * pvol + o] = label[src];
  }
}

// ------------------------------------------------------------------------------------------------ dropout / drop-path
// (mix64 and the key / group-hash helpers live in common.h: the attention kernels draw the same masks)

// one 64-bit hash per group of 4 consecutive channels: four 16-bit draws against a 16-bit threshold (p is quantised to 1 / 65536)
template <class T>
__global__ void __launch_bounds__(256) dropout_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy, int64_t rows, int C, int64_t rps,
                                                      unsigned thresh, float scale, uint64_t key, const uint64_t* __restrict__ step_dev) {
  const uint64_t k = dropout_step_key(key, step_dev);
  const int cg = (C + 3) / 4;
  const int64_t total = rows * cg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cg;
    const int c0 = (int)(i - r * cg) * 4;
    const uint64_t h = rps > 0 ? mix64(k + (uint64_t)(r / rps) * 0xD1342543DE82EF95ull) : mix64(k + (uint64_t)i * 0xD1342543DE82EF95ull);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c0 + e < C) {
        const unsigned draw = rps > 0 ? (unsigned)(h & 0xffff) : (unsigned)((h >> (16 * e)) & 0xffff);
        const float v = to_f32(x[r * ldx + c0 + e]);
        y[r * ldy + c0 + e] = from_f32<T>(draw >= thresh ? v * scale : 0.f);
      }
    }
  }
}

static __global__ void counter_add_kernel(uint64_t* c, uint64_t v) { *c += v; }
static __global__ void counter_copy_kernel(uint64_t* d, const uint64_t* s) { *d = *s; }

// ------------------------------------------------------------------------------------------------ resampling
struct ResampleArgs { int C, Di, Hi, Wi, Do, Ho, Wo; };

__device__ __forceinline__ float rs_src(int dst, int in, int out) { return ((float)dst + 0.5f) * ((float)in / (float)out) - 0.5f; }

static __global__ void __launch_bounds__(256) resample_linear_kernel(const float* __restrict__ in, float* __restrict__ out, ResampleArgs a) {
  const int64_t ovol = (int64_t)a.Do * a.Ho * a.Wo, ivol = (int64_t)a.Di * a.Hi * a.Wi;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < ovol; o += (int64_t)gridDim.x * 256) {
    const int w = (int)(o % a.Wo), h = (int)((o / a.Wo) % a.Ho), d = (int)(o / ((int64_t)a.Wo * a.Ho));
    const float fd = fminf(fmaxf(rs_src(d, a.Di, a.Do), 0.f), (float)(a.Di - 1));
    const float fh = fminf(fmaxf(rs_src(h, a.Hi, a.Ho), 0.f), (float)(a.Hi - 1));
    const float fw = fminf(fmaxf(rs_src(w, a.Wi, a.Wo), 0.f), (float)(a.Wi - 1));
    const int d0 = (int)fd, h0 = (int)fh, w0 = (int)fw;
    const int d1 = min(d0 + 1, a.Di - 1), h1 = min(h0 + 1, a.Hi - 1), w1 = min(w0 + 1, a.Wi - 1);
    const float td = fd - d0, th = fh - h0, tw = fw - w0;
    for (int c = 0; c < a.C; ++c) {
      const float* p = in + (int64_t)c * ivol;
      auto at = [&](int z, int y, int x) { return p[((int64_t)z * a.Hi + y) * a.Wi + x]; };
      const float c00 = at(d0, h0, w0) * (1.f - tw) + at(d0, h0, w1) * tw, c01 = at(d0, h1, w0) * (1.f - tw) + at(d0, h1, w1) * tw;
      const float c10 = at(d1, h0, w0) * (1.f - tw) + at(d1, h0, w1) * tw, c11 = at(d1, h1, w0) * (1.f - tw) + at(d1, h1, w1) * tw;
      out[(int64_t)c * ovol + o] = (c00 * (1.f - th) + c01 * th) * (1.f - td) + (c10 * (1.f - th) + c11 * th) * td;
    }
  }
}

template <class E>
__global__ void __launch_bounds__(256) resample_nearest_kernel(const E* __restrict__ in, E* __restrict__ out, ResampleArgs a) {
  const int64_t ovol = (int64_t)a.Do * a.Ho * a.Wo, ivol = (int64_t)a.Di * a.Hi * a.Wi;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < ovol; o += (int64_t)gridDim.x * 256) {
    const int w = (int)(o % a.Wo), h = (int)((o / a.Wo) % a.Ho), d = (int)(o / ((int64_t)a.Wo * a.Ho));
    const int sd = min(max((int)floorf(rs_src(d, a.Di, a.Do) + 0.5f), 0), a.Di - 1);
    const int sh = min(max((int)floorf(rs_src(h, a.Hi, a.Ho) + 0.5f), 0), a.Hi - 1);
    const int sw = min(max((int)floorf(rs_src(w, a.Wi, a.Wo) + 0.5f), 0), a.Wi - 1);
    for (int c = 0; c < a.C; ++c) out[(int64_t)c * ovol + o] = in[(int64_t)c * ivol + ((int64_t)sd * a.Hi + sh) * a.Wi + sw];
  }
}

// ------------------------------------------------------------------------------------------------ prediction export
// Pass 1: first-maximum argmax of the logits box into a uint8 class map [bd][bh][bw] (lanes along w: every channel row is read coalesced).
static __global__ void __launch_bounds__(256) export_argmax_kernel(const float* __restrict__ logits, uint8_t* __restrict__ cls, int C, int H, int W,
                                                                   int64_t vox, int d0, int h0, int w0, int bh, int bw, int nbox) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < nbox; e += gridDim.x * 256) {
    const int w = e % bw, h = (e / bw) % bh, d = e / (bw * bh);
    const float* x = logits + ((int64_t)(d0 + d) * H + (h0 + h)) * W + (w0 + w);
    int arg = 0;
    float mx = x[0];
    for (int c = 1; c < C; ++c) {
      const float v = x[(int64_t)c * vox];
      if (v > mx) { mx = v; arg = c; }            // strict: the FIRST maximum wins; a NaN after channel 0 never does
    }
    cls[e] = (uint8_t)arg;
  }
}

// Pass 2: one workgroup = a 64 (X) x 64 (axis f) output tile at one coordinate of axis g.  The class-map bytes under the tile are read with the
// lanes along whichever of X / f indexes the map's fast axis, staged in LDS, then written out with the lanes along X (whole 128-B lines of
// uint16), through the LUT.  M: the class map's element - the argmax pass's uint8 map of the box, or a caller's uint8 / int32 map of the whole volume,
// whose values outside [0, C) take the LUT's extra entry 64 (= 0).
constexpr int EXPORT_TILE = 64, EXPORT_LD = EXPORT_TILE + 1;
struct ExportArgs {
  const int32_t* tab[3];           // output axis X, Y, Z -> table
  int n[3], lo[3], bn[3], st[3];   // per output axis: size, box origin / extent of its logits axis, class-map stride
  int f, g, fast_x, C;
};

template <class M, class O>
__global__ void __launch_bounds__(256) export_gather_kernel(const M* __restrict__ cls, const int32_t* __restrict__ lut, O* __restrict__ out, ExportArgs a) {
  __shared__ int offs[2][EXPORT_TILE];
  __shared__ uint8_t tile[EXPORT_TILE * EXPORT_LD];         // [j along f][i along X]
  __shared__ O lut_s[65];
  const int tid = threadIdx.x, x0 = blockIdx.x * EXPORT_TILE, j0 = blockIdx.y * EXPORT_TILE, cg = blockIdx.z;
  const int nx = a.n[0], nf = a.n[a.f];
  if (tid < 2 * EXPORT_TILE) {
    const int ax = tid < EXPORT_TILE ? 0 : a.f, i = tid & (EXPORT_TILE - 1), c = (ax == 0 ? x0 : j0) + i;
    offs[tid >> 6][i] = c < a.n[ax] ? min(max(a.tab[ax][c] - a.lo[ax], 0), a.bn[ax] - 1) * a.st[ax] : 0;
  } else if (tid < 2 * EXPORT_TILE + a.C) lut_s[tid - 2 * EXPORT_TILE] = (O)lut[tid - 2 * EXPORT_TILE];
  else if (tid == 255) lut_s[64] = (O)0;
  __syncthreads();
  const int og = min(max(a.tab[a.g][cg] - a.lo[a.g], 0), a.bn[a.g] - 1) * a.st[a.g];
#pragma unroll 4
  for (int k = 0; k < EXPORT_TILE * EXPORT_TILE / 256; ++k) {
    const int e = tid + 256 * k;
    const int i = a.fast_x ? (e & 63) : (e >> 6), j = a.fast_x ? (e >> 6) : (e & 63);
    if (x0 + i < nx && j0 + j < nf) {
      const uint32_t c = (uint32_t)cls[(int64_t)offs[0][i] + offs[1][j] + og];
      tile[j * EXPORT_LD + i] = c < (uint32_t)a.C ? (uint8_t)c : (uint8_t)64;
    }
  }
  __syncthreads();
  const int64_t ost[3] = {1, (int64_t)nx, (int64_t)nx * a.n[1]};
  O* ob = out + x0 + (int64_t)j0 * ost[a.f] + (int64_t)cg * ost[a.g];
#pragma unroll 4
  for (int k = 0; k < EXPORT_TILE * EXPORT_TILE / 256; ++k) {
    const int e = tid + 256 * k, i = e & 63, j = e >> 6;
    if (x0 + i < nx && j0 + j < nf) ob[i + (int64_t)j * ost[a.f]] = lut_s[tile[j * EXPORT_LD + i]];
  }
}

template <class F> static int dispatch_label(int dt, F&& f) {
  switch (dt) {
    case MISEG_LABEL_F32: return f((const float*)nullptr);
    case MISEG_LABEL_I32: return f((const int32_t*)nullptr);
    case MISEG_LABEL_I64: return f((const int64_t*)nullptr);
    case MISEG_LABEL_U8: return f((const uint8_t*)nullptr);
  }
  return set_error(MISEG_E_BADARG, "unknown label dtype %d", dt);
}

static int loss_check(const miseg_seg_loss_params* p, const char* what) {
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_seg_loss_params), MISEG_E_BADARG, "%s: struct_size %u != %zu (header / binding drift)", what,
                p ? p->struct_size : 0u, sizeof(miseg_seg_loss_params));
  MISEG_REQUIRE(p->logits && p->label && p->sums && p->workspace, MISEG_E_BADARG, "%s: null pointer", what);
  MISEG_REQUIRE(p->B > 0 && p->B <= 64 && p->C >= 2 && p->C <= LOSS_MAXC && p->S > 0, MISEG_E_UNSUPPORTED, "%s: B %d (<= 64), C %d (2..%d)", what, p->B, p->C, LOSS_MAXC);
  MISEG_REQUIRE(p->kind == MISEG_LOSS_DICE_FOCAL || p->kind == MISEG_LOSS_DICE_CE || p->kind == MISEG_LOSS_GDICE_FOCAL, MISEG_E_BADARG, "%s: kind %d", what, p->kind);
  MISEG_REQUIRE(p->kind != MISEG_LOSS_GDICE_FOCAL || (p->weight_type >= MISEG_GDICE_W_SQUARE && p->weight_type <= MISEG_GDICE_W_UNIFORM), MISEG_E_BADARG,
                "%s: weight_type %d", what, p->weight_type);
  return MISEG_OK;
}

static LossGeom loss_geom(const miseg_seg_loss_params* p) {
  LossGeom g;
  g.B = p->B; g.C = p->C; g.kind = p->kind; g.c0 = p->include_background ? 0 : 1; g.sq = p->squared_pred ? 1 : 0; g.S = p->S; g.gamma = p->gamma;
  g.wt = p->weight_type;
  if (p->kind == MISEG_LOSS_GDICE_FOCAL) g.sq = 0;      // the generalized Dice never squares the prediction
  return g;
}

}  // namespace miseg

using namespace miseg;

extern "C" size_t miseg_seg_loss_workspace_bytes(int B, int C, int64_t S) {
  return (size_t)B * (size_t)cdiv(S, LOSS_VPB) * (3 * C + 1) * sizeof(double);
}

extern "C" int miseg_seg_loss_fwd(const miseg_seg_loss_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  if (int rc = loss_check(p, "seg_loss_fwd")) return rc;
  MISEG_REQUIRE(p->loss, MISEG_E_BADARG, "seg_loss_fwd: null loss pointer");
  const LossGeom g = loss_geom(p);
  const int nblk = cdiv(p->S, LOSS_VPB);
  const bool vec = p->S % 4 == 0 && ((uintptr_t)p->logits & 15) == 0;
  return dispatch_label(p->label_dtype, [&](auto* tag) -> int {
    typedef typename std::remove_const<typename std::remove_pointer<decltype(tag)>::type>::type L;
    dim3 grid(nblk, p->B);
    if (p->C <= 8) {
      if (vec) seg_loss_fwd_kernel<L, 8, LOSS_VEC><<<grid, 256, 0, s>>>(p->logits, (const L*)p->label, g, (double*)p->workspace);
      else seg_loss_fwd_kernel<L, 8, 1><<<grid, 256, 0, s>>>(p->logits, (const L*)p->label, g, (double*)p->workspace);
    } else {
      seg_loss_fwd_kernel<L, LOSS_MAXC, 1><<<grid, 256, 0, s>>>(p->logits, (const L*)p->label, g, (double*)p->workspace);
    }
    MISEG_LAUNCH_CHECK("seg_loss_fwd");
    seg_loss_finalize_kernel<<<1, 1024, 0, s>>>((const double*)p->workspace, nblk, g, p->smooth_nr, p->smooth_dr, p->lambda_dice, p->lambda_other, p->sums, p->loss);
    MISEG_LAUNCH_CHECK("seg_loss_finalize");
    return MISEG_OK;
  });
}

extern "C" int miseg_seg_loss_bwd(const miseg_seg_loss_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  if (int rc = loss_check(p, "seg_loss_bwd")) return rc;
  MISEG_REQUIRE(p->dlogits, MISEG_E_BADARG, "seg_loss_bwd: null dlogits pointer");
  const LossGeom g = loss_geom(p);
  const int nblk = cdiv(p->S, LOSS_VPB);
  const bool vec = p->S % 4 == 0 && ((uintptr_t)p->logits & 15) == 0 && ((uintptr_t)p->dlogits & 15) == 0;
  return dispatch_label(p->label_dtype, [&](auto* tag) -> int {
    typedef typename std::remove_const<typename std::remove_pointer<decltype(tag)>::type>::type L;
    dim3 grid(nblk, p->B);
#define MISEG_LB(MAXC, VEC, GD) seg_loss_bwd_kernel<L, MAXC, VEC, GD><<<grid, 256, 0, s>>>(p->logits, (const L*)p->label, g, p->smooth_nr, p->smooth_dr, p->lambda_dice, \
                                                                                            p->lambda_other, p->sums, p->gscale, p->dlogits)
    if (p->kind == MISEG_LOSS_GDICE_FOCAL) {
      if (p->C <= 8) {
        if (vec) MISEG_LB(8, LOSS_VEC, true); else MISEG_LB(8, 1, true);
      } else MISEG_LB(LOSS_MAXC, 1, true);
    } else if (p->C <= 8) {
      if (vec) MISEG_LB(8, LOSS_VEC, false); else MISEG_LB(8, 1, false);
    } else MISEG_LB(LOSS_MAXC, 1, false);
#undef MISEG_LB
    MISEG_LAUNCH_CHECK("seg_loss_bwd");
    return MISEG_OK;
  });
}

extern "C" int miseg_dice_metric(const miseg_dice_metric_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_dice_metric_params), MISEG_E_BADARG, "dice_metric: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_dice_metric_params));
  MISEG_REQUIRE(p->logits && p->label && p->counts && p->dice, MISEG_E_BADARG, "dice_metric: null pointer");
  MISEG_REQUIRE(p->B > 0 && p->C >= 1 && p->C <= 64 && p->S > 0, MISEG_E_UNSUPPORTED, "dice_metric: C %d (1..64)", p->C);
  MISEG_REQUIRE(!p->gdice || (p->weight_type >= MISEG_GDICE_W_SQUARE && p->weight_type <= MISEG_GDICE_W_UNIFORM), MISEG_E_BADARG, "dice_metric: weight_type %d",
                p->weight_type);
  if (fill_words_async(p->counts, 0, (size_t)p->B * p->C * 3 * 2, s) != hipSuccess) return set_error(MISEG_E_LAUNCH, "dice_metric: fill");
  return dispatch_label(p->label_dtype, [&](auto* tag) -> int {
    typedef typename std::remove_const<typename std::remove_pointer<decltype(tag)>::type>::type L;
    int gx = cdiv(p->S, 256 * 8);
    if (gx > 2048) gx = 2048;
    dice_count_kernel<L, 64><<<dim3(gx, p->B), 256, 0, s>>>(p->logits, (const L*)p->label, p->C, p->S, (unsigned long long*)p->counts);
    MISEG_LAUNCH_CHECK("dice_count");
    dice_finalize_kernel<<<cdiv(p->B * p->C, 64), 64, 0, s>>>((const unsigned long long*)p->counts, p->B * p->C, p->dice, p->C,
                                                              p->include_background || p->C == 1 ? 0 : 1, p->weight_type, p->gdice);
    MISEG_LAUNCH_CHECK("dice_finalize");
    return MISEG_OK;
  });
}

// miseg_opt_step (clipped == false: rec / mode / clip_value unused) and miseg_opt_step_clipped
static int opt_step_launch(const miseg_opt_step_params* p, bool clipped, const miseg_grad_clip_record* rec, int mode, float clip_value, hipStream_t s) {
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_opt_step_params), MISEG_E_BADARG, "opt_step: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_opt_step_params));
  MISEG_REQUIRE(p->descs_dev && p->grad && p->state1 && p->steps && p->ndesc > 0 && p->total_blocks > 0, MISEG_E_BADARG, "opt_step: null pointer / empty table");
  MISEG_REQUIRE(p->kind == MISEG_OPT_ADAMW || p->kind == MISEG_OPT_ADAM || p->kind == MISEG_OPT_SGD_NESTEROV, MISEG_E_BADARG, "opt_step: kind %d", p->kind);
  MISEG_REQUIRE(p->kind == MISEG_OPT_SGD_NESTEROV || p->state2, MISEG_E_BADARG, "opt_step: Adam needs state2");
  MISEG_REQUIRE(p->index || p->count_n < 0 || p->count_n == p->ndesc, MISEG_E_BADARG, "opt_step: count_n %d without an index table", p->count_n);
  float* s2 = p->kind == MISEG_OPT_SGD_NESTEROV ? nullptr : p->state2;
  if (clipped)
    opt_step_kernel<true><<<p->total_blocks, 256, 0, s>>>(p->descs_dev, p->ndesc, p->kind, p->grad, p->state1, s2, p->used, p->steps, p->lr, p->beta1, p->beta2, p->eps,
                                                         p->weight_decay, p->momentum, p->lr_dev, p->index, rec, mode, clip_value);
  else
    opt_step_kernel<false><<<p->total_blocks, 256, 0, s>>>(p->descs_dev, p->ndesc, p->kind, p->grad, p->state1, s2, p->used, p->steps, p->lr, p->beta1, p->beta2, p->eps,
                                                          p->weight_decay, p->momentum, p->lr_dev, p->index, nullptr, MISEG_CLIP_NONE, 0.f);
  MISEG_LAUNCH_CHECK("opt_step");
  const int cn = p->count_n < 0 ? p->ndesc : p->count_n;
  if (cn > 0) {
    const int rc = opt_count_launch(p->used, p->steps, cn, p->params_version, nullptr, s, clipped ? rec : nullptr);
    if (rc != MISEG_OK) return rc;
  }
  return MISEG_OK;
}

extern "C" int miseg_opt_step(const miseg_opt_step_params* p, miseg_stream_t s_) {
  return opt_step_launch(p, false, nullptr, MISEG_CLIP_NONE, 0.f, (hipStream_t)s_);
}

int miseg::opt_clip_check(const miseg_grad_clip_record* rec, int mode, float clip_value, const char* what) {
  MISEG_REQUIRE(mode == MISEG_CLIP_NONE || mode == MISEG_CLIP_NORM || mode == MISEG_CLIP_VALUE, MISEG_E_BADARG, "%s: clip mode %d", what, mode);
  MISEG_REQUIRE(rec || mode == MISEG_CLIP_VALUE, MISEG_E_BADARG, "%s: clip mode %d needs the record miseg_grad_norm fills", what, mode);
  MISEG_REQUIRE(mode != MISEG_CLIP_VALUE || (isfinite(clip_value) && clip_value > 0.f), MISEG_E_BADARG, "%s: clip_value %g must be finite and > 0", what,
                (double)clip_value);
  return MISEG_OK;
}

extern "C" int miseg_opt_step_clipped(const miseg_opt_step_params* p, const miseg_grad_clip_record* rec, int mode, float clip_value, miseg_stream_t s_) {
  const int rc = opt_clip_check(rec, mode, clip_value, "opt_step_clipped");
  if (rc != MISEG_OK) return rc;
  return opt_step_launch(p, true, rec, mode, clip_value, (hipStream_t)s_);
}

int miseg::opt_count_launch(const int32_t* used, int32_t* steps, int n, int64_t* params_version, int64_t* pack_state, hipStream_t s,
                            const miseg_grad_clip_record* rec) {
  opt_count_kernel<<<cdiv(n, 256), 256, 0, s>>>(used, steps, n, params_version, pack_state, rec);
  MISEG_LAUNCH_CHECK("opt_count");
  return MISEG_OK;
}

extern "C" size_t miseg_grad_norm_workspace_bytes(int total_blocks, int ndesc) {
  if (total_blocks <= 0 || ndesc <= 0) return 0;
  return ((size_t)total_blocks + (size_t)ndesc) * sizeof(double);      // the blocks' partials, then the tensors' sums
}

extern "C" int miseg_grad_norm(const miseg_grad_norm_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_grad_norm_params), MISEG_E_BADARG, "grad_norm: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_grad_norm_params));
  MISEG_REQUIRE(p->descs_dev && p->grad && p->workspace && p->record && p->ndesc > 0 && p->total_blocks > 0, MISEG_E_BADARG, "grad_norm: null pointer / empty table");
  MISEG_REQUIRE((((uintptr_t)p->workspace) & 7) == 0, MISEG_E_BADARG, "grad_norm: the workspace must be 8-byte aligned");
  MISEG_REQUIRE(p->mode == MISEG_CLIP_NONE || p->mode == MISEG_CLIP_NORM || p->mode == MISEG_CLIP_VALUE, MISEG_E_BADARG, "grad_norm: clip mode %d", p->mode);
  MISEG_REQUIRE(p->mode != MISEG_CLIP_NORM || (isfinite(p->max_norm) && p->max_norm > 0.f), MISEG_E_BADARG, "grad_norm: max_norm %g must be finite and > 0",
                (double)p->max_norm);
  double* part = (double*)p->workspace;
  grad_sqsum_kernel<<<p->total_blocks, 256, 0, s>>>(p->descs_dev, p->ndesc, p->grad, p->used, part);
  MISEG_LAUNCH_CHECK("grad_sqsum");
  grad_norm_finish_kernel<<<1, GN_THREADS, 0, s>>>(p->descs_dev, p->ndesc, p->total_blocks, part, part + p->total_blocks, p->mode, p->max_norm,
                                                  p->skip_nonfinite ? 1 : 0, p->record, p->per_param);
  MISEG_LAUNCH_CHECK("grad_norm_finish");
  return MISEG_OK;
}

extern "C" int miseg_grad_fold(const miseg_grad_fold_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_grad_fold_params), MISEG_E_BADARG, "grad_fold: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_grad_fold_params));
  MISEG_REQUIRE(p->descs_dev && p->grad && p->acc && p->ops && p->ndesc > 0 && p->total_blocks > 0 && p->arena_elems > 0, MISEG_E_BADARG,
                "grad_fold: null pointer / empty table");
  MISEG_REQUIRE(isfinite(p->scale) && p->scale > 0.f, MISEG_E_BADARG, "grad_fold: scale %g must be finite and > 0", (double)p->scale);
  const uintptr_t g0 = (uintptr_t)p->grad, a0 = (uintptr_t)p->acc, bytes = (uintptr_t)p->arena_elems * sizeof(float);
  MISEG_REQUIRE((g0 & 15) == 0 && (a0 & 15) == 0 && (((uintptr_t)p->ops) & 3) == 0, MISEG_E_BADARG,
                "grad_fold: grad and acc must be 16-byte aligned (ops: 4-byte)");
  MISEG_REQUIRE(g0 + bytes <= a0 || a0 + bytes <= g0, MISEG_E_BADARG, "grad_fold: grad and acc overlap");
  grad_fold_kernel<<<p->total_blocks, 256, 0, s>>>(p->descs_dev, p->ndesc, p->grad, p->acc, p->ops, p->scale);
  MISEG_LAUNCH_CHECK("grad_fold");
  return MISEG_OK;
}

extern "C" int miseg_weight_average(const miseg_weight_average_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_weight_average_params), MISEG_E_BADARG, "weight_average: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_weight_average_params));
  MISEG_REQUIRE(p->descs_dev && p->avg && p->record, MISEG_E_BADARG, "weight_average: null pointer (descs_dev / avg / record)");
  MISEG_REQUIRE(p->ndesc > 0 && p->total_blocks > 0, MISEG_E_BADARG, "weight_average: empty table (ndesc %d, total_blocks %d)", p->ndesc, p->total_blocks);
  MISEG_REQUIRE(p->mode == MISEG_AVG_EMA || p->mode == MISEG_AVG_MEAN, MISEG_E_BADARG, "weight_average: mode %d", p->mode);
  MISEG_REQUIRE(isfinite(p->decay) && p->decay >= 0.f && p->decay < 1.f, MISEG_E_BADARG, "weight_average: decay %g must be finite and in [0, 1)", (double)p->decay);
  MISEG_REQUIRE(p->every >= 1, MISEG_E_BADARG, "weight_average: every %d must be >= 1", p->every);
  MISEG_REQUIRE(p->start >= 0, MISEG_E_BADARG, "weight_average: start %d must be >= 0", p->start);
  MISEG_REQUIRE((((uintptr_t)p->avg) & 15) == 0 && (((uintptr_t)p->record) & 3) == 0, MISEG_E_BADARG,
                "weight_average: avg must be 16-byte aligned (record: 4-byte)");
  weight_average_tick_kernel<<<1, 1, 0, s>>>(p->record, p->clip_record, p->mode, p->decay, p->warmup ? 1 : 0, p->start, p->every);
  MISEG_LAUNCH_CHECK("weight_average_tick");
  weight_average_kernel<<<p->total_blocks, 256, 0, s>>>(p->descs_dev, p->ndesc, p->avg, p->record, p->clip_record);
  MISEG_LAUNCH_CHECK("weight_average");
  return MISEG_OK;
}

extern "C" int miseg_weight_swap(const miseg_weight_swap_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_weight_swap_params), MISEG_E_BADARG, "weight_swap: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_weight_swap_params));
  MISEG_REQUIRE(p->descs_dev && p->avg, MISEG_E_BADARG, "weight_swap: null pointer (descs_dev / avg)");
  MISEG_REQUIRE(p->ndesc > 0 && p->total_blocks > 0, MISEG_E_BADARG, "weight_swap: empty table (ndesc %d, total_blocks %d)", p->ndesc, p->total_blocks);
  MISEG_REQUIRE((((uintptr_t)p->avg) & 15) == 0, MISEG_E_BADARG, "weight_swap: avg must be 16-byte aligned");
  weight_swap_kernel<<<p->total_blocks, 256, 0, s>>>(p->descs_dev, p->ndesc, p->avg, p->params_version);
  MISEG_LAUNCH_CHECK("weight_swap");
  return MISEG_OK;
}

extern "C" int miseg_stitch_windows(const miseg_stitch_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_stitch_params), MISEG_E_BADARG, "stitch_windows: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_stitch_params));
  MISEG_REQUIRE(p->win && p->out && p->start_d && p->start_h && p->start_w, MISEG_E_BADARG, "stitch_windows: null pointer");
  MISEG_REQUIRE(p->nd > 0 && p->nh > 0 && p->nw > 0 && p->nd <= MISEG_STITCH_MAX_WINDOWS && p->nh <= MISEG_STITCH_MAX_WINDOWS && p->nw <= MISEG_STITCH_MAX_WINDOWS,
                MISEG_E_UNSUPPORTED, "stitch_windows: %d x %d x %d windows (max %d per axis)", p->nd, p->nh, p->nw, MISEG_STITCH_MAX_WINDOWS);
  MISEG_REQUIRE(p->C > 0 && p->D > 0 && p->H > 0 && p->W > 0 && p->H <= 65535 && p->D <= 65535, MISEG_E_BADARG, "stitch_windows: bad volume");
  MISEG_REQUIRE(p->rd > 0 && p->rh > 0 && p->rw > 0 && (int64_t)p->rd * p->rh * p->rw <= INT32_MAX, MISEG_E_BADARG, "stitch_windows: bad roi %d x %d x %d", p->rd,
                p->rh, p->rw);
  MISEG_REQUIRE(p->weight || !p->wsum, MISEG_E_BADARG, "stitch_windows: wsum is the weighted count: it needs a weight map");
  StitchArgs a;
  a.C = p->C; a.D = p->D; a.H = p->H; a.W = p->W; a.rd = p->rd; a.rh = p->rh; a.rw = p->rw; a.nd = p->nd; a.nh = p->nh; a.nw = p->nw;
  const int* src[3] = {p->start_d, p->start_h, p->start_w};
  int* dst[3] = {a.sd, a.sh, a.sw};
  const int n[3] = {p->nd, p->nh, p->nw}, r[3] = {p->rd, p->rh, p->rw}, size[3] = {p->D, p->H, p->W};
  const bool slab = p->d_count > 0;
  MISEG_REQUIRE(p->d_count >= 0 && (!slab || (p->d_begin >= 0 && p->d_begin + p->d_count <= p->D)), MISEG_E_BADARG, "stitch_windows: slab [%d, %d + %d) of depth %d",
                p->d_begin, p->d_begin, p->d_count, p->D);
  a.d0 = slab ? p->d_begin : 0;
  for (int ax = 0; ax < 3; ++ax) {
    for (int i = 0; i < MISEG_STITCH_MAX_WINDOWS; ++i) dst[ax][i] = i < n[ax] ? src[ax][i] : 0;
    // every coordinate must be covered, windows inside the volume, starts non-decreasing: checked here, on the host, before any launch
    int reach = 0;
    for (int i = 0; i < n[ax]; ++i) {
      if (ax == 0 && slab && i == 0) {      // resident layers of a slab: the first one only has to reach back to the slab's first depth
        MISEG_REQUIRE(src[0][0] >= 0 && src[0][0] <= p->d_begin, MISEG_E_BADARG, "stitch_windows: the first resident layer starts at %d, behind the slab's first depth %d",
                      src[0][0], p->d_begin);
        reach = src[0][0];
      }
      MISEG_REQUIRE(src[ax][i] >= 0 && src[ax][i] + r[ax] <= size[ax] && (i == 0 || src[ax][i] >= src[ax][i - 1]) && src[ax][i] <= reach, MISEG_E_BADARG,
                    "stitch_windows: axis %d window %d start %d (roi %d, size %d) leaves a gap or leaves the volume", ax, i, src[ax][i], r[ax], size[ax]);
      reach = src[ax][i] + r[ax];
    }
    if (ax == 0 && slab) {
      MISEG_REQUIRE(reach >= p->d_begin + p->d_count, MISEG_E_BADARG, "stitch_windows: the resident layers cover depths up to %d, the slab ends at %d", reach,
                    p->d_begin + p->d_count);
      continue;
    }
    MISEG_REQUIRE(reach == size[ax], MISEG_E_BADARG, "stitch_windows: axis %d is covered up to %d of %d", ax, reach, size[ax]);
  }
  const dim3 grid(cdiv(p->W, 256), p->H, slab ? p->d_count : p->D);
  if (p->weight) stitch_weighted_kernel<<<grid, 256, 0, s>>>(p->win, p->weight, p->out, p->count, p->wsum, a);
  else stitch_kernel<<<grid, 256, 0, s>>>(p->win, p->out, p->count, a);
  MISEG_LAUNCH_CHECK("stitch_windows");
  return MISEG_OK;
}

extern "C" int miseg_augment_crop(const miseg_augment_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_augment_params), MISEG_E_BADARG, "augment_crop: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_augment_params));
  MISEG_REQUIRE(p->image && p->out_image && p->samples_host && (!p->label || p->out_label), MISEG_E_BADARG, "augment_crop: null pointer");
  MISEG_REQUIRE(p->n > 0 && p->n <= MISEG_AUG_MAX_SAMPLES && p->C > 0, MISEG_E_UNSUPPORTED, "augment_crop: %d samples (max %d)", p->n, MISEG_AUG_MAX_SAMPLES);
  MISEG_REQUIRE(p->label_bytes == 1 || p->label_bytes == 4 || p->label_bytes == 8 || !p->label, MISEG_E_UNSUPPORTED, "augment_crop: label element of %d bytes", p->label_bytes);
  AugArgs a;
  a.C = p->C; a.D = p->D; a.H = p->H; a.W = p->W; a.rd = p->rd; a.rh = p->rh; a.rw = p->rw; a.n = p->n; a.lb = p->label_bytes;
  for (int i = 0; i < p->n; ++i) {
    const miseg_aug_sample& q = p->samples_host[i];
    // every gathered coordinate stays inside the volume: checked here, on the host, before the launch
    MISEG_REQUIRE(q.origin[0] >= 0 && q.origin[1] >= 0 && q.origin[2] >= 0 && q.origin[0] + p->rd <= p->D && q.origin[1] + p->rh <= p->H && q.origin[2] + p->rw <= p->W,
                  MISEG_E_BADARG, "augment_crop: sample %d crop (%d,%d,%d)+(%d,%d,%d) leaves the %dx%dx%d volume", i, q.origin[0], q.origin[1], q.origin[2], p->rd, p->rh,
                  p->rw, p->D, p->H, p->W);
    MISEG_REQUIRE(!(q.rot_k & 1) || p->rd == p->rh, MISEG_E_BADARG, "augment_crop: an odd number of quarter turns needs roi_d == roi_h");
    a.s[i] = q;
  }
  int gx = cdiv((int64_t)p->rd * p->rh * p->rw, 256 * 4);
  if (gx > 1024) gx = 1024;
  const dim3 grid(gx, 1, p->n);
  if (!p->label || p->label_bytes == 1) augment_kernel<uint8_t><<<grid, 256, 0, s>>>(p->image, (const uint8_t*)p->label, p->out_image, (uint8_t*)p->out_label, a);
  else if (p->label_bytes == 4) augment_kernel<uint32_t><<<grid, 256, 0, s>>>(p->image, (const uint32_t*)p->label, p->out_image, (uint32_t*)p->out_label, a);
  else augment_kernel<uint64_t><<<grid, 256, 0, s>>>(p->image, (const uint64_t*)p->label, p->out_image, (uint64_t*)p->out_label, a);
  MISEG_LAUNCH_CHECK("augment_crop");
  return MISEG_OK;
}

extern "C" int miseg_resample3d(const miseg_resample3d_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_resample3d_params), MISEG_E_BADARG, "resample3d: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_resample3d_params));
  MISEG_REQUIRE(p->in && p->out && p->C > 0 && p->Di > 0 && p->Hi > 0 && p->Wi > 0 && p->Do > 0 && p->Ho > 0 && p->Wo > 0, MISEG_E_BADARG, "resample3d: bad arguments");
  ResampleArgs a{p->C, p->Di, p->Hi, p->Wi, p->Do, p->Ho, p->Wo};
  int grid = cdiv((int64_t)p->Do * p->Ho * p->Wo, 256 * 4);
  if (grid > 4096) grid = 4096;
  if (p->mode == 0) {
    MISEG_REQUIRE(p->elem_bytes == 4, MISEG_E_UNSUPPORTED, "resample3d: trilinear needs fp32");
    resample_linear_kernel<<<grid, 256, 0, s>>>((const float*)p->in, (float*)p->out, a);
  } else if (p->mode == 1) {
    if (p->elem_bytes == 1) resample_nearest_kernel<uint8_t><<<grid, 256, 0, s>>>((const uint8_t*)p->in, (uint8_t*)p->out, a);
    else if (p->elem_bytes == 4) resample_nearest_kernel<uint32_t><<<grid, 256, 0, s>>>((const uint32_t*)p->in, (uint32_t*)p->out, a);
    else if (p->elem_bytes == 8) resample_nearest_kernel<uint64_t><<<grid, 256, 0, s>>>((const uint64_t*)p->in, (uint64_t*)p->out, a);
    else return set_error(MISEG_E_UNSUPPORTED, "resample3d: element of %d bytes", p->elem_bytes);
  } else return set_error(MISEG_E_BADARG, "resample3d: mode %d", p->mode);
  MISEG_LAUNCH_CHECK("resample3d");
  return MISEG_OK;
}

extern "C" size_t miseg_label_export_workspace_bytes(int box_nd, int box_nh, int box_nw) {
  if (box_nd <= 0 || box_nh <= 0 || box_nw <= 0) return 0;
  return (((size_t)box_nd * box_nh * box_nw) + 255) & ~(size_t)255;
}

extern "C" int miseg_label_export(const miseg_label_export_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_label_export_params), MISEG_E_BADARG, "label_export: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_label_export_params));
  MISEG_REQUIRE((p->logits != nullptr) != (p->cls != nullptr), MISEG_E_BADARG, "label_export: exactly one of logits / cls");
  MISEG_REQUIRE(p->table_x && p->table_y && p->table_z && p->lut && (p->workspace || p->cls) && p->out, MISEG_E_BADARG, "label_export: null pointer");
  MISEG_REQUIRE(!p->cls || p->cls_bytes == 1 || p->cls_bytes == 4, MISEG_E_BADARG, "label_export: cls_bytes %d (1 or 4)", p->cls_bytes);
  MISEG_REQUIRE(p->C >= 1 && p->C <= 64, MISEG_E_BADARG, "label_export: C %d (1..64)", p->C);
  MISEG_REQUIRE(p->out_bytes == 1 || p->out_bytes == 2 || p->out_bytes == 4, MISEG_E_BADARG, "label_export: out_bytes %d (1, 2 or 4)", p->out_bytes);
  const int dims[3] = {p->D, p->H, p->W}, lo[3] = {p->box_d0, p->box_h0, p->box_w0}, bn[3] = {p->box_nd, p->box_nh, p->box_nw};
  const int n[3] = {p->nx, p->ny, p->nz}, axis[3] = {p->axis_x, p->axis_y, p->axis_z};
  for (int k = 0; k < 3; ++k) {
    MISEG_REQUIRE(dims[k] > 0 && dims[k] <= 65535 && n[k] > 0 && n[k] <= 65535, MISEG_E_BADARG, "label_export: logits %dx%dx%d, out %dx%dx%d (sides 1..65535)",
                  p->D, p->H, p->W, p->nx, p->ny, p->nz);
    MISEG_REQUIRE(lo[k] >= 0 && bn[k] > 0 && lo[k] + bn[k] <= dims[k], MISEG_E_BADARG, "label_export: box axis %d [%d, %d + %d) leaves the side %d", k, lo[k],
                  lo[k], bn[k], dims[k]);
    MISEG_REQUIRE(axis[k] >= 0 && axis[k] < 3 && axis[k] != axis[(k + 1) % 3] && axis[k] != axis[(k + 2) % 3], MISEG_E_BADARG,
                  "label_export: axes (%d, %d, %d) are not a permutation of (0, 1, 2)", axis[0], axis[1], axis[2]);
  }
  const int64_t nbox = (int64_t)bn[0] * bn[1] * bn[2];
  MISEG_REQUIRE(nbox < ((int64_t)1 << 31), MISEG_E_UNSUPPORTED, "label_export: box of %lld voxels (below 2^31)", (long long)nbox);
  uint8_t* cls = (uint8_t*)p->workspace;
  if (p->logits) {
    int g1 = cdiv(nbox, 256 * 4);
    if (g1 > 8192) g1 = 8192;
    export_argmax_kernel<<<g1, 256, 0, s>>>(p->logits, cls, p->C, p->H, p->W, (int64_t)p->D * p->H * p->W, lo[0], lo[1], lo[2], bn[1], bn[2], (int)nbox);
    MISEG_LAUNCH_CHECK("label_export argmax");
  } else {
    MISEG_REQUIRE((int64_t)p->D * p->H * p->W < ((int64_t)1 << 31), MISEG_E_UNSUPPORTED, "label_export: a class map of %lld voxels (below 2^31)",
                  (long long)p->D * p->H * p->W);
  }
  ExportArgs a;
  // the argmax pass packs the box; a given map is read where it lies: the whole volume's strides, from the box's first voxel
  const int st[3] = {p->logits ? bn[1] * bn[2] : p->H * p->W, p->logits ? bn[2] : p->W, 1};
  const int64_t first = p->logits ? 0 : ((int64_t)lo[0] * p->H + lo[1]) * p->W + lo[2];
  const int32_t* tab[3] = {p->table_x, p->table_y, p->table_z};
  for (int k = 0; k < 3; ++k) { a.tab[k] = tab[k]; a.n[k] = n[k]; a.lo[k] = lo[axis[k]]; a.bn[k] = bn[axis[k]]; a.st[k] = st[axis[k]]; }
  // the tile's second axis: the one that indexes the class map's fast axis W, unless X does (then Y)
  a.fast_x = axis[0] == 2;
  a.f = a.fast_x ? 1 : (axis[1] == 2 ? 1 : 2);
  a.g = 3 - a.f;
  a.C = p->C;
  const dim3 grid(cdiv(n[0], EXPORT_TILE), cdiv(n[a.f], EXPORT_TILE), n[a.g]);
  const void* lut = p->lut;
  auto gather = [&](auto* m) {
    if (p->out_bytes == 1) export_gather_kernel<<<grid, 256, 0, s>>>(m, (const int32_t*)lut, (uint8_t*)p->out, a);
    else if (p->out_bytes == 2) export_gather_kernel<<<grid, 256, 0, s>>>(m, (const int32_t*)lut, (uint16_t*)p->out, a);
    else export_gather_kernel<<<grid, 256, 0, s>>>(m, (const int32_t*)lut, (uint32_t*)p->out, a);
  };
  if (p->logits) gather((const uint8_t*)cls);
  else if (p->cls_bytes == 1) gather((const uint8_t*)p->cls + first);
  else gather((const int32_t*)p->cls + first);
  MISEG_LAUNCH_CHECK("label_export gather");
  return MISEG_OK;
}

extern "C" int miseg_dropout(const miseg_dropout_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_dropout_params), MISEG_E_BADARG, "dropout: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_dropout_params));
  MISEG_REQUIRE(p->x && p->y && p->rows > 0 && p->C > 0 && p->rows_per_sample >= 0, MISEG_E_BADARG, "dropout: bad arguments");
  MISEG_REQUIRE(p->p >= 0.f && p->p < 1.f, MISEG_E_BADARG, "dropout: p = %f must lie in [0, 1)", (double)p->p);
  const unsigned thresh = (unsigned)lrintf(p->p * 65536.f);
  const float scale = 1.f / (1.f - (float)thresh / 65536.f);
  const uint64_t key = dropout_host_key(p->seed, p->stream_id);
  int grid = cdiv(p->rows * ((p->C + 3) / 4), 256 * 4);
  if (grid > 4096) grid = 4096;
  return dispatch_dtype(p->dtype, [&](auto* tag) -> int {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    dropout_kernel<T><<<grid, 256, 0, s>>>((const T*)p->x, p->ldx, (T*)p->y, p->ldy, p->rows, p->C, p->rows_per_sample, thresh, scale, key, p->step_dev);
    MISEG_LAUNCH_CHECK("dropout");
    return MISEG_OK;
  });
}

extern "C" int miseg_counter_add(uint64_t* c, uint64_t v, miseg_stream_t s_) {
  MISEG_REQUIRE(c, MISEG_E_BADARG, "counter_add: null pointer");
  counter_add_kernel<<<1, 1, 0, (hipStream_t)s_>>>(c, v);
  MISEG_LAUNCH_CHECK("counter_add");
  return MISEG_OK;
}

// one-thread spin on a device flag (round 4): returns once *flag >= *want - set by miseg_counter_copy from another stream / another graph launch -
// or after `timeout_ticks` of the 100 MHz wall clock, in which case *timed_out is incremented and the caller's results are not to be trusted
// (every wave reaches an exit: a flag that never comes costs the timeout, not the card).  Agent-scope acquire loads: the flag is written by
// a kernel that may run on another XCD.
__global__ void flag_wait_kernel(const uint64_t* flag, const uint64_t* want, uint64_t timeout_ticks, uint32_t* timed_out) {
  const uint64_t w = *want, t0 = wall_clock64();
  while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < w) {
    if (wall_clock64() - t0 > timeout_ticks) {
      if (timed_out) atomicAdd(timed_out, 1u);
      return;
    }
    __builtin_amdgcn_s_sleep(32);
  }
}

extern "C" int miseg_flag_wait(const uint64_t* flag, const uint64_t* want, uint64_t timeout_us, uint32_t* timed_out, miseg_stream_t s_) {
  MISEG_REQUIRE(flag && want, MISEG_E_BADARG, "flag_wait: null pointer");
  MISEG_REQUIRE(timeout_us > 0 && timeout_us <= 2000000, MISEG_E_BADARG, "flag_wait: timeout %llu us (1 .. 2,000,000)", (unsigned long long)timeout_us);
  flag_wait_kernel<<<1, 1, 0, (hipStream_t)s_>>>(flag, want, timeout_us * 100, timed_out);
  MISEG_LAUNCH_CHECK("flag_wait");
  return MISEG_OK;
}

__global__ void stamp_kernel(uint64_t* slot) { *slot = wall_clock64(); }

extern "C" int miseg_debug_stamp(uint64_t* slot, miseg_stream_t s_) {
  MISEG_REQUIRE(slot, MISEG_E_BADARG, "debug_stamp: null pointer");
  stamp_kernel<<<1, 1, 0, (hipStream_t)s_>>>(slot);
  MISEG_LAUNCH_CHECK("debug_stamp");
  return MISEG_OK;
}

extern "C" int miseg_counter_copy(uint64_t* d, const uint64_t* src, miseg_stream_t s_) {
  MISEG_REQUIRE(d && src, MISEG_E_BADARG, "counter_copy: null pointer");
  counter_copy_kernel<<<1, 1, 0, (hipStream_t)s_>>>(d, src);
  MISEG_LAUNCH_CHECK("counter_copy");
  return MISEG_OK;
}
