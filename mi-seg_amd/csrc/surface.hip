// Symmetric average surface distance after argmax (reference test.py:145-151: SurfaceDistanceMetric(symmetric=True, distance_metric='euclidean')).
// MONAI 1.1.0 metrics/surface_distance.py + metrics/utils.py restated (parity unpinned); per sample b and class c with
// P = (pred == c), G = (label == c):
//   * the masks are cropped to the tight box of P | G and squeezed: an axis on which the box is one voxel thick has no neighbours;
//   * edges E = M ^ erode(M) with a cross structure and a zero border (voxels on the box border with a neighbour outside it are edges);
//   * d(A -> B) = exact Euclidean distance of every voxel of E_A to the nearest voxel of E_B (inf rules in surface_finalize_kernel).
// Passes, all over the per-(b, c) boxes packed one after another into the distance buffers (one launch per pass covers every box that fits):
//   1. surface_classify_kernel: argmax (or the given class map) and the label as uint8 class maps + per-(b, c) boxes (LDS, then global atomicMin)
//   2. surface_edt_w_kernel:    edge bytes and the first EDT pass along the contiguous axis, one wave per line (prefix-max / suffix-min scans)
//   3. surface_edt_h_kernel:    exact lower envelope along H (Meijster's second phase), one thread per line, stacks in a [n][lines] scratch
//   4. surface_edt_d_gather_kernel: the same along D, fused with the gather: sqrt(d^2) summed in double at every edge voxel of the other set
//   5. surface_finalize_kernel: fixed-order sum of the per-workgroup partials, inf / NaN rules, fp64 [B][C'] out
// Squared distances are int32 and exact (every box side <= 4096: d^2 < 2^26 < SD_INF).
// Hausdorff distance (MONAI 1.1.0 metrics/hausdorff_distance.py) from the same launch set: an exact order statistic of
// the integer d^2 of every direction's list (sqrt is monotone), found by a two-level radix select, 2^26 = 8192 coarse x 8192 fine bins:
//   4'. surface_edt_d_select_kernel: pass 4 that also leaves each edge voxel's d^2 in the H pass's dead input buffer and counts d^2 >> 13
//       (LDS histogram, non-zero bins flushed with one integer atomic each into coarse[item][dir][8192])
//   4a. surface_rank_kernel:   prefix scan of one coarse table: the coarse bins that hold ranks lo and hi, and the ranks inside them
//   4b. surface_select_kernel: d^2 & 8191 of the edge voxels whose coarse bin is one of those (at most two), LDS histogram -> fine[item][dir][2][8192]
//   5'. surface_finalize_hd_kernel: the two exact d^2 from the fine tables, sqrt in double, the percentile's interpolation, inf / NaN rules; the
//       ASD by the same sums in the same order as pass 5
// Normalized surface Dice at per-class tolerances: the share of both lists' distances that are <= tau_c, counted on the
// integer d^2 against the host-made bound T_c = max {k : sqrt((double)k) <= tau_c} by the NSD instantiations of pass 4 / 4' (one uint32 count per
// workgroup beside its partial) and divided once, in double, by passes 5 / 5'.
// Integer counters and integer atomics only: no result depends on arrival order.
#include "common.h"
#include <float.h>
#include <limits.h>
#include <math.h>
#include <algorithm>
#include <type_traits>
#include <vector>

namespace miseg {

namespace {

constexpr int SD_MAXC = 64;
constexpr int SD_MAXDIM = 4096;
constexpr int32_t SD_INF = 1 << 30;      // "no seed on this line / plane": above every real squared distance, below INT_MAX after + n^2
constexpr uint8_t SD_NONE = 255;         // class-map value of a voxel that belongs to no class

// one (b, c) box; both directions live in the distance buffers at [off, off + vol) (seeds = E_G: d(P -> G)) and [off + vol, off + 2 vol)
// (seeds = E_P: d(G -> P)); edge bytes (bit 0: E_P, bit 1: E_G) at [off / 2, off / 2 + vol) of the edge buffer
struct SdItem {
  int32_t b, c, d0, h0, w0, nd, nh, nw;
  int64_t off;       // word offset of direction 0 within the group's buffers (= 2 x the volume of the boxes before it)
  int64_t wline0;    // first W-line of the box within its group (W pass: one wave per (d, h) line)
  int64_t hblk0;     // first workgroup of the box within its group (H pass: 2 x cdiv(nd nw, 256))
  int64_t dblk0;     // first workgroup of the box over ALL groups (D pass: 2 x cdiv(nh nw, 256)) = its first partial slot
};

struct SdPartial { double sum; unsigned long long n; };

constexpr int SD_SHIFT = 13;
constexpr int SD_BINS = 1 << SD_SHIFT;   // coarse bins d^2 >> 13 and fine bins d^2 & 8191 (d^2 < 2^26)
constexpr int SD_LBINS = 2048;           // coarse bins the D pass counts in LDS (d < 4096); the rare farther ones go to global memory one by one
constexpr uint32_t SD_NOBIN = 0xffffffffu;

// ranks lo / hi of one direction's list as (coarse bin, rank among the values of that bin); SD_NOBIN: the list is empty
struct SdSel { uint32_t bin_lo, rank_lo, bin_hi, rank_hi; };

// the Hausdorff tables behind the buffers of sd_layout, indexed by item over all groups (like the partials)
struct SdHdLayout { size_t coarse, fine, sel, total; };

// the surface Dice's tables behind those: the per-workgroup counts of d^2 <= T (indexed like the partials) and T per class
struct SdNsdLayout { size_t within, bound, total; };

struct SdLayout {
  size_t pcls, lcls, boxes, index, items, partials, edges, buf0, buf1, stack, total;
  int64_t cap;       // voxels of boxes one group may hold (the volume S)
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

SdLayout sd_layout(int B, int C, int D, int H, int W) {
  SdLayout L;
  const int64_t S = (int64_t)D * H * W;
  const size_t nblk = (size_t)B * C * 2 * cdiv((long)H * W, 256);
  L.cap = S;
  size_t o = 0;
  L.pcls = o;      o = align256(o + (size_t)B * S);
  L.lcls = o;      o = align256(o + (size_t)B * S);
  L.boxes = o;     o = align256(o + (size_t)B * C * 6 * 4);
  L.index = o;     o = align256(o + (size_t)B * C * 4);
  L.items = o;     o = align256(o + (size_t)B * C * sizeof(SdItem));
  L.partials = o;  o = align256(o + nblk * sizeof(SdPartial));
  L.edges = o;     o = align256(o + (size_t)S);
  L.buf0 = o;      o = align256(o + (size_t)2 * S * 4);
  L.buf1 = o;      o = align256(o + (size_t)2 * S * 4);
  L.stack = o;     o = align256(o + (size_t)2 * S * 4);
  L.total = o;
  return L;
}

SdHdLayout sd_hd_layout(const SdLayout& L, int B, int C) {
  SdHdLayout Q;
  const size_t items = (size_t)B * C;
  size_t o = L.total;
  Q.coarse = o;    o = align256(o + items * 2 * SD_BINS * 4);
  Q.fine = o;      o = align256(o + items * 2 * 2 * SD_BINS * 4);
  Q.sel = o;       o = align256(o + items * 2 * sizeof(SdSel));
  Q.total = o;
  return Q;
}

SdNsdLayout sd_nsd_layout(const SdHdLayout& Q, int B, int C, int H, int W) {
  SdNsdLayout N;
  const size_t nblk = (size_t)B * C * 2 * cdiv((long)H * W, 256);
  size_t o = Q.total;
  N.within = o;    o = align256(o + nblk * 4);
  N.bound = o;     o = align256(o + (size_t)C * 4);
  N.total = o;
  return N;
}

// the largest integer k with sqrt((double)k) <= tau (tau >= 0, finite), at most 2^26 - 1: above every real d^2 (sides <= 4096), below SD_INF.
// d <= tau <=> d^2 <= k for every d = sqrt((double)d2) the CPU restatement compares.
int32_t sd_nsd_bound(double tau) {
  const double lim = (double)((1 << 26) - 1);
  const double t2 = tau * tau;
  int64_t k = t2 < lim ? (int64_t)floor(t2) : (int64_t)lim;
  while (k > 0 && sqrt((double)k) > tau) --k;
  while (k + 1 <= (int64_t)lim && sqrt((double)(k + 1)) <= tau) ++k;
  return (int32_t)k;
}

template <class L> __device__ __forceinline__ int sd_label_at(const L* lab, int64_t i) { return (int)lab[i]; }

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// union of this lane's voxel into the box of class `cls` (SD_NONE: none): one pass of the wave per distinct class among its lanes
__device__ __forceinline__ void wave_box_update(int cls, int d, int h, int w, int* sbox) {
  unsigned long long pend = __ballot(cls != SD_NONE);
  while (pend) {
    const int leader = __ffsll((long long)pend) - 1;
    const int c = __shfl(cls, leader, 64);
    const bool mine = cls == c;
    const int v0 = wave_min_i32(mine ? d : INT_MAX), v1 = wave_min_i32(mine ? h : INT_MAX), v2 = wave_min_i32(mine ? w : INT_MAX);
    const int v3 = wave_min_i32(mine ? -d : INT_MAX), v4 = wave_min_i32(mine ? -h : INT_MAX), v5 = wave_min_i32(mine ? -w : INT_MAX);
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&sbox[c * 6 + 0], v0); atomicMin(&sbox[c * 6 + 1], v1); atomicMin(&sbox[c * 6 + 2], v2);
      atomicMin(&sbox[c * 6 + 3], v3); atomicMin(&sbox[c * 6 + 4], v4); atomicMin(&sbox[c * 6 + 5], v5);
    }
    pend &= ~__ballot(mine);
  }
}

// boxes[b][c][6] = (dmin, hmin, wmin, -dmax, -hmax, -wmax), INT_MAX where the class is absent (filled before the launch)
template <class L, bool LOGITS>
__global__ void __launch_bounds__(256) surface_classify_kernel(const float* __restrict__ logits, const int32_t* __restrict__ pred, const L* __restrict__ label,
                                                               int C, int H, int W, int64_t S, uint8_t* __restrict__ pcls, uint8_t* __restrict__ lcls,
                                                               int* __restrict__ boxes) {
  __shared__ int sbox[SD_MAXC * 6];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < C * 6; i += 256) sbox[i] = INT_MAX;
  __syncthreads();
  const int64_t HW = (int64_t)H * W;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < S; base += (int64_t)gridDim.x * 256) {      // uniform trip count: the ballots see whole waves
    const int64_t s = base + tid;
    int p = SD_NONE, g = SD_NONE, d = 0, h = 0, w = 0;
    if (s < S) {
      if constexpr (LOGITS) {
        const float* xb = logits + (int64_t)b * C * S + s;
        float mx = xb[0];
        p = 0;
        for (int c = 1; c < C; ++c) {
          const float v = xb[(int64_t)c * S];
          if (v > mx) { mx = v; p = c; }          // strict: the FIRST maximum wins (torch.argmax, dice_count_kernel)
        }
      } else {
        const int v = pred[(int64_t)b * S + s];
        p = (v >= 0 && v < C) ? v : SD_NONE;
      }
      const int l = sd_label_at(label, (int64_t)b * S + s);
      g = (l >= 0 && l < C) ? l : SD_NONE;
      pcls[(int64_t)b * S + s] = (uint8_t)p;
      lcls[(int64_t)b * S + s] = (uint8_t)g;
      d = (int)(s / HW);
      const int64_t r = s - (int64_t)d * HW;
      h = (int)(r / W);
      w = (int)(r - (int64_t)h * W);
    }
    wave_box_update(p, d, h, w, sbox);
    wave_box_update(g != p ? g : SD_NONE, d, h, w, sbox);
  }
  __syncthreads();
  for (int i = tid; i < C * 6; i += 256)
    if (sbox[i] != INT_MAX) atomicMin(&boxes[(int64_t)b * C * 6 + i], sbox[i]);
}

// the item of workgroup / wave `x` among n items whose first index is key(item) (ascending, key(items[0]) <= x)
template <class K> __device__ __forceinline__ int find_item(const SdItem* items, int n, int64_t x, K key) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (key(items[mid]) <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// (d, h, w) box-local: is the voxel an edge of the mask {cls == c}?  cm points at the voxel in its class map.
__device__ __forceinline__ bool sd_edge(const uint8_t* cm, int c, int d, int h, int w, const SdItem& it, int64_t HW, int W) {
  if (cm[0] != c) return false;
  bool e = false;
  if (it.nd > 1) e = e || d == 0 || d == it.nd - 1 || cm[-HW] != c || cm[HW] != c;
  if (it.nh > 1) e = e || h == 0 || h == it.nh - 1 || cm[-W] != c || cm[W] != c;
  if (it.nw > 1) e = e || w == 0 || w == it.nw - 1 || cm[-1] != c || cm[1] != c;
  return e;
}

// pass 2: one wave per (d, h) line of a box: edge bytes, then the distance along W to the nearest seed of each direction, squared (SD_INF: none)
__global__ void __launch_bounds__(256) surface_edt_w_kernel(const SdItem* __restrict__ items, int nitems, int64_t nlines, const uint8_t* __restrict__ pcls,
                                                            const uint8_t* __restrict__ lcls, int H, int W, int64_t S, uint8_t* __restrict__ edges,
                                                            int32_t* __restrict__ out) {
  const int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (line >= nlines) return;                        // whole waves leave: no barrier in this kernel
  const int lane = threadIdx.x & 63;
  const SdItem it = items[find_item(items, nitems, line, [](const SdItem& x) { return x.wline0; })];
  const int64_t l = line - it.wline0;
  const int d = (int)(l / it.nh), h = (int)(l - (int64_t)d * it.nh), n = it.nw;
  const int64_t HW = (int64_t)H * W, vol = (int64_t)it.nd * it.nh * it.nw;
  const int64_t g0 = (int64_t)it.b * S + (int64_t)(it.d0 + d) * HW + (int64_t)(it.h0 + h) * W + it.w0;    // voxel x = 0 of the line in the class maps
  const int64_t o0 = (int64_t)(d * it.nh + h) * n;                                                            // ... in the box
  int32_t* out0 = out + it.off + o0;             // seeds E_G: d(P -> G)
  int32_t* out1 = out + it.off + vol + o0;       // seeds E_P: d(G -> P)
  uint8_t* eb = edges + it.off / 2 + o0;
  // forward: edges and the nearest seed at or left of x (prefix max of the seed positions), kept in out0 / out1 for the backward scan
  int carry0 = -1, carry1 = -1;
  for (int x0 = 0; x0 < n; x0 += 64) {
    const int x = x0 + lane;
    bool ep = false, eg = false;
    if (x < n) {
      ep = sd_edge(pcls + g0 + x, it.c, d, h, x, it, HW, W);
      eg = sd_edge(lcls + g0 + x, it.c, d, h, x, it, HW, W);
      eb[x] = (uint8_t)(ep | (eg << 1));
    }
    int l0 = eg ? x : -1, l1 = ep ? x : -1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t0 = __shfl_up(l0, o, 64), t1 = __shfl_up(l1, o, 64);
      if (lane >= o) { l0 = max(l0, t0); l1 = max(l1, t1); }
    }
    l0 = max(l0, carry0);
    l1 = max(l1, carry1);
    if (x < n) { out0[x] = l0; out1[x] = l1; }
    carry0 = __shfl(l0, 63, 64);
    carry1 = __shfl(l1, 63, 64);
  }
  // backward: the nearest seed at or right of x (suffix min), then the squared distance to the nearer of the two
  carry0 = INT_MAX; carry1 = INT_MAX;
  for (int x0 = ((n - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
    const int x = x0 + lane;
    int l0 = -1, l1 = -1;
    if (x < n) { l0 = out0[x]; l1 = out1[x]; }
    int r0 = (x < n && l0 == x) ? x : INT_MAX, r1 = (x < n && l1 == x) ? x : INT_MAX;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t0 = __shfl_down(r0, o, 64), t1 = __shfl_down(r1, o, 64);
      if (lane + o < 64) { r0 = min(r0, t0); r1 = min(r1, t1); }
    }
    r0 = min(r0, carry0);
    r1 = min(r1, carry1);
    if (x < n) {
      int g = INT_MAX;
      if (l0 >= 0) g = x - l0;
      if (r0 != INT_MAX) g = min(g, r0 - x);
      out0[x] = g == INT_MAX ? SD_INF : g * g;
      g = INT_MAX;
      if (l1 >= 0) g = x - l1;
      if (r1 != INT_MAX) g = min(g, r1 - x);
      out1[x] = g == INT_MAX ? SD_INF : g * g;
    }
    carry0 = __shfl(r0, 0, 64);
    carry1 = __shfl(r1, 0, 64);
  }
}

// Meijster's second phase on one line: f(u) = in[u * fs], n values; dt(u) = min_i f(i) + (u - i)^2 is handed to emit(u, dt) for u = n-1 .. 0.
// The envelope stack (s: the parabola, t: where it starts to win) lives in st[q * ss], packed s << 16 | t.
template <class E>
__device__ __forceinline__ void envelope_line(const int32_t* __restrict__ in, int64_t fs, int n, uint32_t* __restrict__ st, int64_t ss, E emit) {
  int q = 0, sq = 0, tq = 0;
  int64_t fq = in[0];
  st[0] = 0u;
  for (int u = 1; u < n; ++u) {
    const int64_t fu = in[(int64_t)u * fs];
    // pop while the top parabola loses to u where it starts to win
    while (q >= 0 && (int64_t)(tq - sq) * (tq - sq) + fq > (int64_t)(tq - u) * (tq - u) + fu) {
      --q;
      if (q >= 0) {
        const uint32_t e = st[(int64_t)q * ss];
        sq = (int)(e >> 16); tq = (int)(e & 0xffffu);
        fq = in[(int64_t)sq * fs];
      }
    }
    if (q < 0) {
      q = 0; sq = u; tq = 0; fq = fu;
      st[0] = (uint32_t)u << 16;
    } else {
      // first position where u is at least as near: 1 + floor(sep); the numerator is >= 2 tq (u - sq) >= 0 here
      const int64_t w = 1 + ((int64_t)u * u - (int64_t)sq * sq + fu - fq) / (2 * (int64_t)(u - sq));
      if (w < n) {
        ++q; sq = u; tq = (int)w; fq = fu;
        st[(int64_t)q * ss] = ((uint32_t)u << 16) | (uint32_t)w;
      }
    }
  }
  for (int u = n - 1; u >= 0; --u) {
    emit(u, (int32_t)((int64_t)(u - sq) * (u - sq) + fq));
    if (u == tq && q > 0) {
      --q;
      const uint32_t e = st[(int64_t)q * ss];
      sq = (int)(e >> 16); tq = (int)(e & 0xffffu);
      fq = in[(int64_t)sq * fs];
    }
  }
}

// pass 3: along H, one thread per (direction, d, w) line; adjacent threads take adjacent w (coalesced), workgroups never straddle a box
__global__ void __launch_bounds__(256) surface_edt_h_kernel(const SdItem* __restrict__ items, int nitems, const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                            uint32_t* __restrict__ stack) {
  const SdItem it = items[find_item(items, nitems, (int64_t)blockIdx.x, [](const SdItem& x) { return x.hblk0; })];
  const int64_t nl = (int64_t)it.nd * it.nw, vol = nl * it.nh;
  const int64_t nb = cdiv(nl, 256);
  int64_t lb = (int64_t)blockIdx.x - it.hblk0;
  const int dir = lb >= nb;
  const int64_t l = (lb - dir * nb) * 256 + threadIdx.x;
  if (l >= nl) return;
  const int d = (int)(l / it.nw), w = (int)(l - (int64_t)d * it.nw);
  const int64_t base = it.off + dir * vol + (int64_t)d * it.nh * it.nw + w;     // (d, h = 0, w) of this direction's box
  int32_t* o = out + base;
  envelope_line(in + base, it.nw, it.nh, stack + it.off + dir * vol + l, nl, [&](int u, int32_t v) { o[(int64_t)u * it.nw] = v; });
}

__device__ __forceinline__ void block_sum_partial(double s, unsigned long long n, SdPartial* __restrict__ slot) {
  __shared__ double ws[4];
  __shared__ unsigned long long wn[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    n += __shfl_xor(n, o, 64);
  }
  if ((threadIdx.x & 63) == 0) { ws[threadIdx.x >> 6] = s; wn[threadIdx.x >> 6] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    slot->sum = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    slot->n = wn[0] + wn[1] + wn[2] + wn[3];
  }
}

// the workgroup's count of d^2 <= T (at most 256 x 4096), after block_sum_partial: its own LDS words, one more barrier
__device__ __forceinline__ void block_sum_within(uint32_t m, uint32_t* __restrict__ slot) {
  __shared__ uint32_t wm[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) *slot = wm[0] + wm[1] + wm[2] + wm[3];
}

// pass 4: along D, one thread per (direction, h, w) line, fused with the gather: direction 0 sums sqrt(d^2) over E_P (distance to E_G),
// direction 1 over E_G (distance to E_P); one partial per workgroup, in slot dblk0 + the workgroup's index within the box.
// HD: every edge voxel's d^2 is also left in dout (the layout of `in`) and counted by d^2 >> 13 (values without a seed fall into the last bin:
// their lists are all inf and never selected from) in hist (LDS, SD_LBINS bins + the last one), then in coarse[item_base + item][dir][].
// NSD: the edge voxels with d^2 <= bound[class of the item] are counted too, one count per workgroup in within[the partial's slot].
template <bool HD, bool NSD>
__device__ __forceinline__ void sd_d_pass(const SdItem* __restrict__ items, int nitems, int64_t dblk_base, const int32_t* __restrict__ in,
                                          const uint8_t* __restrict__ edges, uint32_t* __restrict__ stack, SdPartial* __restrict__ partials, int item_base,
                                          int32_t* __restrict__ dout, uint32_t* __restrict__ coarse, uint32_t* hist, const int32_t* __restrict__ bound,
                                          uint32_t* __restrict__ within) {
  const int k = find_item(items, nitems, (int64_t)blockIdx.x + dblk_base, [](const SdItem& x) { return x.dblk0; });
  const SdItem it = items[k];
  const int64_t nl = (int64_t)it.nh * it.nw, vol = nl * it.nd;
  const int64_t nb = cdiv(nl, 256);
  const int64_t lb = (int64_t)blockIdx.x + dblk_base - it.dblk0;
  const int dir = lb >= nb;
  const int64_t l = (lb - dir * nb) * 256 + threadIdx.x;
  uint32_t* ctab = nullptr;
  if constexpr (HD) {
    ctab = coarse + ((int64_t)(item_base + k) * 2 + dir) * SD_BINS;
    for (int j = threadIdx.x; j <= SD_LBINS; j += 256) hist[j] = 0u;
    __syncthreads();
  }
  double sum = 0.0;
  unsigned long long cnt = 0;
  int32_t T = 0;
  uint32_t hit = 0;
  if constexpr (NSD) T = bound[it.c];
  if (l < nl) {
    const uint8_t* eb = edges + it.off / 2 + l;
    const uint8_t bit = dir == 0 ? 1 : 2;
    int32_t* o = nullptr;
    if constexpr (HD) o = dout + it.off + dir * vol + l;
    envelope_line(in + it.off + dir * vol + l, nl, it.nd, stack + it.off + dir * vol + l, nl, [&](int u, int32_t v) {
      if (eb[(int64_t)u * nl] & bit) {
        sum += sqrt((double)v);
        ++cnt;
        if constexpr (NSD) hit += v <= T;
        if constexpr (HD) {
          o[(int64_t)u * nl] = v;
          const int bin = min(v >> SD_SHIFT, SD_BINS - 1);
          if (bin < SD_LBINS) atomicAdd(&hist[bin], 1u);
          else if (bin == SD_BINS - 1) atomicAdd(&hist[SD_LBINS], 1u);       // no seed: a whole list at one address
          else atomicAdd(&ctab[bin], 1u);
        }
      }
    });
  }
  block_sum_partial(sum, cnt, partials + it.dblk0 + lb);        // its barrier also closes the histogram
  if constexpr (NSD) block_sum_within(hit, within + it.dblk0 + lb);
  if constexpr (HD) {
    for (int j = threadIdx.x; j <= SD_LBINS; j += 256) {
      const uint32_t c = hist[j];
      if (c) atomicAdd(&ctab[j < SD_LBINS ? j : SD_BINS - 1], c);
    }
  }
}

__global__ void __launch_bounds__(256) surface_edt_d_gather_kernel(const SdItem* __restrict__ items, int nitems, int64_t dblk_base, const int32_t* __restrict__ in,
                                                                   const uint8_t* __restrict__ edges, uint32_t* __restrict__ stack, SdPartial* __restrict__ partials) {
  sd_d_pass<false, false>(items, nitems, dblk_base, in, edges, stack, partials, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
}

__global__ void __launch_bounds__(256) surface_edt_d_select_kernel(const SdItem* __restrict__ items, int nitems, int64_t dblk_base, const int32_t* __restrict__ in,
                                                                   const uint8_t* __restrict__ edges, uint32_t* __restrict__ stack, SdPartial* __restrict__ partials,
                                                                   int item_base, int32_t* __restrict__ dout, uint32_t* __restrict__ coarse) {
  __shared__ uint32_t hist[SD_LBINS + 1];
  sd_d_pass<true, false>(items, nitems, dblk_base, in, edges, stack, partials, item_base, dout, coarse, hist, nullptr, nullptr);
}

// passes 4 and 4' with the surface Dice's count
__global__ void __launch_bounds__(256) surface_edt_d_gather_nsd_kernel(const SdItem* __restrict__ items, int nitems, int64_t dblk_base, const int32_t* __restrict__ in,
                                                                       const uint8_t* __restrict__ edges, uint32_t* __restrict__ stack, SdPartial* __restrict__ partials,
                                                                       const int32_t* __restrict__ bound, uint32_t* __restrict__ within) {
  sd_d_pass<false, true>(items, nitems, dblk_base, in, edges, stack, partials, 0, nullptr, nullptr, nullptr, bound, within);
}

__global__ void __launch_bounds__(256) surface_edt_d_select_nsd_kernel(const SdItem* __restrict__ items, int nitems, int64_t dblk_base, const int32_t* __restrict__ in,
                                                                       const uint8_t* __restrict__ edges, uint32_t* __restrict__ stack, SdPartial* __restrict__ partials,
                                                                       int item_base, int32_t* __restrict__ dout, uint32_t* __restrict__ coarse,
                                                                       const int32_t* __restrict__ bound, uint32_t* __restrict__ within) {
  __shared__ uint32_t hist[SD_LBINS + 1];
  sd_d_pass<true, true>(items, nitems, dblk_base, in, edges, stack, partials, item_base, dout, coarse, hist, bound, within);
}

// ranks of the percentile in an ascending list of n > 0 values (numpy's "linear" method; pct <= 0: the maximum): value = v_lo + (v_hi - v_lo) frac
__device__ __forceinline__ void sd_ranks(double pct, unsigned long long n, unsigned long long& lo, unsigned long long& hi, double& frac) {
  if (!(pct > 0.0)) { lo = hi = n - 1; frac = 0.0; return; }
  const double pos = pct / 100.0 * (double)(n - 1);
  lo = (unsigned long long)floor(pos);
  if (lo > n - 1) lo = n - 1;
  hi = lo + 1 < n ? lo + 1 : n - 1;
  frac = pos - (double)lo;
}

// 256 threads over one table of SD_BINS counters: thread t owns bins [32 t, 32 t + 32).  sd_block_prefix: the count before and inside the
// thread's bins, the total in sh[256] (sh: 257 words of LDS, free again on return).  sd_resolve: the one thread whose bins hold rank r
// (r < total) writes the bin and r's rank inside it.
struct SdPrefix { unsigned long long excl, sum; };

__device__ __forceinline__ SdPrefix sd_block_prefix(const uint32_t* __restrict__ tab, unsigned long long* sh) {
  const int t = threadIdx.x;
  SdPrefix p;
  p.sum = 0;
  for (int j = 0; j < SD_BINS / 256; ++j) p.sum += tab[t * (SD_BINS / 256) + j];
  sh[t] = p.sum;
  __syncthreads();
  p.excl = 0;
  for (int j = 0; j < t; ++j) p.excl += sh[j];
  if (t == 255) sh[256] = p.excl + p.sum;
  __syncthreads();
  return p;
}

__device__ __forceinline__ void sd_resolve(const uint32_t* __restrict__ tab, const SdPrefix& p, unsigned long long r, uint32_t* bin, uint32_t* rank) {
  if (r < p.excl || r >= p.excl + p.sum) return;
  unsigned long long acc = p.excl;
  for (int j = 0; j < SD_BINS / 256; ++j) {
    const int b = threadIdx.x * (SD_BINS / 256) + j;
    const uint32_t c = tab[b];
    if (r < acc + c) { *bin = (uint32_t)b; *rank = (uint32_t)(r - acc); return; }
    acc += c;
  }
}

// pass 4a: one workgroup per (item of the group, direction): where ranks lo and hi of the direction's list fall in its coarse table
__global__ void __launch_bounds__(256) surface_rank_kernel(const uint32_t* __restrict__ coarse, int item_base, double pct, SdSel* __restrict__ sels) {
  __shared__ unsigned long long sh[257];
  __shared__ uint32_t res[4];
  const int64_t slot = (int64_t)(item_base + blockIdx.x) * 2 + blockIdx.y;
  const uint32_t* tab = coarse + slot * SD_BINS;
  if (threadIdx.x == 0) { res[0] = SD_NOBIN; res[1] = 0u; res[2] = SD_NOBIN; res[3] = 0u; }
  const SdPrefix p = sd_block_prefix(tab, sh);
  const unsigned long long n = sh[256];
  if (n > 0) {
    unsigned long long lo, hi;
    double frac;
    sd_ranks(pct, n, lo, hi, frac);
    sd_resolve(tab, p, lo, &res[0], &res[1]);
    sd_resolve(tab, p, hi, &res[2], &res[3]);
  }
  __syncthreads();
  if (threadIdx.x == 0) { SdSel s; s.bin_lo = res[0]; s.rank_lo = res[1]; s.bin_hi = res[2]; s.rank_hi = res[3]; sels[slot] = s; }
}

// pass 4b: workgroups (x, item of the group x direction, which of lo / hi) stride over the box: the low 13 bits of the edge voxels' d^2 whose
// coarse bin is the selected one, counted in LDS, then in fine[item][dir][which][].  hi shares lo's table when both fall in one coarse bin.
// The edge bytes are read 16 at a time from 16-byte aligned addresses (up to 15 bytes before and after the box are read and masked off: they
// lie inside the workspace); d^2 is read at the edge voxels only.
__global__ void __launch_bounds__(256) surface_select_kernel(const SdItem* __restrict__ items, int item_base, const SdSel* __restrict__ sels,
                                                             const uint8_t* __restrict__ edges, const int32_t* __restrict__ d2, uint32_t* __restrict__ fine) {
  __shared__ uint32_t hist[SD_BINS];
  const int k = item_base + (blockIdx.y >> 1), dir = blockIdx.y & 1, which = blockIdx.z;
  const SdItem it = items[k];
  const int64_t vol = (int64_t)it.nd * it.nh * it.nw;
  const uint8_t* eb = edges + it.off / 2;
  const int a = (int)((uintptr_t)eb & 15);
  const int64_t nchunk = (vol + a + 15) >> 4;
  if ((int64_t)blockIdx.x * 256 >= nchunk) return;
  const SdSel sel = sels[(int64_t)k * 2 + dir];
  const uint32_t target = which ? sel.bin_hi : sel.bin_lo;
  if (target == SD_NOBIN || (which && sel.bin_hi == sel.bin_lo)) return;
  for (int j = threadIdx.x; j < SD_BINS; j += 256) hist[j] = 0u;
  __syncthreads();
  const int32_t* v = d2 + it.off + dir * vol;
  const uint32_t mask = (dir == 0 ? 1u : 2u) * 0x01010101u;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (int64_t)gridDim.x * 256) {
    const int64_t i0 = c * 16 - a;
    const uint4 q = *reinterpret_cast<const uint4*>(eb + i0);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t e = w[j] & mask;
      while (e) {
        const int64_t i = i0 + j * 4 + ((__ffs((int)e) - 1) >> 3);
        e &= e - 1;
        if (i >= 0 && i < vol) {
          const int32_t x = v[i];
          if ((uint32_t)min(x >> SD_SHIFT, SD_BINS - 1) == target) atomicAdd(&hist[x & (SD_BINS - 1)], 1u);
        }
      }
    }
  }
  __syncthreads();
  uint32_t* ftab = fine + (((int64_t)k * 2 + dir) * 2 + which) * SD_BINS;
  for (int j = threadIdx.x; j < SD_BINS; j += 256) {
    const uint32_t c = hist[j];
    if (c) atomicAdd(&ftab[j], c);
  }
}

// the partials of one box in their fixed order: s[dir], n[dir] (n[0] = |E_P|, n[1] = |E_G|)
__device__ __forceinline__ void sd_sum_partials(const SdItem& it, const SdPartial* __restrict__ partials, double* s, unsigned long long* n) {
  const int64_t nb = cdiv((int64_t)it.nh * it.nw, 256);
  s[0] = s[1] = 0.0;
  n[0] = n[1] = 0;
  for (int dir = 0; dir < 2; ++dir)
    for (int64_t j = 0; j < nb; ++j) {
      const SdPartial p = partials[it.dblk0 + dir * nb + j];
      s[dir] += p.sum;
      n[dir] += p.n;
    }
}

// rules of MONAI's get_surface_distance / compute_average_surface_distance
__device__ __forceinline__ double sd_asd_value(const double* s, const unsigned long long* n, int symmetric) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  const unsigned long long np = n[0], ng = n[1];   // |E_P|, |E_G|
  // d(P -> G): |E_P| infs if E_G is empty, else |E_G| infs if E_P is empty, else the distances
  unsigned long long tot = 0;
  bool has_inf = false;
  double sum = 0.0;
  if (ng == 0) { tot += np; has_inf |= np > 0; }
  else if (np == 0) { tot += ng; has_inf = true; }
  else { tot += np; sum += s[0]; }
  if (symmetric) {
    if (np == 0) { tot += ng; has_inf |= ng > 0; }
    else if (ng == 0) { tot += np; has_inf = true; }
    else { tot += ng; sum += s[1]; }
  }
  return tot == 0 ? nan : has_inf ? inf : sum / (double)tot;
}

// the surface Dice of one box: its workgroups' counts of d^2 <= T in the order of sd_sum_partials, over both lists' lengths.  Both lists have
// |E_P| + |E_G| entries in all whichever edge set is empty (DESIGN.md section 7.1 rule 4): NaN if that is 0; all inf, so 0, if one set is empty.
__device__ __forceinline__ double sd_nsd_value(const SdItem& it, const uint32_t* __restrict__ within, const unsigned long long* n) {
  if (n[0] == 0 && n[1] == 0) return __longlong_as_double(0x7ff8000000000000ll);
  if (n[0] == 0 || n[1] == 0) return 0.0;
  const int64_t nb = cdiv((int64_t)it.nh * it.nw, 256);
  unsigned long long m = 0;
  for (int64_t j = 0; j < 2 * nb; ++j) m += within[it.dblk0 + j];
  return (double)m / (double)(n[0] + n[1]);
}

// pass 5: one thread per (b, c'); asd or nsd may be NULL (not both)
__global__ void surface_finalize_kernel(const int32_t* __restrict__ index, const SdItem* __restrict__ items, const SdPartial* __restrict__ partials, int B, int C,
                                        int c0, int symmetric, double* __restrict__ asd, const uint32_t* __restrict__ within, double* __restrict__ nsd) {
  const int Cp = C - c0;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * Cp) return;
  const int b = i / Cp, c = c0 + i % Cp;
  const int k = index[b * C + c];
  if (k < 0) {                                     // no foreground: both edge sets empty
    if (asd) asd[i] = __longlong_as_double(0x7ff8000000000000ll);
    if (nsd) nsd[i] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const SdItem it = items[k];
  double s[2];
  unsigned long long n[2];
  sd_sum_partials(it, partials, s, n);
  if (asd) asd[i] = sd_asd_value(s, n, symmetric);
  if (nsd) nsd[i] = sd_nsd_value(it, within, n);
}

// pass 5': one workgroup per (b, c'): the ASD and the surface Dice as pass 5 (thread 0), and the Hausdorff distance from the fine tables.  h(A -> B): NaN for an
// empty list, inf when one edge set is empty (every percentile: DESIGN.md section 7.5 rule 2), else the percentile of the list.
__global__ void __launch_bounds__(256) surface_finalize_hd_kernel(const int32_t* __restrict__ index, const SdItem* __restrict__ items, const SdPartial* __restrict__ partials,
                                                                  const SdSel* __restrict__ sels, const uint32_t* __restrict__ fine, int C, int c0, int symmetric,
                                                                  int directed, double pct, double* __restrict__ asd, double* __restrict__ hd,
                                                                  const uint32_t* __restrict__ within, double* __restrict__ nsd) {
  __shared__ unsigned long long sh[257];
  __shared__ unsigned long long sn[2];
  __shared__ uint32_t res[4];
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  const int Cp = C - c0;
  const int i = blockIdx.x;
  const int b = i / Cp, c = c0 + i % Cp;
  const int k = index[b * C + c];
  if (k < 0) {                                     // no foreground: both edge sets empty
    if (threadIdx.x == 0) { if (asd) asd[i] = nan; hd[i] = nan; if (nsd) nsd[i] = nan; }
    return;
  }
  if (threadIdx.x == 0) {
    const SdItem it = items[k];
    double s[2];
    unsigned long long n[2];
    sd_sum_partials(it, partials, s, n);
    if (asd) asd[i] = sd_asd_value(s, n, symmetric);
    if (nsd) nsd[i] = sd_nsd_value(it, within, n);
    sn[0] = n[0]; sn[1] = n[1];
  }
  __syncthreads();
  if (sn[0] == 0 || sn[1] == 0) {                  // both directions' lists are empty together, or all inf together
    if (threadIdx.x == 0) hd[i] = (sn[0] == 0 && sn[1] == 0) ? nan : inf;
    return;
  }
  double h[2] = {0.0, 0.0};
  for (int dir = 0; dir < (directed ? 1 : 2); ++dir) {
    const SdSel sel = sels[(int64_t)k * 2 + dir];
    const uint32_t* tlo = fine + ((int64_t)k * 2 + dir) * 2 * SD_BINS;
    uint32_t unused;
    SdPrefix p = sd_block_prefix(tlo, sh);
    sd_resolve(tlo, p, sel.rank_lo, &res[0], &unused);
    if (sel.bin_hi == sel.bin_lo) {
      sd_resolve(tlo, p, sel.rank_hi, &res[1], &unused);
    } else {
      p = sd_block_prefix(tlo + SD_BINS, sh);
      sd_resolve(tlo + SD_BINS, p, sel.rank_hi, &res[1], &unused);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long lo, hi;
      double frac;
      sd_ranks(pct, sn[dir], lo, hi, frac);
      const double vlo = sqrt((double)((sel.bin_lo << SD_SHIFT) | res[0])), vhi = sqrt((double)((sel.bin_hi << SD_SHIFT) | res[1]));
      h[dir] = __dadd_rn(vlo, __dmul_rn(vhi - vlo, frac));          // two roundings, as the CPU restatement: no fused multiply-add
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) hd[i] = directed ? h[0] : fmax(h[0], h[1]);
}

template <class F> int sd_dispatch_label(int dt, F&& f) {
  switch (dt) {
    case MISEG_LABEL_F32: return f((const float*)nullptr);
    case MISEG_LABEL_I32: return f((const int32_t*)nullptr);
    case MISEG_LABEL_I64: return f((const int64_t*)nullptr);
    case MISEG_LABEL_U8: return f((const uint8_t*)nullptr);
  }
  return set_error(MISEG_E_BADARG, "surface_distance: unknown label dtype %d", dt);
}

}  // namespace

}  // namespace miseg

using namespace miseg;

extern "C" size_t miseg_surface_distance_workspace_bytes(int B, int C, int D, int H, int W) {
  if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  return sd_layout(B, C, D, H, W).total;
}

extern "C" size_t miseg_surface_metrics_workspace_bytes(int B, int C, int D, int H, int W) {
  if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  return sd_hd_layout(sd_layout(B, C, D, H, W), B, C).total;
}

extern "C" size_t miseg_surface_dice_workspace_bytes(int B, int C, int D, int H, int W) {
  if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  return sd_nsd_layout(sd_hd_layout(sd_layout(B, C, D, H, W), B, C), B, C, H, W).total;
}

namespace miseg {
namespace {

// the three entry points: the ASD (p.asd), the Hausdorff distance (p.hd), the surface Dice (p.nsd), or several from one launch set; `who` names
// the entry point in messages
int surface_run(const miseg_surface_dice_params& q, const char* who, hipStream_t s) {
  const miseg_surface_dice_params* p = &q;
  MISEG_REQUIRE((p->logits != nullptr) != (p->pred != nullptr), MISEG_E_BADARG, "%s: exactly one of logits / pred", who);
  MISEG_REQUIRE(p->label && p->workspace && (p->asd || p->hd || p->nsd), MISEG_E_BADARG, "%s: null pointer", who);
  MISEG_REQUIRE(!p->nsd || p->thresholds, MISEG_E_BADARG, "%s: nsd without thresholds", who);
  MISEG_REQUIRE(!p->hd || p->percentile <= 100.0, MISEG_E_BADARG, "%s: percentile %g (at most 100; <= 0: the maximum)", who, p->percentile);
  MISEG_REQUIRE(p->B > 0 && p->C >= 1 && p->C <= SD_MAXC, MISEG_E_UNSUPPORTED, "%s: B %d, C %d (1..%d)", who, p->B, p->C, SD_MAXC);
  MISEG_REQUIRE(p->D > 0 && p->H > 0 && p->W > 0 && p->D <= SD_MAXDIM && p->H <= SD_MAXDIM && p->W <= SD_MAXDIM, MISEG_E_UNSUPPORTED,
                "%s: volume %d x %d x %d (a 3-D volume, every side 1..%d)", who, p->D, p->H, p->W, SD_MAXDIM);
  MISEG_REQUIRE(!p->hd || (int64_t)p->D * p->H * p->W < ((int64_t)1 << 32), MISEG_E_UNSUPPORTED, "%s: the Hausdorff distance counts in 32 bits: fewer than 2^32 voxels",
                who);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  MISEG_REQUIRE(hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone, MISEG_E_UNSUPPORTED,
                "%s: reads the class boxes back to the host, cannot be captured", who);
  const int B = p->B, C = p->C, c0 = p->include_background ? 0 : 1, Cp = C - c0;
  std::vector<int32_t> hbound((size_t)C, 0);       // T per class c (class 0 without the background: never read)
  if (p->nsd)
    for (int j = 0; j < Cp; ++j) {
      const double tau = p->thresholds[j];
      MISEG_REQUIRE(tau >= 0.0 && tau <= DBL_MAX, MISEG_E_BADARG, "%s: thresholds[%d] = %g (finite and >= 0)", who, j, tau);
      hbound[(size_t)c0 + j] = sd_nsd_bound(tau);
    }
  if (Cp == 0) return MISEG_OK;
  const int64_t S = (int64_t)p->D * p->H * p->W;
  const SdLayout L = sd_layout(B, C, p->D, p->H, p->W);
  char* ws = (char*)p->workspace;
  uint8_t* pcls = (uint8_t*)(ws + L.pcls);
  uint8_t* lcls = (uint8_t*)(ws + L.lcls);
  int* boxes = (int*)(ws + L.boxes);
  int32_t* index = (int32_t*)(ws + L.index);
  SdItem* items = (SdItem*)(ws + L.items);
  SdPartial* partials = (SdPartial*)(ws + L.partials);
  uint8_t* edges = (uint8_t*)(ws + L.edges);
  int32_t* buf0 = (int32_t*)(ws + L.buf0);
  int32_t* buf1 = (int32_t*)(ws + L.buf1);
  uint32_t* stack = (uint32_t*)(ws + L.stack);
  const SdHdLayout Q = sd_hd_layout(L, B, C);        // read only with hd: miseg_surface_distance's workspace ends at L.total
  uint32_t* coarse = (uint32_t*)(ws + Q.coarse);
  uint32_t* fine = (uint32_t*)(ws + Q.fine);
  SdSel* sels = (SdSel*)(ws + Q.sel);
  const SdNsdLayout N = sd_nsd_layout(Q, B, C, p->H, p->W);      // read only with nsd: the other entry points' workspaces end before it
  uint32_t* within = (uint32_t*)(ws + N.within);
  int32_t* bound = (int32_t*)(ws + N.bound);

  // 1. class maps + boxes
  if (fill_words_async(boxes, 0x7fffffffu, (size_t)B * C * 6, s) != hipSuccess) return set_error(MISEG_E_LAUNCH, "%s: fill", who);
  const int rc = sd_dispatch_label(p->label_dtype, [&](auto* tag) -> int {
    typedef typename std::remove_const<typename std::remove_pointer<decltype(tag)>::type>::type LT;
    int gx = cdiv(S, 256 * 8);
    if (gx > 2048) gx = 2048;
    if (p->logits)
      surface_classify_kernel<LT, true><<<dim3(gx, B), 256, 0, s>>>(p->logits, nullptr, (const LT*)p->label, C, p->H, p->W, S, pcls, lcls, boxes);
    else
      surface_classify_kernel<LT, false><<<dim3(gx, B), 256, 0, s>>>(nullptr, p->pred, (const LT*)p->label, C, p->H, p->W, S, pcls, lcls, boxes);
    MISEG_LAUNCH_CHECK("surface_classify");
    return MISEG_OK;
  });
  if (rc != MISEG_OK) return rc;

  // 2. the boxes decide the work: read them back (B x C x 24 bytes), pack the boxes into groups that fit the buffers
  std::vector<int> hbox((size_t)B * C * 6);
  if (hipMemcpyAsync(hbox.data(), boxes, hbox.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return set_error(MISEG_E_LAUNCH, "%s: box read-back", who);
  std::vector<int32_t> hindex((size_t)B * C, -1);
  std::vector<SdItem> hitems;
  std::vector<int> group_first;                  // index of the first item of every group
  int64_t gvol = 0, wl = 0, hb = 0, db = 0;
  for (int b = 0; b < B; ++b)
    for (int c = c0; c < C; ++c) {
      const int* bx = &hbox[((size_t)b * C + c) * 6];
      if (bx[0] == INT_MAX) continue;
      SdItem it;
      it.b = b; it.c = c; it.d0 = bx[0]; it.h0 = bx[1]; it.w0 = bx[2];
      it.nd = -bx[3] - bx[0] + 1; it.nh = -bx[4] - bx[1] + 1; it.nw = -bx[5] - bx[2] + 1;
      const int64_t vol = (int64_t)it.nd * it.nh * it.nw;
      if (group_first.empty() || gvol + vol > L.cap) {
        group_first.push_back((int)hitems.size());
        gvol = wl = hb = 0;
      }
      it.off = 2 * gvol; it.wline0 = wl; it.hblk0 = hb; it.dblk0 = db;
      gvol += vol;
      wl += (int64_t)it.nd * it.nh;
      hb += 2 * (int64_t)cdiv((int64_t)it.nd * it.nw, 256);
      db += 2 * (int64_t)cdiv((int64_t)it.nh * it.nw, 256);
      hindex[(size_t)b * C + c] = (int32_t)hitems.size();
      hitems.push_back(it);
    }
  if (hipMemcpyAsync(index, hindex.data(), hindex.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return set_error(MISEG_E_LAUNCH, "%s: index upload", who);
  if (!hitems.empty() && hipMemcpyAsync(items, hitems.data(), hitems.size() * sizeof(SdItem), hipMemcpyHostToDevice, s) != hipSuccess)
    return set_error(MISEG_E_LAUNCH, "%s: item upload", who);
  if (p->nsd && hipMemcpyAsync(bound, hbound.data(), hbound.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return set_error(MISEG_E_LAUNCH, "%s: bound upload", who);

  // 3. per group: W pass, H pass, D pass + gather (the groups reuse the buffers; stream order serialises them).  With hd the group's select
  // passes follow at once: they read the d^2 the D pass left in buf0, which the next group's W pass overwrites.
  group_first.push_back((int)hitems.size());
  if (p->hd && !hitems.empty() &&
      (fill_words_async(coarse, 0u, hitems.size() * 2 * SD_BINS, s) != hipSuccess || fill_words_async(fine, 0u, hitems.size() * 4 * SD_BINS, s) != hipSuccess))
    return set_error(MISEG_E_LAUNCH, "%s: table fill", who);
  for (size_t g = 0; g + 1 < group_first.size(); ++g) {
    const int f = group_first[g], n = group_first[g + 1] - f;
    const SdItem& last = hitems[f + n - 1];
    const int64_t nlines = last.wline0 + (int64_t)last.nd * last.nh;
    const int64_t hblocks = last.hblk0 + 2 * (int64_t)cdiv((int64_t)last.nd * last.nw, 256);
    const int64_t dblocks = last.dblk0 + 2 * (int64_t)cdiv((int64_t)last.nh * last.nw, 256) - hitems[f].dblk0;
    surface_edt_w_kernel<<<(unsigned)cdiv(nlines, 4), 256, 0, s>>>(items + f, n, nlines, pcls, lcls, p->H, p->W, S, edges, buf0);
    MISEG_LAUNCH_CHECK("surface_edt_w");
    surface_edt_h_kernel<<<(unsigned)hblocks, 256, 0, s>>>(items + f, n, buf0, buf1, stack);
    MISEG_LAUNCH_CHECK("surface_edt_h");
    if (!p->hd) {
      if (p->nsd)
        surface_edt_d_gather_nsd_kernel<<<(unsigned)dblocks, 256, 0, s>>>(items + f, n, hitems[f].dblk0, buf1, edges, stack, partials, bound, within);
      else
        surface_edt_d_gather_kernel<<<(unsigned)dblocks, 256, 0, s>>>(items + f, n, hitems[f].dblk0, buf1, edges, stack, partials);
      MISEG_LAUNCH_CHECK("surface_edt_d_gather");
      continue;
    }
    if (p->nsd)
      surface_edt_d_select_nsd_kernel<<<(unsigned)dblocks, 256, 0, s>>>(items + f, n, hitems[f].dblk0, buf1, edges, stack, partials, f, buf0, coarse, bound,
                                                                        within);
    else
      surface_edt_d_select_kernel<<<(unsigned)dblocks, 256, 0, s>>>(items + f, n, hitems[f].dblk0, buf1, edges, stack, partials, f, buf0, coarse);
    MISEG_LAUNCH_CHECK("surface_edt_d_select");
    surface_rank_kernel<<<dim3(n, 2), 256, 0, s>>>(coarse, f, p->percentile, sels);
    MISEG_LAUNCH_CHECK("surface_rank");
    int64_t maxvol = 0;
    for (int i = f; i < f + n; ++i) maxvol = std::max(maxvol, (int64_t)hitems[i].nd * hitems[i].nh * hitems[i].nw);
    const int64_t sx = std::min<int64_t>(cdiv(maxvol, 256 * 16 * 8), 512);  // >= 8 chunks of 16 voxels per thread before a workgroup pays for its table
    for (int i = 0; i < n; i += 16384) {                                     // grid.y holds 65535
      surface_select_kernel<<<dim3((unsigned)sx, 2 * std::min(n - i, 16384), 2), 256, 0, s>>>(items, f + i, sels, edges, buf0, fine);
      MISEG_LAUNCH_CHECK("surface_select");
    }
  }
  if (p->hd) {
    surface_finalize_hd_kernel<<<B * Cp, 256, 0, s>>>(index, items, partials, sels, fine, C, c0, p->symmetric, p->directed, p->percentile, p->asd, p->hd,
                                                      p->nsd ? within : nullptr, p->nsd);
    MISEG_LAUNCH_CHECK("surface_finalize_hd");
  } else {
    surface_finalize_kernel<<<cdiv((long)B * Cp, 64), 64, 0, s>>>(index, items, partials, B, C, c0, p->symmetric, p->asd, p->nsd ? within : nullptr, p->nsd);
    MISEG_LAUNCH_CHECK("surface_finalize");
  }
  // the host vectors above are the sources of the uploads: they must outlive them
  if (hipStreamSynchronize(s) != hipSuccess) return set_error(MISEG_E_LAUNCH, "%s: synchronize", who);
  return MISEG_OK;
}

}  // namespace
}  // namespace miseg

extern "C" int miseg_surface_distance(const miseg_surface_distance_params* p, miseg_stream_t s_) {
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_surface_distance_params), MISEG_E_BADARG, "surface_distance: struct_size %u != %zu",
                p ? p->struct_size : 0u, sizeof(miseg_surface_distance_params));
  MISEG_REQUIRE(p->asd, MISEG_E_BADARG, "surface_distance: null pointer");
  miseg_surface_dice_params q = {};
  q.struct_size = sizeof(q);
  q.logits = p->logits; q.pred = p->pred; q.label = p->label; q.label_dtype = p->label_dtype;
  q.B = p->B; q.C = p->C; q.D = p->D; q.H = p->H; q.W = p->W;
  q.include_background = p->include_background; q.symmetric = p->symmetric;
  q.workspace = p->workspace; q.asd = p->asd;          // hd and nsd stay NULL: the launch set of the ASD alone
  return surface_run(q, "surface_distance", (hipStream_t)s_);
}

extern "C" int miseg_surface_metrics(const miseg_surface_metrics_params* p, miseg_stream_t s_) {
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_surface_metrics_params), MISEG_E_BADARG, "surface_metrics: struct_size %u != %zu",
                p ? p->struct_size : 0u, sizeof(miseg_surface_metrics_params));
  MISEG_REQUIRE(p->asd || p->hd, MISEG_E_BADARG, "surface_metrics: null pointer");
  miseg_surface_dice_params q = {};
  q.struct_size = sizeof(q);
  q.logits = p->logits; q.pred = p->pred; q.label = p->label; q.label_dtype = p->label_dtype;
  q.B = p->B; q.C = p->C; q.D = p->D; q.H = p->H; q.W = p->W;
  q.include_background = p->include_background; q.symmetric = p->symmetric;
  q.workspace = p->workspace; q.asd = p->asd; q.hd = p->hd; q.percentile = p->percentile; q.directed = p->directed;      // nsd stays NULL
  return surface_run(q, "surface_metrics", (hipStream_t)s_);
}

extern "C" int miseg_surface_dice(const miseg_surface_dice_params* p, miseg_stream_t s_) {
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_surface_dice_params), MISEG_E_BADARG, "surface_dice: struct_size %u != %zu",
                p ? p->struct_size : 0u, sizeof(miseg_surface_dice_params));
  return surface_run(*p, "surface_dice", (hipStream_t)s_);
}
