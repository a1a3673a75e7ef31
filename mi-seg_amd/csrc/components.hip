// Connected-component post-processing on ONE union-find labelling core: keep-largest (MONAI 1.1.0 KeepLargestConnectedComponent with
// num_components = 1, restated) and fill-holes (MONAI 1.1.0 FillHoles restated; section 7.8).  The core labels the voxels
// a rule calls members, inside the box the rule gives, two neighbouring members (6 / 18 / 26 neighbourhood, never across a row, slice or sample
// end) being united iff the rule calls them the same.  Three passes, each a launch of its own (a kernel boundary is the only visibility point
// between workgroups this file relies on):
//   cc_local_kernel:    one workgroup per 8 x 8 x 64 (D x H x W) tile that meets the box: union-find in LDS over the tile's own voxels; every
//      member's parent becomes the smallest linear index of its in-tile component
//   cc_merge_kernel:    unions across tile faces, edges and corners with atomicMin on the int32 parent volume
//   cc_flatten_kernel:  every member's parent becomes its root
// Invariants: a voxel's parent is always a voxel of its own component with an index <= its own, and parents only ever decrease.  So every find
// terminates, a stale parent read is still a valid (older) ancestor, and when all unions are done the root of a component is its smallest
// linear index: the result does not depend on scheduling.  A union loops only on the value its atomicMin returned; finds merely pick the pair
// the next atomicMin is tried on (two voxels found under one ancestor are already connected by unions some thread has committed to).  No
// kernel waits for another workgroup.  Integer atomics only.
// Keep-largest (KeepRule: the applied-class voxels of the whole volume, the same iff of one class or the mode is joint; ONE labelling serves
// every class), six launches:
//   1. cc_classify_kernel: the given class map, or the first-maximum argmax of the logits, as a uint8 map (CC_NONE: no class); zeroes the
//      best table and the statistics
//   2. - 4. the core, which also counts: the local pass leaves each in-tile component's voxel count in size[] at its root (0 elsewhere), the
//      flatten adds every tile-level size to size[root] (one integer atomic per (tile, component), never one per voxel)
//   5. cc_select_kernel:   every root does one 64-bit atomicMax of (size << 32) | (0xFFFFFFFF - root) into best[b][group]: the largest
//      component, the smallest root among equals
//   6. cc_apply_kernel:    an applied voxel whose root is not its group's winner becomes 0; everything else keeps its value; statistics
// Fill-holes (FillRule) runs the core per label on the complement: see further down.
#include "common.h"
#include <type_traits>

namespace miseg {

namespace {

constexpr int CC_TD = 8, CC_TH = 8, CC_TW = 64, CC_TV = CC_TD * CC_TH * CC_TW, CC_PER = CC_TV / 256;
constexpr uint8_t CC_NONE = 255;         // map value of a voxel that belongs to no class
constexpr int CC_GROUPS = 64;            // best[b][CC_GROUPS]: one entry per class (independent) or entry 0 (joint)
constexpr int FH_BOX = 6;                // per (sample, label): min d, h, w, max d, h, w of the label's voxels (min > max: absent)
constexpr int FH_EMPTY_MIN = 0x7FFFFFFF;

struct CcGeom {
  int B, C, D, H, W, conn;
};

struct CcBox {
  int d0, h0, w0, nd, nh, nw;            // the domain of a labelling inside the volume; nd == 0: empty
};

__device__ __forceinline__ bool cc_is_applied(uint8_t m, uint64_t applied) { return m < 64 && ((applied >> m) & 1ull); }

// What the two labellings differ in.  member / same / box as above; off(): a map value no member has (the tile kernel's LDS map holds it
// wherever a voxel is not in the labelling); RUNS: the W-row run rule (cc_local_kernel); SIZES: component sizes are counted.
struct KeepRule {
  uint64_t applied;
  int joint;
  static constexpr bool RUNS = false;      // (would probably be faster switched on, per class in independent mode: a change of speed to be measured on its own)
  static constexpr bool SIZES = true;
  __device__ __forceinline__ bool member(uint8_t m) const { return cc_is_applied(m, applied); }
  __device__ __forceinline__ bool same(uint8_t a, uint8_t b) const { return joint || a == b; }
  __device__ __forceinline__ uint8_t off() const { return CC_NONE; }
  __device__ __forceinline__ CcBox box(int, const CcGeom& g) const { return {0, 0, 0, g.D, g.H, g.W}; }
};

// the voxels that are not `label`, all one kind, inside the label's bounding box grown by one voxel and clipped to the volume
struct FillRule {
  const int* boxes;                        // [B][CC_GROUPS][FH_BOX]
  int label;
  static constexpr bool RUNS = true;
  static constexpr bool SIZES = false;
  __device__ __forceinline__ bool member(uint8_t m) const { return m != (uint8_t)label; }
  __device__ __forceinline__ bool same(uint8_t, uint8_t) const { return true; }
  __device__ __forceinline__ uint8_t off() const { return (uint8_t)label; }
  __device__ __forceinline__ CcBox box(int b, const CcGeom& g) const {
    const int* q = boxes + ((int64_t)b * CC_GROUPS + label) * FH_BOX;
    CcBox x = {0, 0, 0, 0, 0, 0};
    const int d0 = q[0], h0 = q[1], w0 = q[2], d1 = q[3], h1 = q[4], w1 = q[5];
    if (d1 < d0) return x;
    x.d0 = max(d0 - 1, 0); x.h0 = max(h0 - 1, 0); x.w0 = max(w0 - 1, 0);
    x.nd = min(d1 + 1, g.D - 1) - x.d0 + 1; x.nh = min(h1 + 1, g.H - 1) - x.h0 + 1; x.nw = min(w1 + 1, g.W - 1) - x.w0 + 1;
    return x;
  }
};

// the half of the neighbourhood that precedes a voxel in raster order (each pair is visited once, from its later voxel)
__device__ __forceinline__ constexpr bool cc_backward(int dd, int dh, int dw) { return dd < 0 || (dd == 0 && (dh < 0 || (dh == 0 && dw < 0))); }

// voxel i of the box, in raster order
__device__ __forceinline__ void cc_voxel(const CcBox& x, int i, int& d, int& h, int& w) {
  w = x.w0 + i % x.nw;
  h = x.h0 + (i / x.nw) % x.nh;
  d = x.d0 + i / (x.nw * x.nh);
}

// The working uint8 map's value at voxel v of sample b.  I = float: the first-maximum argmax of logits [B][C][V]; uint8_t / int32_t: the class
// map [B][V]'s own value, CC_NONE where it lies outside [0, C)
template <class I> __device__ __forceinline__ uint8_t cc_map_value(const I* __restrict__ in, int b, int v, int C, int V) {
  if constexpr (std::is_same<I, float>::value) {
    const float* x = in + (int64_t)b * C * V + v;
    int arg = 0;
    float mx = x[0];
    for (int c = 1; c < C; ++c) {
      const float val = x[(int64_t)c * V];
      if (val > mx) { mx = val; arg = c; }        // strict: the FIRST maximum wins; a NaN after channel 0 never does (miseg_label_export)
    }
    return (uint8_t)arg;
  } else {
    const I val = in[(int64_t)b * V + v];
    return (uint32_t)val < (uint32_t)C ? (uint8_t)val : CC_NONE;
  }
}

// Keep-largest pass 1
template <class I>
__global__ void __launch_bounds__(256) cc_classify_kernel(const I* __restrict__ in, uint8_t* __restrict__ map, unsigned long long* __restrict__ best,
                                                          unsigned long long* __restrict__ stats, int B, int C, int V) {
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    for (int i = threadIdx.x; i < B * CC_GROUPS; i += 256) best[i] = 0ull;
    if (stats)
      for (int i = threadIdx.x; i < B * C * 3; i += 256) stats[i] = 0ull;
  }
  for (int b = blockIdx.y; b < B; b += gridDim.y)
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256)      // (64-bit: v + stride may pass 2^31)
      map[(int64_t)b * V + v_] = cc_map_value(in, b, (int)v_, C, V);
}

__device__ __forceinline__ int cc_lds_find(int* lab, int x) {
  int p;
  while ((p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = p;
  return x;
}

__device__ __forceinline__ void cc_lds_union(int* lab, int a, int b) {
  for (;;) {
    a = cc_lds_find(lab, a);
    b = cc_lds_find(lab, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b);
    if (old == a) return;        // a was a root and now hangs under b
    a = old;                     // a had a parent `old` already: that link may just have been replaced by b, so (old, b) is united next
  }
}

// The tile-local pass, over the tiles that meet the box.  `size` is written only under R::SIZES.
// The run rule (R::RUNS; it takes every two members for the same): a wave's 64 lanes are one W row of the tile, so every member starts under the
// first voxel of its run of members (one ballot), and two neighbouring rows are then united only at the first pair of each run they share.
template <class R>
__global__ void __launch_bounds__(256) cc_local_kernel(const uint8_t* __restrict__ map, int32_t* __restrict__ parent, uint32_t* __restrict__ size, CcGeom g, R rule) {
  __shared__ uint8_t cm[CC_TV];          // the map value of a member inside the box, else `off`
  __shared__ int lab[CC_TV];
  __shared__ int cnt[R::SIZES ? CC_TV : 1];      // (never referenced without SIZES: takes no LDS there)
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t V = (int64_t)g.D * g.H * g.W;
  const uint8_t off = rule.off();
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    const CcBox x = rule.box(b, g);
    if (x.nd == 0) continue;                                   // (uniform over the workgroup, as is the tile loop's bound)
    const int td0 = x.d0 / CC_TD, th0 = x.h0 / CC_TH, tw0 = x.w0 / CC_TW;
    const int ntd = (x.d0 + x.nd - 1) / CC_TD - td0 + 1, nth = (x.h0 + x.nh - 1) / CC_TH - th0 + 1, ntw = (x.w0 + x.nw - 1) / CC_TW - tw0 + 1;
    const int tiles = ntd * nth * ntw;                         // (each holds a voxel of the volume: below 2^31)
    const uint8_t* mb = map + (int64_t)b * V;
    int32_t* pb = parent + (int64_t)b * V;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
      const int w0 = (tw0 + t % ntw) * CC_TW, h0 = (th0 + (t / ntw) % nth) * CC_TH, d0 = (td0 + t / (ntw * nth)) * CC_TD;
#pragma unroll
      for (int k = 0; k < CC_PER; ++k) {
        const int l = tid + 256 * k, d = d0 + (l >> 9), h = h0 + ((l >> 6) & 7), w = w0 + (l & 63);
        uint8_t m = off;
        if (d >= x.d0 && d < x.d0 + x.nd && h >= x.h0 && h < x.h0 + x.nh && w >= x.w0 && w < x.w0 + x.nw) m = mb[((int64_t)d * g.H + h) * g.W + w];
        const bool p = rule.member(m);
        cm[l] = p ? m : off;
        if constexpr (R::RUNS) {
          // the rows are united along W before any union is tried (all voxels of a solid region queueing on their west neighbour otherwise)
          const unsigned long long gaps = ~__ballot(p) & ((1ull << lane) - 1ull);
          lab[l] = p && gaps ? l - lane + 64 - __clzll(gaps) : p ? l - lane : l;
        } else {
          lab[l] = l;
        }
        if constexpr (R::SIZES) cnt[l] = 0;
      }
      __syncthreads();
      // the three loops over a thread's 16 voxels that walk the forest stay rolled: unrolled, the 13 inlined union loops per voxel took the
      // keep-largest kernel to 218 VGPRs (2 waves per SIMD); rolled it needs 76 and the LDS bounds it at 4 workgroups per CU (the whole call
      // 5.55 -> 4.84 ms at 512x512x363)
#pragma unroll 1
      for (int k = 0; k < CC_PER; ++k) {
        const int l = tid + 256 * k, ld = l >> 9, lh = (l >> 6) & 7, lw = l & 63;
        const uint8_t m = cm[l];
        if (m == off) continue;
        [[maybe_unused]] bool west = false;
        if constexpr (R::RUNS) west = lw > 0 && cm[l - 1] != off;
#pragma unroll
        for (int dd = -1; dd <= 0; ++dd)
#pragma unroll
          for (int dh = -1; dh <= 1; ++dh)
#pragma unroll
            for (int dw = -1; dw <= 1; ++dw) {
              if (!cc_backward(dd, dh, dw) || (dd != 0) + (dh != 0) + (dw != 0) > g.conn) continue;
              if (R::RUNS && dd == 0 && dh == 0) continue;      // (the west neighbour: united from the start)
              if (ld + dd < 0 || lh + dh < 0 || lh + dh >= CC_TH || lw + dw < 0 || lw + dw >= CC_TW) continue;      // cc_merge_kernel's
              const int n = l + dd * (CC_TH * CC_TW) + dh * CC_TW + dw;
              const uint8_t mn = cm[n];
              if (mn == off || !rule.same(m, mn)) continue;
              if constexpr (R::RUNS) {
                // nearly every voxel is a member where the rule is on, so two neighbouring W rows meet along whole runs: only a run's first pair
                // unites them.  The pair one voxel to the west (same offset, also inside the tile) is some thread's, and each row's run is one set already.
                if (west && lw + dw > 0 && cm[n - 1] != off) continue;
              }
              cc_lds_union(lab, l, n);
            }
      }
      __syncthreads();
      // every union is done: a find now returns the final in-tile root (writing it back meanwhile only shortens other threads' walks)
#pragma unroll 1
      for (int k = 0; k < CC_PER; ++k) {
        const int l = tid + 256 * k;
        if (cm[l] != off) __hip_atomic_store(lab + l, cc_lds_find(lab, l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      __syncthreads();
      if constexpr (R::SIZES) {
        // in-tile component sizes: one LDS add per (wave, root) - the lanes of a wave are 64 voxels of one W row and mostly share a root
#pragma unroll 1
        for (int k = 0; k < CC_PER; ++k) {
          const int l = tid + 256 * k;
          const bool on = cm[l] != off;
          const int r = on ? lab[l] : -1;
          unsigned long long rem = __ballot(on);
          while (rem) {
            const int leader = __ffsll(rem) - 1;
            const int rl = __shfl(r, leader, 64);
            const unsigned long long same = __ballot(on && r == rl);
            if (lane == leader) atomicAdd(cnt + rl, (int)__popcll(same));
            rem &= ~same;
          }
        }
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < CC_PER; ++k) {
        const int l = tid + 256 * k;
        if (cm[l] == off) continue;      // (also every position outside the box); parent / size of other voxels are never read
        const int r = lab[l];
        const int64_t v = ((int64_t)(d0 + (l >> 9)) * g.H + (h0 + ((l >> 6) & 7))) * g.W + (w0 + (l & 63));
        const int64_t vr = ((int64_t)(d0 + (r >> 9)) * g.H + (h0 + ((r >> 6) & 7))) * g.W + (w0 + (r & 63));
        pb[v] = (int32_t)vr;
        if constexpr (R::SIZES) size[(int64_t)b * V + v] = r == l ? (uint32_t)cnt[l] : 0u;
      }
      __syncthreads();      // the next tile of this workgroup reuses the LDS arrays
    }
  }
}

// agent-scope loads: parents are being lowered by other workgroups' atomics while this walk runs (a value another XCD has since lowered is still
// an ancestor, see the invariants above).  A walk of more than one step hangs x directly under what it found, with atomicMin: a plain store
// could put an older ancestor over a lower parent a concurrent union has just set.  Without this the chains grow with every tile a component
// crosses and every border voxel walks them again (keep-largest's merge 2.96 -> 2.23 ms at 512 x 512 x 363).
__device__ __forceinline__ int cc_find(int32_t* parent, int x) {
  const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (p == x) return x;
  int r = p, q;
  while ((q = __hip_atomic_load(parent + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != r) r = q;
  if (r != p) atomicMin(parent + x, r);
  return r;
}

__device__ __forceinline__ void cc_union(int32_t* parent, int a, int b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

// The border merge: one thread per voxel of the box; only the voxels on a tile's border have a backward neighbour in another tile, and a
// neighbour outside the box is not in the labelling
template <class R>
__global__ void __launch_bounds__(256) cc_merge_kernel(const uint8_t* __restrict__ map, int32_t* __restrict__ parent, CcGeom g, R rule) {
  const int V = g.D * g.H * g.W, HW = g.H * g.W;
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    const CcBox x = rule.box(b, g);
    const int64_t nbox = (int64_t)x.nd * x.nh * x.nw;
    const uint8_t* mb = map + (int64_t)b * V;
    int32_t* pb = parent + (int64_t)b * V;
    for (int64_t i_ = (int64_t)blockIdx.x * 256 + threadIdx.x; i_ < nbox; i_ += (int64_t)gridDim.x * 256) {      // (64-bit: i + stride may pass 2^31)
      int d, h, w;
      cc_voxel(x, (int)i_, d, h, w);
      if ((d & (CC_TD - 1)) != 0 && (h & (CC_TH - 1)) != 0 && (h & (CC_TH - 1)) != CC_TH - 1 && (w & (CC_TW - 1)) != 0 && (w & (CC_TW - 1)) != CC_TW - 1) continue;
      const int v = (d * g.H + h) * g.W + w;
      const uint8_t m = mb[v];
      if (!rule.member(m)) continue;
      [[maybe_unused]] bool west = false;      // the voxel before v in its row: same tile, in the labelling
      if constexpr (R::RUNS) west = (w & (CC_TW - 1)) != 0 && w > x.w0 && rule.member(mb[v - 1]);
#pragma unroll
      for (int dd = -1; dd <= 0; ++dd)
#pragma unroll
        for (int dh = -1; dh <= 1; ++dh)
#pragma unroll
          for (int dw = -1; dw <= 1; ++dw) {
            if (!cc_backward(dd, dh, dw) || (dd != 0) + (dh != 0) + (dw != 0) > g.conn) continue;
            const int nd = d + dd, nh = h + dh, nw = w + dw;
            if (nd < x.d0 || nh < x.h0 || nh >= x.h0 + x.nh || nw < x.w0 || nw >= x.w0 + x.nw) continue;      // the box lies inside the volume: no wrap around a row, slice or sample end
            if ((nd >> 3) == (d >> 3) && (nh >> 3) == (h >> 3) && (nw >> 6) == (w >> 6)) continue;              // same tile: cc_local_kernel did it
            const int n = v + dd * HW + dh * g.W + dw;
            const uint8_t mn = mb[n];
            if (!rule.member(mn) || !rule.same(m, mn)) continue;
            if constexpr (R::RUNS) {
              // the run rule of cc_local_kernel across a D or H tile border (neither v nor n starts a W tile, so the border is not a W one):
              // v - 1 and n - 1 are the same kind of pair, visited by v - 1's thread, and each is tied to its row neighbour inside its own tile
              if (west && (nw & (CC_TW - 1)) != 0 && nw > x.w0 && rule.member(mb[n - 1])) continue;
            }
            cc_union(pb, v, n);
          }
    }
  }
}
static_assert(CC_TD == 8 && CC_TH == 8 && CC_TW == 64, "cc_local_kernel / cc_merge_kernel decode tile coordinates with these shifts");

// The flatten.  Concurrent shortening of other voxels' parents is harmless: old and new value are both ancestors.
template <class R>
__global__ void __launch_bounds__(256) cc_flatten_kernel(const uint8_t* __restrict__ map, int32_t* __restrict__ parent, uint32_t* __restrict__ size, CcGeom g, R rule) {
  const int V = g.D * g.H * g.W;
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    const CcBox x = rule.box(b, g);
    const int64_t nbox = (int64_t)x.nd * x.nh * x.nw;
    const uint8_t* mb = map + (int64_t)b * V;
    int32_t* pb = parent + (int64_t)b * V;
    for (int64_t i_ = (int64_t)blockIdx.x * 256 + threadIdx.x; i_ < nbox; i_ += (int64_t)gridDim.x * 256) {      // (64-bit: i + stride may pass 2^31)
      int v = x.d0 * g.H * g.W + (int)i_;        // a box of whole slices (the whole volume is one) is a contiguous run: nothing to decode
      if (x.nh != g.H || x.nw != g.W) {
        int d, h, w;
        cc_voxel(x, (int)i_, d, h, w);
        v = (d * g.H + h) * g.W + w;
      }
      if (!rule.member(mb[v])) continue;
      int r = v, p;
      while ((p = __hip_atomic_load(pb + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != r) r = p;
      if (r == v) continue;                      // a root keeps its own tile's count; the other tiles' counts are added to it below
      __hip_atomic_store(pb + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if constexpr (R::SIZES) {
        uint32_t* sb = size + (int64_t)b * V;
        const uint32_t s = sb[v];                // > 0: v led a tile-level component; v is no root, so nobody adds to size[v]
        if (s) atomicAdd(sb + r, s);
      }
    }
  }
}

// Keep-largest pass 5
__global__ void __launch_bounds__(256) cc_select_kernel(const uint8_t* __restrict__ map, const int32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                                                        unsigned long long* __restrict__ best, CcGeom g, KeepRule rule) {
  const int V = g.D * g.H * g.W;
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    const uint8_t* mb = map + (int64_t)b * V;
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256) {      // (64-bit: v + stride may pass 2^31)
      const int v = (int)v_;
      const uint8_t m = mb[v];
      if (!rule.member(m) || parent[(int64_t)b * V + v] != v) continue;
      const unsigned long long key = ((unsigned long long)size[(int64_t)b * V + v] << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)v);
      unsigned long long* slot = best + (int64_t)b * CC_GROUPS + (rule.joint ? 0 : m);
      // the table only grows: a root that is below what the slot already held cannot win, and thousands of one-voxel islands need not queue
      // on one address for that (keys differ between roots, so nothing is skipped that could have been the maximum): 1.01 -> 0.13 ms
      if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(slot, key);
    }
  }
}

// Keep-largest pass 6.  I: the given class map's element (values outside [0, C) are copied through), or float for "the map came from logits"
template <class I, class O>
__global__ void __launch_bounds__(256) cc_apply_kernel(const I* in, const uint8_t* __restrict__ map, const int32_t* __restrict__ parent,
                                                       const unsigned long long* __restrict__ best, O* out, unsigned long long* __restrict__ stats, CcGeom g,
                                                       KeepRule rule) {
  __shared__ int hist[CC_GROUPS * 3];
  const int V = g.D * g.H * g.W;
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    if (stats) {
      for (int i = threadIdx.x; i < CC_GROUPS * 3; i += 256) hist[i] = 0;
      __syncthreads();
    }
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256) {      // (64-bit: v + stride may pass 2^31)
      const int v = (int)v_;
      const int64_t i = (int64_t)b * V + v;
      const uint8_t m = map[i];
      if (m == CC_NONE) {
        if constexpr (!std::is_same<I, float>::value) out[i] = (O)in[i];
        continue;
      }
      bool keep = true, root = false;
      if (rule.member(m)) {
        const int r = parent[i];
        root = r == v;
        keep = (uint32_t)r == 0xFFFFFFFFu - (uint32_t)best[(int64_t)b * CC_GROUPS + (rule.joint ? 0 : m)];
      }
      out[i] = keep ? (O)m : (O)0;
      if (stats) {
        atomicAdd(hist + m * 3, 1);
        if (keep) atomicAdd(hist + m * 3 + 1, 1);
        if (root) atomicAdd(hist + m * 3 + 2, 1);
      }
    }
    if (stats) {
      __syncthreads();
      for (int i = threadIdx.x; i < g.C * 3; i += 256)
        if (hist[i]) atomicAdd(stats + (int64_t)b * g.C * 3 + i, (unsigned long long)hist[i]);
      __syncthreads();
    }
  }
}

// ---- Fill-holes ------------------------------------------------------------------------------------------------------------------------------------
// A hole of label L is a connected component of the complement of L that holds no voxel on a face of the volume: the labelling core under
// FillRule, and an "open" flag in place of a size.  A working uint8 map is updated in place label after label, in ascending order; per label,
// each step a launch of its own:
//   cc_local_kernel / cc_merge_kernel / cc_flatten_kernel: the three labelling passes over the passable (!= L) voxels
//   fh_flag_kernel:  the root r of every passable face voxel gets parent[r] = ~r (negative: open; many threads store the same value)
//   fh_fill_kernel:  a passable voxel whose root is not flagged becomes L
// Every pass is confined to L's bounding box grown by one voxel and clipped to the volume, all six faces of that box taken as open: a hole of L
// lies inside L's box, and a passable voxel outside the box reaches a volume face in a straight line away from it.  The boxes of all labels are
// taken once from the incoming map (fh_prepare_kernel): a later pass only ever loses voxels of its label to earlier fills, so its first box still
// holds them all.  An absent label has an empty box and its five launches return at once; the host reads nothing back.
__global__ void __launch_bounds__(256) fh_init_kernel(int* __restrict__ box, unsigned long long* __restrict__ stats, int B, int C) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < B * CC_GROUPS * FH_BOX; i += gridDim.x * 256) box[i] = (i % FH_BOX) < 3 ? FH_EMPTY_MIN : -1;
  if (stats)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B * C; i += gridDim.x * 256) stats[i] = 0ull;
}

// the working map and the bounding box of every applied label: a workgroup gathers its voxels' boxes in LDS - a read first, an atomic only
// where the box grows, which stops after a few voxels per label - and then does the same on the global table
template <class I>
__global__ void __launch_bounds__(256) fh_prepare_kernel(const I* __restrict__ in, uint8_t* __restrict__ work, int* __restrict__ box, CcGeom g, uint64_t applied) {
  __shared__ int lbox[CC_GROUPS * FH_BOX];
  const int V = g.D * g.H * g.W, HW = g.H * g.W;
  for (int i = threadIdx.x; i < CC_GROUPS * FH_BOX; i += 256) lbox[i] = (i % FH_BOX) < 3 ? FH_EMPTY_MIN : -1;
  __syncthreads();
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256) {      // (64-bit: v + stride may pass 2^31)
      const int v = (int)v_;
      const uint8_t m = cc_map_value(in, b, v, g.C, V);
      work[(int64_t)b * V + v] = m;
      if (!cc_is_applied(m, applied)) continue;
      const int c3[3] = {v / HW, (v / g.W) % g.H, v % g.W};
      int* q = lbox + m * FH_BOX;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (c3[k] < __hip_atomic_load(q + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMin(q + k, c3[k]);
        if (c3[k] > __hip_atomic_load(q + 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(q + 3 + k, c3[k]);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC_GROUPS * FH_BOX; i += 256) {
      const int val = lbox[i];
      int* q = box + (int64_t)b * CC_GROUPS * FH_BOX + i;
      if ((i % FH_BOX) < 3) {
        if (val < __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(q, val);
        lbox[i] = FH_EMPTY_MIN;
      } else {
        if (val > __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(q, val);
        lbox[i] = -1;
      }
    }
    __syncthreads();
  }
}

// the six faces of the box, one index range per pair of opposite faces (edges and corners come up more than once: the same store again).
// Every parent is a root after the flatten; a root r holds r, or ~r once it is flagged.
__global__ void __launch_bounds__(256) fh_flag_kernel(const uint8_t* __restrict__ work, int32_t* __restrict__ parent, CcGeom g, FillRule rule) {
  const int V = g.D * g.H * g.W;
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    const CcBox x = rule.box(b, g);
    const int64_t fd = (int64_t)x.nh * x.nw, fh = (int64_t)x.nd * x.nw, fw = (int64_t)x.nd * x.nh, faces = 2 * (fd + fh + fw);
    const uint8_t* mb = work + (int64_t)b * V;
    int32_t* pb = parent + (int64_t)b * V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < faces; i += (int64_t)gridDim.x * 256) {
      int d, h, w;
      if (i < 2 * fd) {
        const int j = (int)(i % fd);
        d = i < fd ? 0 : x.nd - 1; h = j / x.nw; w = j % x.nw;
      } else if (i < 2 * (fd + fh)) {
        const int64_t k = i - 2 * fd;
        const int j = (int)(k % fh);
        h = k < fh ? 0 : x.nh - 1; d = j / x.nw; w = j % x.nw;
      } else {
        const int64_t k = i - 2 * (fd + fh);
        const int j = (int)(k % fw);
        w = k < fw ? 0 : x.nw - 1; d = j / x.nh; h = j % x.nh;
      }
      const int v = ((x.d0 + d) * g.H + (x.h0 + h)) * g.W + (x.w0 + w);
      if (!rule.member(mb[v])) continue;
      const int r = __hip_atomic_load(pb + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r < 0) continue;                                                                        // v is a root, flagged already
      if (r != v && __hip_atomic_load(pb + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
      __hip_atomic_store(pb + r, ~r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void __launch_bounds__(256) fh_fill_kernel(uint8_t* __restrict__ work, const int32_t* __restrict__ parent, unsigned long long* __restrict__ stats,
                                                      CcGeom g, FillRule rule) {
  __shared__ unsigned int total;
  const int V = g.D * g.H * g.W;
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    const CcBox x = rule.box(b, g);
    const int64_t nbox = (int64_t)x.nd * x.nh * x.nw;
    if (nbox == 0) continue;                                   // (uniform over the workgroup)
    uint8_t* mb = work + (int64_t)b * V;
    const int32_t* pb = parent + (int64_t)b * V;
    if (threadIdx.x == 0) total = 0u;
    __syncthreads();
    unsigned int mine = 0;
    for (int64_t i_ = (int64_t)blockIdx.x * 256 + threadIdx.x; i_ < nbox; i_ += (int64_t)gridDim.x * 256) {
      int d, h, w;
      cc_voxel(x, (int)i_, d, h, w);
      const int v = (d * g.H + h) * g.W + w;
      if (!rule.member(mb[v])) continue;
      const int r = pb[v];
      if (r < 0 || pb[r] < 0) continue;                        // open
      mb[v] = (uint8_t)rule.label;
      ++mine;
    }
    if (stats) {
      if (mine) atomicAdd(&total, mine);
      __syncthreads();
      if (threadIdx.x == 0 && total) atomicAdd(stats + (int64_t)b * g.C + rule.label, (unsigned long long)total);
    }
    __syncthreads();
  }
}

// I: the given class map's element (a value outside [0, C) that no pass filled is copied through), or float for "the map came from logits"
template <class I, class O>
__global__ void __launch_bounds__(256) fh_output_kernel(const I* in, const uint8_t* __restrict__ work, O* out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint8_t m = work[i];
    if constexpr (!std::is_same<I, float>::value) {
      if (m == CC_NONE) { out[i] = (O)in[i]; continue; }
    }
    out[i] = (O)m;
  }
}

inline size_t cc_align(size_t n) { return (n + 255) & ~(size_t)255; }

// The argument checks both entry points share (each checks its own struct_size first); `applied` is cut to the C classes there are.
int cc_check_args(const char* name, const void* logits, const void* cls, int cls_bytes, const void* out, const void* workspace, int out_bytes, int B, int C,
                  int D, int H, int W, int connectivity, uint64_t* applied) {
  MISEG_REQUIRE((logits != nullptr) != (cls != nullptr), MISEG_E_BADARG, "%s: exactly one of logits / cls", name);
  MISEG_REQUIRE(!cls || cls_bytes == 1 || cls_bytes == 4, MISEG_E_BADARG, "%s: cls_bytes %d (1 or 4)", name, cls_bytes);
  MISEG_REQUIRE(out && workspace, MISEG_E_BADARG, "%s: null out / workspace pointer", name);
  MISEG_REQUIRE(out_bytes == 1 || out_bytes == 4, MISEG_E_BADARG, "%s: out_bytes %d (1 or 4)", name, out_bytes);
  MISEG_REQUIRE(C >= 1 && C <= 64, MISEG_E_BADARG, "%s: C %d (1..64)", name, C);
  MISEG_REQUIRE(connectivity >= 1 && connectivity <= 3, MISEG_E_BADARG, "%s: connectivity %d (1, 2 or 3)", name, connectivity);
  MISEG_REQUIRE(B >= 1 && D >= 1 && D <= 65535 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535, MISEG_E_BADARG,
                "%s: B %d (>= 1), volume %dx%dx%d (sides 1..65535)", name, B, D, H, W);
  const int64_t V64 = (int64_t)D * H * W;
  MISEG_REQUIRE(V64 < ((int64_t)1 << 31), MISEG_E_UNSUPPORTED, "%s: a sample of %lld voxels (below 2^31)", name, (long long)V64);
  if (C < 64) *applied &= (1ull << C) - 1;
  return MISEG_OK;
}

// f(in, out) with the call's input (the logits, or the class map in its width) and its output as typed pointers: the 3 x 2 element types
template <class F> void cc_typed(const void* logits, const void* cls, int cls_bytes, void* out, int out_bytes, F f) {
  auto with_in = [&](auto* in) {
    if (out_bytes == 1) f(in, (uint8_t*)out);
    else f(in, (int32_t*)out);
  };
  if (logits) with_in((const float*)logits);
  else if (cls_bytes == 1) with_in((const uint8_t*)cls);
  else with_in((const int32_t*)cls);
}

// the grid of the per-voxel passes over samples of V voxels, and that of the tile pass
inline dim3 cc_grid(int V, int B, int cap = 8192) { return dim3(cdiv(V, 256) < cap ? cdiv(V, 256) : cap, B < 65535 ? B : 65535); }
inline dim3 cc_tile_grid(const CcGeom& g) {
  const int64_t tiles = (int64_t)cdiv(g.D, CC_TD) * cdiv(g.H, CC_TH) * cdiv(g.W, CC_TW);
  return dim3((int)(tiles < (1 << 20) ? tiles : (1 << 20)), g.B < 65535 ? g.B : 65535);
}

}  // namespace

}  // namespace miseg

using namespace miseg;

extern "C" size_t miseg_keep_largest_workspace_bytes(int B, int D, int H, int W) {
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  const size_t n = (size_t)B * D * H * W;
  return 2 * cc_align(4 * n) + cc_align(n) + cc_align((size_t)B * CC_GROUPS * 8);
}

extern "C" int miseg_keep_largest(const miseg_keep_largest_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_keep_largest_params), MISEG_E_BADARG, "keep_largest: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_keep_largest_params));
  KeepRule rule = {p->applied, p->independent ? 0 : 1};
  if (const int e = cc_check_args("keep_largest", p->logits, p->cls, p->cls_bytes, p->out, p->workspace, p->out_bytes, p->B, p->C, p->D, p->H, p->W,
                                  p->connectivity, &rule.applied))
    return e;
  const CcGeom g = {p->B, p->C, p->D, p->H, p->W, p->connectivity};
  const int V = p->D * p->H * p->W;
  const size_t n = (size_t)p->B * V;
  char* ws = (char*)p->workspace;
  int32_t* parent = (int32_t*)ws;
  uint32_t* size = (uint32_t*)(ws + cc_align(4 * n));
  uint8_t* map = (uint8_t*)(ws + 2 * cc_align(4 * n));
  unsigned long long* best = (unsigned long long*)(ws + 2 * cc_align(4 * n) + cc_align(n));
  unsigned long long* stats = (unsigned long long*)p->stats;
  const dim3 grid = cc_grid(V, p->B);
  cc_typed(p->logits, p->cls, p->cls_bytes, p->out, p->out_bytes, [&](auto* in, auto*) { cc_classify_kernel<<<grid, 256, 0, s>>>(in, map, best, stats, g.B, g.C, V); });
  MISEG_LAUNCH_CHECK("keep_largest classify");
  cc_local_kernel<<<cc_tile_grid(g), 256, 0, s>>>(map, parent, size, g, rule);
  MISEG_LAUNCH_CHECK("keep_largest local");
  cc_merge_kernel<<<grid, 256, 0, s>>>(map, parent, g, rule);
  MISEG_LAUNCH_CHECK("keep_largest merge");
  cc_flatten_kernel<<<grid, 256, 0, s>>>(map, parent, size, g, rule);
  MISEG_LAUNCH_CHECK("keep_largest flatten");
  cc_select_kernel<<<grid, 256, 0, s>>>(map, parent, size, best, g, rule);
  MISEG_LAUNCH_CHECK("keep_largest select");
  cc_typed(p->logits, p->cls, p->cls_bytes, p->out, p->out_bytes,
           [&](auto* in, auto* out) { cc_apply_kernel<<<grid, 256, 0, s>>>(in, map, parent, best, out, stats, g, rule); });
  MISEG_LAUNCH_CHECK("keep_largest apply");
  return MISEG_OK;
}

extern "C" size_t miseg_fill_holes_workspace_bytes(int B, int D, int H, int W) {
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  const size_t n = (size_t)B * D * H * W;
  return cc_align(4 * n) + cc_align(n) + cc_align((size_t)B * CC_GROUPS * FH_BOX * 4);
}

extern "C" int miseg_fill_holes(const miseg_fill_holes_params* p, miseg_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  MISEG_REQUIRE(p && p->struct_size == sizeof(miseg_fill_holes_params), MISEG_E_BADARG, "fill_holes: struct_size %u != %zu", p ? p->struct_size : 0u,
                sizeof(miseg_fill_holes_params));
  uint64_t applied = p->applied;
  if (const int e = cc_check_args("fill_holes", p->logits, p->cls, p->cls_bytes, p->out, p->workspace, p->out_bytes, p->B, p->C, p->D, p->H, p->W,
                                  p->connectivity, &applied))
    return e;
  applied &= ~1ull;      // label 0 is the background: never applied
  const CcGeom g = {p->B, p->C, p->D, p->H, p->W, p->connectivity};
  const int V = p->D * p->H * p->W;
  const size_t n = (size_t)p->B * V;
  char* ws = (char*)p->workspace;
  int32_t* parent = (int32_t*)ws;
  uint8_t* work = (uint8_t*)(ws + cc_align(4 * n));
  int* box = (int*)(ws + cc_align(4 * n) + cc_align(n));
  unsigned long long* stats = (unsigned long long*)p->stats;
  const dim3 grid = cc_grid(V, p->B), tgrid = cc_tile_grid(g);
  const dim3 fgrid = cc_grid(V, p->B, 1024);      // (the faces of a box are few voxels; the grid-stride loops take whatever a grid does not)
  fh_init_kernel<<<cdiv(p->B * CC_GROUPS * FH_BOX, 256) < 1024 ? cdiv(p->B * CC_GROUPS * FH_BOX, 256) : 1024, 256, 0, s>>>(box, stats, p->B, p->C);
  MISEG_LAUNCH_CHECK("fill_holes init");
  cc_typed(p->logits, p->cls, p->cls_bytes, p->out, p->out_bytes, [&](auto* in, auto*) { fh_prepare_kernel<<<grid, 256, 0, s>>>(in, work, box, g, applied); });
  MISEG_LAUNCH_CHECK("fill_holes prepare");
  if (p->D > 1 && p->H > 1 && p->W > 1) {        // with a side of 1 every voxel lies on a face: nothing can be filled
    for (int L = 1; L < p->C; ++L) {
      if (!((applied >> L) & 1ull)) continue;
      const FillRule rule = {box, L};
      cc_local_kernel<<<tgrid, 256, 0, s>>>(work, parent, (uint32_t*)nullptr, g, rule);
      MISEG_LAUNCH_CHECK("fill_holes local");
      cc_merge_kernel<<<grid, 256, 0, s>>>(work, parent, g, rule);
      MISEG_LAUNCH_CHECK("fill_holes merge");
      cc_flatten_kernel<<<grid, 256, 0, s>>>(work, parent, (uint32_t*)nullptr, g, rule);
      MISEG_LAUNCH_CHECK("fill_holes flatten");
      fh_flag_kernel<<<fgrid, 256, 0, s>>>(work, parent, g, rule);
      MISEG_LAUNCH_CHECK("fill_holes flag");
      fh_fill_kernel<<<grid, 256, 0, s>>>(work, parent, stats, g, rule);
      MISEG_LAUNCH_CHECK("fill_holes fill");
    }
  }
  int64_t go = ((int64_t)n + 255) / 256;
  if (go > 8192 * 4) go = 8192 * 4;
  cc_typed(p->logits, p->cls, p->cls_bytes, p->out, p->out_bytes,
           [&](auto* in, auto* out) { fh_output_kernel<<<(int)go, 256, 0, s>>>(in, work, out, (int64_t)n); });
  MISEG_LAUNCH_CHECK("fill_holes output");
  return MISEG_OK;
}
