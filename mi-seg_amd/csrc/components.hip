// Keep-largest-connected-component post-processing (MONAI 1.1.0 KeepLargestConnectedComponent with num_components = 1, restated; DESIGN.md
// section 7.7): ONE union-find labelling of the class map serves every class.  Two neighbouring voxels (6 / 18 / 26 neighbourhood, never across a
// row, slice or sample end) are equivalent iff both belong to an applied class and either they have the same class or the mode is joint.
// Passes, each a launch of its own (a kernel boundary is the only visibility point between workgroups this file relies on):
//   1. cc_classify_kernel: the given class map, or the first-maximum argmax of the logits, as a uint8 map (CC_NONE: no class); zeroes the
//      best table and the statistics
//   2. cc_local_kernel:    one workgroup per 8 x 8 x 64 (D x H x W) tile: union-find in LDS over the tile's own voxels; every applied voxel's
//      parent becomes the smallest linear index of its in-tile component, whose voxel count goes to size[] at that index (0 elsewhere)
//   3. cc_merge_kernel:    unions across tile faces, edges and corners with atomicMin on the int32 parent volume
//   4. cc_flatten_kernel:  every applied voxel's parent becomes its root; every tile-level size is added to size[root] (one integer atomic per
//      (tile, component), never one per voxel)
//   5. cc_select_kernel:   every root does one 64-bit atomicMax of (size << 32) | (0xFFFFFFFF - root) into best[b][group]: the largest
//      component, the smallest root among equals
//   6. cc_apply_kernel:    an applied voxel whose root is not its group's winner becomes 0; everything else keeps its value; statistics
// Invariants: a voxel's parent is always a voxel of its own component with an index <= its own, and parents only ever decrease.  So every find
// terminates, a stale parent read is still a valid (older) ancestor, and when all unions are done the root of a component is its smallest
// linear index: the result does not depend on scheduling.  A union loops only on the value its atomicMin returned; finds merely pick the pair
// the next atomicMin is tried on (two voxels found under one ancestor are already connected by unions some thread has committed to).  No
// kernel waits for another workgroup.  Integer atomics only.
// The fill-holes filter further down (miseg_fill_holes) runs the same labelling per label on the complement.
#include "common.h"
#include <type_traits>

namespace miseg {

namespace {

constexpr int CC_TD = 8, CC_TH = 8, CC_TW = 64, CC_TV = CC_TD * CC_TH * CC_TW, CC_PER = CC_TV / 256;
constexpr uint8_t CC_NONE = 255;         // map value of a voxel that belongs to no class
constexpr int CC_GROUPS = 64;            // best[b][CC_GROUPS]: one entry per class (independent) or entry 0 (joint)

struct CcArgs {
  int B, C, D, H, W, joint, conn;
  uint64_t applied;
  int ntd, nth, ntw;
};

__device__ __forceinline__ bool cc_is_applied(uint8_t m, uint64_t applied) { return m < 64 && ((applied >> m) & 1ull); }
// the half of the neighbourhood that precedes a voxel in raster order (each pair is visited once, from its later voxel)
__device__ __forceinline__ constexpr bool cc_backward(int dd, int dh, int dw) { return dd < 0 || (dd == 0 && (dh < 0 || (dh == 0 && dw < 0))); }

template <class I> __device__ __forceinline__ uint8_t cc_class_of(I v, int C) { return (uint32_t)v < (uint32_t)C ? (uint8_t)v : CC_NONE; }

// Pass 1.  I = float: logits [B][C][V]; uint8_t / int32_t: a class map [B][V]
template <class I>
__global__ void __launch_bounds__(256) cc_classify_kernel(const I* __restrict__ in, uint8_t* __restrict__ map, unsigned long long* __restrict__ best,
                                                          unsigned long long* __restrict__ stats, int B, int C, int V) {
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    for (int i = threadIdx.x; i < B * CC_GROUPS; i += 256) best[i] = 0ull;
    if (stats)
      for (int i = threadIdx.x; i < B * C * 3; i += 256) stats[i] = 0ull;
  }
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256) {      // (64-bit: v + stride may pass 2^31)
      const int v = (int)v_;
      if constexpr (std::is_same<I, float>::value) {
        const float* x = in + (int64_t)b * C * V + v;
        int arg = 0;
        float mx = x[0];
        for (int c = 1; c < C; ++c) {
          const float val = x[(int64_t)c * V];
          if (val > mx) { mx = val; arg = c; }        // strict: the FIRST maximum wins; a NaN after channel 0 never does (miseg_label_export)
        }
        map[(int64_t)b * V + v] = (uint8_t)arg;
      } else {
        map[(int64_t)b * V + v] = cc_class_of(in[(int64_t)b * V + v], C);
      }
    }
  }
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

// Pass 2
__global__ void __launch_bounds__(256) cc_local_kernel(const uint8_t* __restrict__ map, int32_t* __restrict__ parent, uint32_t* __restrict__ size, CcArgs a) {
  __shared__ uint8_t cm[CC_TV];          // the class of an applied voxel inside the volume, else CC_NONE
  __shared__ int lab[CC_TV];
  __shared__ int cnt[CC_TV];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t V = (int64_t)a.D * a.H * a.W, tiles = (int64_t)a.ntd * a.nth * a.ntw, total = tiles * a.B;
  for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
    const int b = (int)(t / tiles), tt = (int)(t % tiles);
    const int w0 = (tt % a.ntw) * CC_TW, h0 = ((tt / a.ntw) % a.nth) * CC_TH, d0 = (tt / (a.ntw * a.nth)) * CC_TD;
    const uint8_t* mb = map + (int64_t)b * V;
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) {
      const int l = tid + 256 * k, d = d0 + (l >> 9), h = h0 + ((l >> 6) & 7), w = w0 + (l & 63);
      uint8_t m = CC_NONE;
      if (d < a.D && h < a.H && w < a.W) m = mb[((int64_t)d * a.H + h) * a.W + w];
      cm[l] = cc_is_applied(m, a.applied) ? m : CC_NONE;
      lab[l] = l;
      cnt[l] = 0;
    }
    __syncthreads();
    // the three loops over a thread's 16 voxels that walk the forest stay rolled: unrolled, the 13 inlined union loops per voxel took the kernel to
    // 218 VGPRs (2 waves per SIMD); rolled it needs 76 and the LDS bounds it at 4 workgroups per CU (the whole call 5.55 -> 4.84 ms at 512x512x363)
#pragma unroll 1
    for (int k = 0; k < CC_PER; ++k) {
      const int l = tid + 256 * k, ld = l >> 9, lh = (l >> 6) & 7, lw = l & 63;
      const uint8_t m = cm[l];
      if (m == CC_NONE) continue;
#pragma unroll
      for (int dd = -1; dd <= 0; ++dd)
#pragma unroll
        for (int dh = -1; dh <= 1; ++dh)
#pragma unroll
          for (int dw = -1; dw <= 1; ++dw) {
            if (!cc_backward(dd, dh, dw) || (dd != 0) + (dh != 0) + (dw != 0) > a.conn) continue;
            if (ld + dd < 0 || lh + dh < 0 || lh + dh >= CC_TH || lw + dw < 0 || lw + dw >= CC_TW) continue;      // cc_merge_kernel's
            const int n = l + dd * (CC_TH * CC_TW) + dh * CC_TW + dw;
            const uint8_t mn = cm[n];
            if (mn != CC_NONE && (a.joint || mn == m)) cc_lds_union(lab, l, n);
          }
    }
    __syncthreads();
    // every union is done: a find now returns the final in-tile root (writing it back meanwhile only shortens other threads' walks)
#pragma unroll 1
    for (int k = 0; k < CC_PER; ++k) {
      const int l = tid + 256 * k;
      if (cm[l] != CC_NONE) __hip_atomic_store(lab + l, cc_lds_find(lab, l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    // in-tile component sizes: one LDS add per (wave, root) - the lanes of a wave are 64 voxels of one W row and mostly share a root
#pragma unroll 1
    for (int k = 0; k < CC_PER; ++k) {
      const int l = tid + 256 * k;
      const bool on = cm[l] != CC_NONE;
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
    int32_t* pb = parent + (int64_t)b * V;
    uint32_t* sb = size + (int64_t)b * V;
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) {
      const int l = tid + 256 * k;
      if (cm[l] == CC_NONE) continue;      // (also every position outside the volume); parent / size of unapplied voxels are never read
      const int r = lab[l];
      const int64_t g = ((int64_t)(d0 + (l >> 9)) * a.H + (h0 + ((l >> 6) & 7))) * a.W + (w0 + (l & 63));
      const int64_t gr = ((int64_t)(d0 + (r >> 9)) * a.H + (h0 + ((r >> 6) & 7))) * a.W + (w0 + (r & 63));
      pb[g] = (int32_t)gr;
      sb[g] = r == l ? (uint32_t)cnt[l] : 0u;
    }
    __syncthreads();      // the next tile of this workgroup reuses the LDS arrays
  }
}

// agent-scope loads: parents are being lowered by other workgroups' atomics while this walk runs (a value another XCD has since lowered is still
// an ancestor, see the invariants above).  A walk of more than one step hangs x directly under what it found, with atomicMin: a plain store
// could put an older ancestor over a lower parent a concurrent union has just set.  Without this the chains grow with every tile a component
// crosses and every border voxel walks them again (cc_merge_kernel 2.96 -> 2.23 ms at 512 x 512 x 363).
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

// Pass 3: one thread per voxel; only the voxels on a tile's border have a backward neighbour in another tile
__global__ void __launch_bounds__(256) cc_merge_kernel(const uint8_t* __restrict__ map, int32_t* __restrict__ parent, CcArgs a) {
  const int V = a.D * a.H * a.W, HW = a.H * a.W;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const uint8_t* mb = map + (int64_t)b * V;
    int32_t* pb = parent + (int64_t)b * V;
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256) {      // (64-bit: v + stride may pass 2^31)
      const int v = (int)v_;
      const int w = v % a.W, h = (v / a.W) % a.H, d = v / HW;
      if ((d & (CC_TD - 1)) != 0 && (h & (CC_TH - 1)) != 0 && (h & (CC_TH - 1)) != CC_TH - 1 && (w & (CC_TW - 1)) != 0 && (w & (CC_TW - 1)) != CC_TW - 1) continue;
      const uint8_t m = mb[v];
      if (!cc_is_applied(m, a.applied)) continue;
#pragma unroll
      for (int dd = -1; dd <= 0; ++dd)
#pragma unroll
        for (int dh = -1; dh <= 1; ++dh)
#pragma unroll
          for (int dw = -1; dw <= 1; ++dw) {
            if (!cc_backward(dd, dh, dw) || (dd != 0) + (dh != 0) + (dw != 0) > a.conn) continue;
            const int nd = d + dd, nh = h + dh, nw = w + dw;
            if (nd < 0 || nh < 0 || nh >= a.H || nw < 0 || nw >= a.W) continue;                       // no wrap around a row, slice or sample end
            if ((nd >> 3) == (d >> 3) && (nh >> 3) == (h >> 3) && (nw >> 6) == (w >> 6)) continue;    // same tile: pass 2 did it
            const int n = v + dd * HW + dh * a.W + dw;
            const uint8_t mn = mb[n];
            if (cc_is_applied(mn, a.applied) && (a.joint || mn == m)) cc_union(pb, v, n);
          }
    }
  }
}
static_assert(CC_TD == 8 && CC_TH == 8 && CC_TW == 64, "cc_local_kernel / cc_merge_kernel decode tile coordinates with these shifts");

// Pass 4.  Concurrent shortening of other voxels' parents is harmless: old and new value are both ancestors.
__global__ void __launch_bounds__(256) cc_flatten_kernel(const uint8_t* __restrict__ map, int32_t* __restrict__ parent, uint32_t* __restrict__ size, CcArgs a) {
  const int V = a.D * a.H * a.W;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const uint8_t* mb = map + (int64_t)b * V;
    int32_t* pb = parent + (int64_t)b * V;
    uint32_t* sb = size + (int64_t)b * V;
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256) {      // (64-bit: v + stride may pass 2^31)
      const int v = (int)v_;
      if (!cc_is_applied(mb[v], a.applied)) continue;
      int r = v, p;
      while ((p = __hip_atomic_load(pb + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != r) r = p;
      if (r == v) continue;                      // a root keeps its own tile's count; the other tiles' counts are added to it below
      __hip_atomic_store(pb + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t s = sb[v];                  // > 0: v led a tile-level component; v is no root, so nobody adds to size[v]
      if (s) atomicAdd(sb + r, s);
    }
  }
}

// Pass 5
__global__ void __launch_bounds__(256) cc_select_kernel(const uint8_t* __restrict__ map, const int32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                                                        unsigned long long* __restrict__ best, CcArgs a) {
  const int V = a.D * a.H * a.W;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const uint8_t* mb = map + (int64_t)b * V;
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256) {      // (64-bit: v + stride may pass 2^31)
      const int v = (int)v_;
      const uint8_t m = mb[v];
      if (!cc_is_applied(m, a.applied) || parent[(int64_t)b * V + v] != v) continue;
      const unsigned long long key = ((unsigned long long)size[(int64_t)b * V + v] << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)v);
      unsigned long long* slot = best + (int64_t)b * CC_GROUPS + (a.joint ? 0 : m);
      // the table only grows: a root that is below what the slot already held cannot win, and thousands of one-voxel islands need not queue
      // on one address for that (keys differ between roots, so nothing is skipped that could have been the maximum): 1.01 -> 0.13 ms
      if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(slot, key);
    }
  }
}

// Pass 6.  I: the given class map's element (values outside [0, C) are copied through), or float for "the map came from logits"
template <class I, class O>
__global__ void __launch_bounds__(256) cc_apply_kernel(const I* in, const uint8_t* __restrict__ map, const int32_t* __restrict__ parent,
                                                       const unsigned long long* __restrict__ best, O* out, unsigned long long* __restrict__ stats, CcArgs a) {
  __shared__ int hist[CC_GROUPS * 3];
  const int V = a.D * a.H * a.W;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    if (stats) {
      for (int i = threadIdx.x; i < CC_GROUPS * 3; i += 256) hist[i] = 0;
      __syncthreads();
    }
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256) {      // (64-bit: v + stride may pass 2^31)
      const int v = (int)v_;
      const int64_t g = (int64_t)b * V + v;
      const uint8_t m = map[g];
      if (m == CC_NONE) {
        if constexpr (!std::is_same<I, float>::value) out[g] = (O)in[g];
        continue;
      }
      bool keep = true, root = false;
      if (cc_is_applied(m, a.applied)) {
        const int r = parent[g];
        root = r == v;
        keep = (uint32_t)r == 0xFFFFFFFFu - (uint32_t)best[(int64_t)b * CC_GROUPS + (a.joint ? 0 : m)];
      }
      out[g] = keep ? (O)m : (O)0;
      if (stats) {
        atomicAdd(hist + m * 3, 1);
        if (keep) atomicAdd(hist + m * 3 + 1, 1);
        if (root) atomicAdd(hist + m * 3 + 2, 1);
      }
    }
    if (stats) {
      __syncthreads();
      for (int i = threadIdx.x; i < a.C * 3; i += 256)
        if (hist[i]) atomicAdd(stats + (int64_t)b * a.C * 3 + i, (unsigned long long)hist[i]);
      __syncthreads();
    }
  }
}

// ---- Fill-holes (MONAI 1.1.0 FillHoles restated) --------------------------------------------------------------------------
// A hole of label L is a connected component of the complement of L that holds no voxel on a face of the volume.  The labelling above with
// another equivalence rule (two neighbouring voxels are equivalent iff neither is L) and an "open" flag in place of a size.  A working uint8
// map is updated in place label after label, in ascending order; per label, each step a launch of its own:
//   fh_local_kernel / fh_merge_kernel / fh_flatten_kernel: the three labelling passes over the passable (!= L) voxels
//   fh_flag_kernel:  the root r of every passable face voxel gets parent[r] = ~r (negative: open; many threads store the same value)
//   fh_fill_kernel:  a passable voxel whose root is not flagged becomes L
// Every pass is confined to L's bounding box grown by one voxel and clipped to the volume, all six faces of that box taken as open: a hole of L
// lies inside L's box, and a passable voxel outside the box reaches a volume face in a straight line away from it.  The boxes of all labels are
// taken once from the incoming map (fh_prepare_kernel): a later pass only ever loses voxels of its label to earlier fills, so its first box still
// holds them all.  An absent label has an empty box and its five launches return at once; the host reads nothing back.
constexpr int FH_BOX = 6;                // per (sample, label): min d, h, w, max d, h, w of the label's voxels (min > max: absent)
constexpr int FH_EMPTY_MIN = 0x7FFFFFFF;

struct FhArgs {
  int B, C, D, H, W, conn, label;
  uint64_t applied;
};

struct FhBox {
  int d0, h0, w0, nd, nh, nw;            // the grown, clipped box; nd == 0: the label is absent
};

__device__ __forceinline__ FhBox fh_box(const int* __restrict__ box, int b, const FhArgs& a) {
  const int* q = box + ((int64_t)b * CC_GROUPS + a.label) * FH_BOX;
  FhBox x = {0, 0, 0, 0, 0, 0};
  const int d0 = q[0], h0 = q[1], w0 = q[2], d1 = q[3], h1 = q[4], w1 = q[5];
  if (d1 < d0) return x;
  x.d0 = max(d0 - 1, 0); x.h0 = max(h0 - 1, 0); x.w0 = max(w0 - 1, 0);
  x.nd = min(d1 + 1, a.D - 1) - x.d0 + 1; x.nh = min(h1 + 1, a.H - 1) - x.h0 + 1; x.nw = min(w1 + 1, a.W - 1) - x.w0 + 1;
  return x;
}

__global__ void __launch_bounds__(256) fh_init_kernel(int* __restrict__ box, unsigned long long* __restrict__ stats, int B, int C) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < B * CC_GROUPS * FH_BOX; i += gridDim.x * 256) box[i] = (i % FH_BOX) < 3 ? FH_EMPTY_MIN : -1;
  if (stats)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B * C; i += gridDim.x * 256) stats[i] = 0ull;
}

// the working map (cc_classify_kernel's rule) and the bounding box of every applied label: a workgroup gathers its voxels' boxes in LDS - a
// read first, an atomic only where the box grows, which stops after a few voxels per label - and then does the same on the global table
template <class I>
__global__ void __launch_bounds__(256) fh_prepare_kernel(const I* __restrict__ in, uint8_t* __restrict__ work, int* __restrict__ box, FhArgs a) {
  __shared__ int lbox[CC_GROUPS * FH_BOX];
  const int V = a.D * a.H * a.W, HW = a.H * a.W;
  for (int i = threadIdx.x; i < CC_GROUPS * FH_BOX; i += 256) lbox[i] = (i % FH_BOX) < 3 ? FH_EMPTY_MIN : -1;
  __syncthreads();
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    for (int64_t v_ = (int64_t)blockIdx.x * 256 + threadIdx.x; v_ < V; v_ += (int64_t)gridDim.x * 256) {      // (64-bit: v + stride may pass 2^31)
      const int v = (int)v_;
      uint8_t m;
      if constexpr (std::is_same<I, float>::value) {
        const float* x = in + (int64_t)b * a.C * V + v;
        int arg = 0;
        float mx = x[0];
        for (int c = 1; c < a.C; ++c) {
          const float val = x[(int64_t)c * V];
          if (val > mx) { mx = val; arg = c; }        // strict: the FIRST maximum wins (cc_classify_kernel)
        }
        m = (uint8_t)arg;
      } else {
        m = cc_class_of(in[(int64_t)b * V + v], a.C);
      }
      work[(int64_t)b * V + v] = m;
      if (!cc_is_applied(m, a.applied)) continue;
      const int c3[3] = {v / HW, (v / a.W) % a.H, v % a.W};
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
      int* g = box + (int64_t)b * CC_GROUPS * FH_BOX + i;
      if ((i % FH_BOX) < 3) {
        if (val < __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(g, val);
        lbox[i] = FH_EMPTY_MIN;
      } else {
        if (val > __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(g, val);
        lbox[i] = -1;
      }
    }
    __syncthreads();
  }
}

// cc_local_kernel over the tiles that meet the box; a voxel is in the labelling iff it lies in the box and is not the label
__global__ void __launch_bounds__(256) fh_local_kernel(const uint8_t* __restrict__ work, int32_t* __restrict__ parent, const int* __restrict__ box, FhArgs a) {
  __shared__ uint8_t on[CC_TV];
  __shared__ int lab[CC_TV];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t V = (int64_t)a.D * a.H * a.W;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const FhBox x = fh_box(box, b, a);
    if (x.nd == 0) continue;                                   // (uniform over the workgroup, as is the tile loop's bound)
    const int td0 = x.d0 / CC_TD, th0 = x.h0 / CC_TH, tw0 = x.w0 / CC_TW;
    const int ntd = (x.d0 + x.nd - 1) / CC_TD - td0 + 1, nth = (x.h0 + x.nh - 1) / CC_TH - th0 + 1, ntw = (x.w0 + x.nw - 1) / CC_TW - tw0 + 1;
    const int tiles = ntd * nth * ntw;                         // (each holds a voxel of the volume: below 2^31)
    const uint8_t* mb = work + (int64_t)b * V;
    int32_t* pb = parent + (int64_t)b * V;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
      const int w0 = (tw0 + t % ntw) * CC_TW, h0 = (th0 + (t / ntw) % nth) * CC_TH, d0 = (td0 + t / (ntw * nth)) * CC_TD;
#pragma unroll
      for (int k = 0; k < CC_PER; ++k) {
        const int l = tid + 256 * k, d = d0 + (l >> 9), h = h0 + ((l >> 6) & 7), w = w0 + (l & 63);
        bool p = false;
        if (d >= x.d0 && d < x.d0 + x.nd && h >= x.h0 && h < x.h0 + x.nh && w >= x.w0 && w < x.w0 + x.nw) p = mb[((int64_t)d * a.H + h) * a.W + w] != (uint8_t)a.label;
        on[l] = p;
        // a wave's 64 lanes are one W row of the tile: every voxel starts under the first voxel of its run of passable voxels, so the rows
        // are united along W before any union is tried (all voxels of a solid region queueing on their west neighbour otherwise)
        const unsigned long long gaps = ~__ballot(p) & ((1ull << lane) - 1ull);
        lab[l] = p && gaps ? l - lane + 64 - __clzll(gaps) : p ? l - lane : l;
      }
      __syncthreads();
#pragma unroll 1
      for (int k = 0; k < CC_PER; ++k) {                       // rolled, as in cc_local_kernel
        const int l = tid + 256 * k, ld = l >> 9, lh = (l >> 6) & 7, lw = l & 63;
        if (!on[l]) continue;
        const bool west = lw > 0 && on[l - 1];
#pragma unroll
        for (int dd = -1; dd <= 0; ++dd)
#pragma unroll
          for (int dh = -1; dh <= 1; ++dh)
#pragma unroll
            for (int dw = -1; dw <= 1; ++dw) {
              if (!cc_backward(dd, dh, dw) || (dd != 0) + (dh != 0) + (dw != 0) > a.conn) continue;
              if (ld + dd < 0 || lh + dh < 0 || lh + dh >= CC_TH || lw + dw < 0 || lw + dw >= CC_TW) continue;      // fh_merge_kernel's
              const int n = l + dd * (CC_TH * CC_TW) + dh * CC_TW + dw;
              if ((dd == 0 && dh == 0) || !on[n]) continue;      // (the west neighbour: united from the start)
              // nearly every voxel is passable here, so two neighbouring W rows meet along whole runs: only a run's first pair unites them.
              // The pair one voxel to the west (same offset, also inside the tile) is some thread's, and each row's run is one set already.
              if (west && lw + dw > 0 && on[n - 1]) continue;
              cc_lds_union(lab, l, n);
            }
      }
      __syncthreads();
#pragma unroll 1
      for (int k = 0; k < CC_PER; ++k) {
        const int l = tid + 256 * k;
        if (on[l]) __hip_atomic_store(lab + l, cc_lds_find(lab, l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < CC_PER; ++k) {
        const int l = tid + 256 * k;
        if (!on[l]) continue;
        const int r = lab[l];
        const int64_t g = ((int64_t)(d0 + (l >> 9)) * a.H + (h0 + ((l >> 6) & 7))) * a.W + (w0 + (l & 63));
        const int64_t gr = ((int64_t)(d0 + (r >> 9)) * a.H + (h0 + ((r >> 6) & 7))) * a.W + (w0 + (r & 63));
        pb[g] = (int32_t)gr;
      }
      __syncthreads();      // the next tile of this workgroup reuses the LDS arrays
    }
  }
}

// voxel i of the box, in raster order
__device__ __forceinline__ void fh_voxel(const FhBox& x, int i, int& d, int& h, int& w) {
  w = x.w0 + i % x.nw;
  h = x.h0 + (i / x.nw) % x.nh;
  d = x.d0 + i / (x.nw * x.nh);
}

// cc_merge_kernel over the box: a neighbour outside the box is not in the labelling
__global__ void __launch_bounds__(256) fh_merge_kernel(const uint8_t* __restrict__ work, int32_t* __restrict__ parent, const int* __restrict__ box, FhArgs a) {
  const int V = a.D * a.H * a.W, HW = a.H * a.W;
  const uint8_t L = (uint8_t)a.label;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const FhBox x = fh_box(box, b, a);
    const int64_t nbox = (int64_t)x.nd * x.nh * x.nw;
    const uint8_t* mb = work + (int64_t)b * V;
    int32_t* pb = parent + (int64_t)b * V;
    for (int64_t i_ = (int64_t)blockIdx.x * 256 + threadIdx.x; i_ < nbox; i_ += (int64_t)gridDim.x * 256) {
      int d, h, w;
      fh_voxel(x, (int)i_, d, h, w);
      if ((d & (CC_TD - 1)) != 0 && (h & (CC_TH - 1)) != 0 && (h & (CC_TH - 1)) != CC_TH - 1 && (w & (CC_TW - 1)) != 0 && (w & (CC_TW - 1)) != CC_TW - 1) continue;
      const int v = (d * a.H + h) * a.W + w;
      if (mb[v] == L) continue;
      const bool west = (w & (CC_TW - 1)) != 0 && w > x.w0 && mb[v - 1] != L;      // the voxel before v in its row: same tile, in the labelling
#pragma unroll
      for (int dd = -1; dd <= 0; ++dd)
#pragma unroll
        for (int dh = -1; dh <= 1; ++dh)
#pragma unroll
          for (int dw = -1; dw <= 1; ++dw) {
            if (!cc_backward(dd, dh, dw) || (dd != 0) + (dh != 0) + (dw != 0) > a.conn) continue;
            const int nd = d + dd, nh = h + dh, nw = w + dw;
            if (nd < x.d0 || nh < x.h0 || nh >= x.h0 + x.nh || nw < x.w0 || nw >= x.w0 + x.nw) continue;      // the box lies inside the volume: no wrap either
            if ((nd >> 3) == (d >> 3) && (nh >> 3) == (h >> 3) && (nw >> 6) == (w >> 6)) continue;              // same tile: fh_local_kernel did it
            const int n = v + dd * HW + dh * a.W + dw;
            if (mb[n] == L) continue;
            // the run rule of fh_local_kernel across a D or H tile border (neither v nor n starts a W tile, so the border is not a W one):
            // v - 1 and n - 1 are the same kind of pair, visited by v - 1's thread, and each is tied to its row neighbour inside its own tile
            if (west && (nw & (CC_TW - 1)) != 0 && nw > x.w0 && mb[n - 1] != L) continue;
            cc_union(pb, v, n);
          }
    }
  }
}

__global__ void __launch_bounds__(256) fh_flatten_kernel(const uint8_t* __restrict__ work, int32_t* __restrict__ parent, const int* __restrict__ box, FhArgs a) {
  const int V = a.D * a.H * a.W;
  const uint8_t L = (uint8_t)a.label;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const FhBox x = fh_box(box, b, a);
    const int64_t nbox = (int64_t)x.nd * x.nh * x.nw;
    const uint8_t* mb = work + (int64_t)b * V;
    int32_t* pb = parent + (int64_t)b * V;
    for (int64_t i_ = (int64_t)blockIdx.x * 256 + threadIdx.x; i_ < nbox; i_ += (int64_t)gridDim.x * 256) {
      int d, h, w;
      fh_voxel(x, (int)i_, d, h, w);
      const int v = (d * a.H + h) * a.W + w;
      if (mb[v] == L) continue;
      int r = v, p;
      while ((p = __hip_atomic_load(pb + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != r) r = p;
      if (r != v) __hip_atomic_store(pb + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// the six faces of the box, one index range per pair of opposite faces (edges and corners come up more than once: the same store again).
// Every parent is a root after the flatten; a root r holds r, or ~r once it is flagged.
__global__ void __launch_bounds__(256) fh_flag_kernel(const uint8_t* __restrict__ work, int32_t* __restrict__ parent, const int* __restrict__ box, FhArgs a) {
  const int V = a.D * a.H * a.W;
  const uint8_t L = (uint8_t)a.label;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const FhBox x = fh_box(box, b, a);
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
      const int v = ((x.d0 + d) * a.H + (x.h0 + h)) * a.W + (x.w0 + w);
      if (mb[v] == L) continue;
      const int r = __hip_atomic_load(pb + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r < 0) continue;                                                                        // v is a root, flagged already
      if (r != v && __hip_atomic_load(pb + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
      __hip_atomic_store(pb + r, ~r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void __launch_bounds__(256) fh_fill_kernel(uint8_t* __restrict__ work, const int32_t* __restrict__ parent, const int* __restrict__ box,
                                                      unsigned long long* __restrict__ stats, FhArgs a) {
  __shared__ unsigned int total;
  const int V = a.D * a.H * a.W;
  const uint8_t L = (uint8_t)a.label;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const FhBox x = fh_box(box, b, a);
    const int64_t nbox = (int64_t)x.nd * x.nh * x.nw;
    if (nbox == 0) continue;                                   // (uniform over the workgroup)
    uint8_t* mb = work + (int64_t)b * V;
    const int32_t* pb = parent + (int64_t)b * V;
    if (threadIdx.x == 0) total = 0u;
    __syncthreads();
    unsigned int mine = 0;
    for (int64_t i_ = (int64_t)blockIdx.x * 256 + threadIdx.x; i_ < nbox; i_ += (int64_t)gridDim.x * 256) {
      int d, h, w;
      fh_voxel(x, (int)i_, d, h, w);
      const int v = (d * a.H + h) * a.W + w;
      if (mb[v] == L) continue;
      const int r = pb[v];
      if (r < 0 || pb[r] < 0) continue;                        // open
      mb[v] = L;
      ++mine;
    }
    if (stats) {
      if (mine) atomicAdd(&total, mine);
      __syncthreads();
      if (threadIdx.x == 0 && total) atomicAdd(stats + (int64_t)b * a.C + a.label, (unsigned long long)total);
    }
    __syncthreads();
  }
}

// I: the given class map's element (a value outside [0, C) that no pass filled is copied through), or float for "the map came from logits"
template <class I, class O>
__global__ void __launch_bounds__(256) fh_output_kernel(const I* in, const uint8_t* __restrict__ work, O* out, int64_t n) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
    const uint8_t m = work[g];
    if constexpr (!std::is_same<I, float>::value) {
      if (m == CC_NONE) { out[g] = (O)in[g]; continue; }
    }
    out[g] = (O)m;
  }
}

inline size_t cc_align(size_t n) { return (n + 255) & ~(size_t)255; }

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
  MISEG_REQUIRE((p->logits != nullptr) != (p->cls != nullptr), MISEG_E_BADARG, "keep_largest: exactly one of logits / cls");
  MISEG_REQUIRE(!p->cls || p->cls_bytes == 1 || p->cls_bytes == 4, MISEG_E_BADARG, "keep_largest: cls_bytes %d (1 or 4)", p->cls_bytes);
  MISEG_REQUIRE(p->out && p->workspace, MISEG_E_BADARG, "keep_largest: null out / workspace pointer");
  MISEG_REQUIRE(p->out_bytes == 1 || p->out_bytes == 4, MISEG_E_BADARG, "keep_largest: out_bytes %d (1 or 4)", p->out_bytes);
  MISEG_REQUIRE(p->C >= 1 && p->C <= 64, MISEG_E_BADARG, "keep_largest: C %d (1..64)", p->C);
  MISEG_REQUIRE(p->connectivity >= 1 && p->connectivity <= 3, MISEG_E_BADARG, "keep_largest: connectivity %d (1, 2 or 3)", p->connectivity);
  MISEG_REQUIRE(p->B >= 1 && p->D >= 1 && p->D <= 65535 && p->H >= 1 && p->H <= 65535 && p->W >= 1 && p->W <= 65535, MISEG_E_BADARG,
                "keep_largest: B %d (>= 1), volume %dx%dx%d (sides 1..65535)", p->B, p->D, p->H, p->W);
  const int64_t V64 = (int64_t)p->D * p->H * p->W;
  MISEG_REQUIRE(V64 < ((int64_t)1 << 31), MISEG_E_UNSUPPORTED, "keep_largest: a sample of %lld voxels (below 2^31)", (long long)V64);
  const int V = (int)V64;
  const size_t n = (size_t)p->B * V;
  char* ws = (char*)p->workspace;
  int32_t* parent = (int32_t*)ws;
  uint32_t* size = (uint32_t*)(ws + cc_align(4 * n));
  uint8_t* map = (uint8_t*)(ws + 2 * cc_align(4 * n));
  unsigned long long* best = (unsigned long long*)(ws + 2 * cc_align(4 * n) + cc_align(n));
  unsigned long long* stats = (unsigned long long*)p->stats;
  CcArgs a;
  a.B = p->B; a.C = p->C; a.D = p->D; a.H = p->H; a.W = p->W; a.joint = p->independent ? 0 : 1; a.conn = p->connectivity;
  a.applied = p->C == 64 ? p->applied : p->applied & ((1ull << p->C) - 1);
  a.ntd = cdiv(p->D, CC_TD); a.nth = cdiv(p->H, CC_TH); a.ntw = cdiv(p->W, CC_TW);
  int gx = cdiv(V, 256);
  if (gx > 8192) gx = 8192;
  const dim3 grid(gx, p->B < 65535 ? p->B : 65535);
  if (p->logits) cc_classify_kernel<float><<<grid, 256, 0, s>>>(p->logits, map, best, stats, p->B, p->C, V);
  else if (p->cls_bytes == 1) cc_classify_kernel<uint8_t><<<grid, 256, 0, s>>>((const uint8_t*)p->cls, map, best, stats, p->B, p->C, V);
  else cc_classify_kernel<int32_t><<<grid, 256, 0, s>>>((const int32_t*)p->cls, map, best, stats, p->B, p->C, V);
  MISEG_LAUNCH_CHECK("keep_largest classify");
  const int64_t tiles = (int64_t)a.ntd * a.nth * a.ntw * p->B;
  cc_local_kernel<<<(int)(tiles < (1 << 20) ? tiles : (1 << 20)), 256, 0, s>>>(map, parent, size, a);
  MISEG_LAUNCH_CHECK("keep_largest local");
  cc_merge_kernel<<<grid, 256, 0, s>>>(map, parent, a);
  MISEG_LAUNCH_CHECK("keep_largest merge");
  cc_flatten_kernel<<<grid, 256, 0, s>>>(map, parent, size, a);
  MISEG_LAUNCH_CHECK("keep_largest flatten");
  cc_select_kernel<<<grid, 256, 0, s>>>(map, parent, size, best, a);
  MISEG_LAUNCH_CHECK("keep_largest select");
  const bool o1 = p->out_bytes == 1;
  if (p->logits) {
    if (o1) cc_apply_kernel<float, uint8_t><<<grid, 256, 0, s>>>(p->logits, map, parent, best, (uint8_t*)p->out, stats, a);
    else cc_apply_kernel<float, int32_t><<<grid, 256, 0, s>>>(p->logits, map, parent, best, (int32_t*)p->out, stats, a);
  } else if (p->cls_bytes == 1) {
    if (o1) cc_apply_kernel<uint8_t, uint8_t><<<grid, 256, 0, s>>>((const uint8_t*)p->cls, map, parent, best, (uint8_t*)p->out, stats, a);
    else cc_apply_kernel<uint8_t, int32_t><<<grid, 256, 0, s>>>((const uint8_t*)p->cls, map, parent, best, (int32_t*)p->out, stats, a);
  } else {
    if (o1) cc_apply_kernel<int32_t, uint8_t><<<grid, 256, 0, s>>>((const int32_t*)p->cls, map, parent, best, (uint8_t*)p->out, stats, a);
    else cc_apply_kernel<int32_t, int32_t><<<grid, 256, 0, s>>>((const int32_t*)p->cls, map, parent, best, (int32_t*)p->out, stats, a);
  }
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
  MISEG_REQUIRE((p->logits != nullptr) != (p->cls != nullptr), MISEG_E_BADARG, "fill_holes: exactly one of logits / cls");
  MISEG_REQUIRE(!p->cls || p->cls_bytes == 1 || p->cls_bytes == 4, MISEG_E_BADARG, "fill_holes: cls_bytes %d (1 or 4)", p->cls_bytes);
  MISEG_REQUIRE(p->out && p->workspace, MISEG_E_BADARG, "fill_holes: null out / workspace pointer");
  MISEG_REQUIRE(p->out_bytes == 1 || p->out_bytes == 4, MISEG_E_BADARG, "fill_holes: out_bytes %d (1 or 4)", p->out_bytes);
  MISEG_REQUIRE(p->C >= 1 && p->C <= 64, MISEG_E_BADARG, "fill_holes: C %d (1..64)", p->C);
  MISEG_REQUIRE(p->connectivity >= 1 && p->connectivity <= 3, MISEG_E_BADARG, "fill_holes: connectivity %d (1, 2 or 3)", p->connectivity);
  MISEG_REQUIRE(p->B >= 1 && p->D >= 1 && p->D <= 65535 && p->H >= 1 && p->H <= 65535 && p->W >= 1 && p->W <= 65535, MISEG_E_BADARG,
                "fill_holes: B %d (>= 1), volume %dx%dx%d (sides 1..65535)", p->B, p->D, p->H, p->W);
  const int64_t V64 = (int64_t)p->D * p->H * p->W;
  MISEG_REQUIRE(V64 < ((int64_t)1 << 31), MISEG_E_UNSUPPORTED, "fill_holes: a sample of %lld voxels (below 2^31)", (long long)V64);
  const int V = (int)V64;
  const size_t n = (size_t)p->B * V;
  char* ws = (char*)p->workspace;
  int32_t* parent = (int32_t*)ws;
  uint8_t* work = (uint8_t*)(ws + cc_align(4 * n));
  int* box = (int*)(ws + cc_align(4 * n) + cc_align(n));
  unsigned long long* stats = (unsigned long long*)p->stats;
  FhArgs a;
  a.B = p->B; a.C = p->C; a.D = p->D; a.H = p->H; a.W = p->W; a.conn = p->connectivity; a.label = 0;
  a.applied = (p->C == 64 ? p->applied : p->applied & ((1ull << p->C) - 1)) & ~1ull;      // label 0 is the background: never applied
  int gx = cdiv(V, 256);
  if (gx > 8192) gx = 8192;
  const int gy = p->B < 65535 ? p->B : 65535;
  const dim3 grid(gx, gy);
  fh_init_kernel<<<cdiv(p->B * CC_GROUPS * FH_BOX, 256) < 1024 ? cdiv(p->B * CC_GROUPS * FH_BOX, 256) : 1024, 256, 0, s>>>(box, stats, p->B, p->C);
  MISEG_LAUNCH_CHECK("fill_holes init");
  if (p->logits) fh_prepare_kernel<float><<<grid, 256, 0, s>>>(p->logits, work, box, a);
  else if (p->cls_bytes == 1) fh_prepare_kernel<uint8_t><<<grid, 256, 0, s>>>((const uint8_t*)p->cls, work, box, a);
  else fh_prepare_kernel<int32_t><<<grid, 256, 0, s>>>((const int32_t*)p->cls, work, box, a);
  MISEG_LAUNCH_CHECK("fill_holes prepare");
  const int64_t tiles = (int64_t)cdiv(p->D, CC_TD) * cdiv(p->H, CC_TH) * cdiv(p->W, CC_TW);
  const dim3 tgrid((int)(tiles < (1 << 20) ? tiles : (1 << 20)), gy);
  // (the faces of a box are few voxels; the grid-stride loops take whatever a grid does not)
  const dim3 fgrid(gx < 1024 ? gx : 1024, gy);
  if (p->D > 1 && p->H > 1 && p->W > 1) {        // with a side of 1 every voxel lies on a face: nothing can be filled
    for (int L = 1; L < p->C; ++L) {
      if (!((a.applied >> L) & 1ull)) continue;
      a.label = L;
      fh_local_kernel<<<tgrid, 256, 0, s>>>(work, parent, box, a);
      MISEG_LAUNCH_CHECK("fill_holes local");
      fh_merge_kernel<<<grid, 256, 0, s>>>(work, parent, box, a);
      MISEG_LAUNCH_CHECK("fill_holes merge");
      fh_flatten_kernel<<<grid, 256, 0, s>>>(work, parent, box, a);
      MISEG_LAUNCH_CHECK("fill_holes flatten");
      fh_flag_kernel<<<fgrid, 256, 0, s>>>(work, parent, box, a);
      MISEG_LAUNCH_CHECK("fill_holes flag");
      fh_fill_kernel<<<grid, 256, 0, s>>>(work, parent, box, stats, a);
      MISEG_LAUNCH_CHECK("fill_holes fill");
    }
  }
  int64_t go = ((int64_t)n + 255) / 256;
  if (go > 8192 * 4) go = 8192 * 4;
  const bool o1 = p->out_bytes == 1;
  if (p->logits) {
    if (o1) fh_output_kernel<float, uint8_t><<<(int)go, 256, 0, s>>>(p->logits, work, (uint8_t*)p->out, (int64_t)n);
    else fh_output_kernel<float, int32_t><<<(int)go, 256, 0, s>>>(p->logits, work, (int32_t*)p->out, (int64_t)n);
  } else if (p->cls_bytes == 1) {
    if (o1) fh_output_kernel<uint8_t, uint8_t><<<(int)go, 256, 0, s>>>((const uint8_t*)p->cls, work, (uint8_t*)p->out, (int64_t)n);
    else fh_output_kernel<uint8_t, int32_t><<<(int)go, 256, 0, s>>>((const uint8_t*)p->cls, work, (int32_t*)p->out, (int64_t)n);
  } else {
    if (o1) fh_output_kernel<int32_t, uint8_t><<<(int)go, 256, 0, s>>>((const int32_t*)p->cls, work, (uint8_t*)p->out, (int64_t)n);
    else fh_output_kernel<int32_t, int32_t><<<(int)go, 256, 0, s>>>((const int32_t*)p->cls, work, (int32_t*)p->out, (int64_t)n);
  }
  MISEG_LAUNCH_CHECK("fill_holes output");
  return MISEG_OK;
}
