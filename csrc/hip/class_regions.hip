// Class regions of the label maps (the v2 GetClassRegions RPC).
//
// A region is a maximal 8-connected set of pixels of ONE class inside the letterbox-valid
// crop labels[:crop_h, :crop_w], for the classes of a 256-bit served set; pixels of other
// classes belong to no region and connect nothing. With the flat crop index i = y * crop_w
// + x, a region's root is its smallest i. Regions of at least min_pixels pixels pass and are
// ordered by (pixels descending, root ascending). Per frame the output is uint32[4 + 6 K]:
//   word 0  n_regions (the true number that pass; may exceed K)   word 2  crop_w
//   word 1  N = crop_w * crop_h                                   word 3  crop_h
//   then, for the first min(n_regions, K) regions in that order, six words:
//     (label << 24) | root, pixels, sum_x, sum_y, x_min | y_min << 16, x_max | y_max << 16
// Words past those are not written. postprocess/regions.py is the numpy definition.
//
// A fixed sequence of seven launches, no host round trip, no allocation (capturable). The
// workspace holds per frame parent[N], cnt[N], kBuckets x 6 x kMaxK statistics words, a
// candidate counter and 2 x kCandidates candidate words; every word that is read is written by an
// earlier kernel of the SAME run.
//   k_cr_local   one workgroup per kTile x kTile tile: union-find in LDS (atomicMin linking:
//                every root is the minimum index of its set). A pixel starts at the first
//                pixel of its horizontal same-class run (one ballot per row), so only runs
//                of adjacent rows are united, once per touching pair. Flattened: parent[i]
//                = flat index of i's tile-local root (kNone outside the class set), cnt[i]
//                = size of the tile-local component at its root, 0 elsewhere.
//   k_cr_merge   the pixels of every tile's top row and left column are united with their
//                same-class neighbours in the adjacent tiles (the diagonal ones across a
//                tile corner included): lock-free find (path halving) + atomicMin as the
//                global union-find of postprocess.hip, parents read and written with
//                agent-scope atomics. No workgroup waits on another. The final root of a
//                component is its smallest flat index whatever the arrival order.
//   k_cr_count   every tile-local root that is not the final root moves its count to the
//                final root, one integer atomic per (tile, component), and points at it.
//   k_cr_gather  the roots with cnt >= min_pixels are appended to the frame's candidate list
//                (at most kCandidates, guaranteed by N / min_pixels <= kCandidates).
//   k_cr_select  one workgroup per frame: the candidates, keyed (pixels, ~root), are ordered
//                by a bitonic sort in LDS (the keys are distinct, so the order does not
//                depend on how the list was filled). Header and words 0, 1 of the first K
//                records are written, the K statistics slots are reset, and cnt[root]
//                becomes kSlotBit | rank for those K roots.
//   k_cr_stats   per tile: coordinate sums and the bounding box of the pixels whose root
//                holds a slot, privatised in LDS per tile-local key (one set of LDS atomics
//                per horizontal run of a key, in closed form), then one set of global
//                integer atomics per (tile, component). A slot has kBuckets copies and a tile adds to
//                the copy of its index modulo kBuckets: a region that covers the frame would
//                otherwise send every tile's atomics to one address, where they queue.
//   k_cr_emit    folds a slot's copies and packs them into words 2 .. 5 of the records.
// All sums are integer: the result is exact and independent of any arrival order.
//
// With a confidence plane (conf[B, H, W], one code per pixel beside the labels) select, stats
// and emit run in their CONF form and a record has a seventh word, sum_conf: the sum of the
// codes of the region's pixels (< 2^24 x 255 < 2^32). The run's closed form does not apply: the
// lanes of a run add their codes in the wave (a segmented shuffle reduction) and the run's
// first lane sends one LDS atomic, to a seventh accumulator plane. The global sums live in
// kBuckets x kMaxK words per frame BEHIND the workspace of the form without confidence, whose
// layout, code path and output are unchanged.
#include "kernels.h"

namespace ssa {
namespace {

constexpr int kTile = 32;
constexpr int kTilePix = kTile * kTile;
constexpr int kThreads = 256;
constexpr int kPixPerThread = kTilePix / kThreads;
constexpr int kCandidates = 4096;
constexpr int kMaxK = 256;
constexpr int kStatWords = 6;  // sum_x, sum_y, x_min, y_min, x_max, y_max
constexpr int kBuckets = 16;   // copies of a statistics slot
constexpr int kSelThreads = 1024;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kSlotBit = 0x80000000u;

struct CrArgs {
  const uint8_t* labels;
  uint32_t* out;
  uint32_t* ws;
  uint32_t cls[8];
  int H, W, crop_h, crop_w, K, N;
  uint32_t min_pixels;
  const uint8_t* conf;  // CONF forms only
  uint32_t* csum;       // CONF forms only: [B][kMaxK][kBuckets] behind the B frames of ws
};

constexpr size_t kTailWords = (size_t)kStatWords * kMaxK * kBuckets + 2 + 2 * (size_t)kCandidates;
__host__ __device__ __forceinline__ size_t frame_words(size_t N) { return 2 * N + kTailWords; }
__device__ __forceinline__ size_t frame_words(const CrArgs& a) { return frame_words((size_t)a.N); }
__device__ __forceinline__ uint32_t* parent_of(const CrArgs& a, int b) { return a.ws + b * frame_words(a); }
__device__ __forceinline__ uint32_t* cnt_of(const CrArgs& a, int b) { return parent_of(a, b) + a.N; }
__device__ __forceinline__ uint32_t* stats_of(const CrArgs& a, int b) { return parent_of(a, b) + 2 * (size_t)a.N; }
// [0]: number of candidates, [2 + 2 j], [3 + 2 j]: pixels and root of candidate j
__device__ __forceinline__ uint32_t* cand_of(const CrArgs& a, int b) {
  return stats_of(a, b) + kStatWords * kMaxK * kBuckets;
}

__device__ __forceinline__ uint32_t* csum_of(const CrArgs& a, int b) {
  return a.csum + (size_t)b * kMaxK * kBuckets;
}

__device__ __forceinline__ bool served(const CrArgs& a, int l) { return (a.cls[l >> 5] >> (l & 31)) & 1u; }

// ---- union-find in LDS (one tile) -------------------------------------------------------
__device__ __forceinline__ uint32_t lds_ld(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ uint32_t lfind(uint32_t* l, uint32_t x) {
  uint32_t y = lds_ld(l + x);
  while (y != x) {
    x = y;
    y = lds_ld(l + x);
  }
  return x;
}

__device__ void lunite(uint32_t* l, uint32_t a, uint32_t b) {
  for (;;) {
    a = lfind(l, a);
    b = lfind(l, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t old = atomicMin(l + b, a);
      if (old == b) return;
      b = old;
    } else {
      const uint32_t old = atomicMin(l + a, b);
      if (old == a) return;
      a = old;
    }
  }
}

// ---- union-find in global memory (across tiles, inside one launch) ------------------------
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ uint32_t gfind(uint32_t* L, uint32_t x) {  // with path halving
  uint32_t y = ld_agent(L + x);
  while (y != x) {
    const uint32_t z = ld_agent(L + y);
    if (z != y) __hip_atomic_store(L + x, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = y;
    y = z;
  }
  return x;
}

__device__ void gunite(uint32_t* L, uint32_t a, uint32_t b) {
  for (;;) {
    a = gfind(L, a);
    b = gfind(L, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t old = atomicMin(L + b, a);
      if (old == b) return;
      b = old;
    } else {
      const uint32_t old = atomicMin(L + a, b);
      if (old == a) return;
      a = old;
    }
  }
}

// Root of x once no kernel changes the parents any more (plain loads).
__device__ __forceinline__ uint32_t find_plain(const uint32_t* L, uint32_t x) {
  uint32_t y = L[x];
  while (y != x) {
    x = y;
    y = L[x];
  }
  return x;
}

// Length of the run that starts at column lx of a tile row, from the row's 32 start flags.
__device__ __forceinline__ uint32_t run_length(uint32_t row_starts, int lx) {
  const uint32_t after = lx == kTile - 1 ? 0u : row_starts >> (lx + 1);
  return after ? (uint32_t)__ffs((int)after) : (uint32_t)(kTile - lx);
}

// ---- 1. tile-local components --------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_cr_local(CrArgs a) {
  __shared__ short lab[kTilePix];      // class id, -1: outside the crop or the class set
  __shared__ uint32_t par[kTilePix];
  __shared__ uint32_t size[kTilePix];
  const int b = blockIdx.z, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const uint8_t* img = a.labels + (size_t)b * a.H * a.W;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) cand_of(a, b)[0] = 0;
  // a wave holds two tile rows (lane & 31 = column): a pixel's first parent is the start of
  // its horizontal run, from the row's ballot of "differs from the pixel to its left"
  uint32_t start[kPixPerThread], len[kPixPerThread];  // len: of the run, at its start
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads, lx = i & (kTile - 1), x = x0 + lx, y = y0 + i / kTile;
    int l = -1;
    if (x < a.crop_w && y < a.crop_h) {
      l = img[(size_t)y * a.W + x];
      if (!served(a, l)) l = -1;
    }
    const int left = __shfl_up(l, 1, 64);
    const unsigned long long starts = __ballot(lx == 0 || left != l);
    const uint32_t row = (uint32_t)(starts >> (tid & 32));  // bit 0 is always set
    start[k] = (uint32_t)(i - lx + 31 - __clz((int)(row & ((2u << lx) - 1u))));
    len[k] = run_length(row, lx);
    lab[i] = (short)l;
    par[i] = start[k];
    size[i] = 0;
  }
  __syncthreads();
  // a run is united with each same-class run of the row above that it touches (8-neighbours),
  // by the first of its pixels that touches it
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads, lx = i & (kTile - 1);
    const int l = lab[i];
    if (l < 0 || i < kTile) continue;
    const bool left = lx > 0 && lab[i - 1] == l, right = lx < kTile - 1 && lab[i + 1] == l;
    const bool upleft = lx > 0 && lab[i - kTile - 1] == l, upright = lx < kTile - 1 && lab[i - kTile + 1] == l;
    if (lab[i - kTile] == l) {
      if (!(left && upleft)) lunite(par, i, i - kTile);  // else the pixel to the left did it
    } else {
      if (upleft && !left) lunite(par, i, i - kTile - 1);
      if (upright && !right) lunite(par, i, i - kTile + 1);  // else the pixel to the right does
    }
  }
  __syncthreads();
  // flatten: the run starts find their roots, then every pixel takes its start's
  uint32_t root[kPixPerThread];
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads;
    root[k] = (lab[i] >= 0 && start[k] == (uint32_t)i) ? lfind(par, i) : kNone;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k)
    if (root[k] != kNone) par[tid + k * kThreads] = root[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads;
    const bool on = lab[i] >= 0;
    const uint32_t r = on ? par[start[k]] : kNone;
    root[k] = r;
    if (on && start[k] == (uint32_t)i) atomicAdd(&size[r], len[k]);  // one add per run
  }
  __syncthreads();
  uint32_t* parent = parent_of(a, b);
  uint32_t* cnt = cnt_of(a, b);
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads, x = x0 + (i & (kTile - 1)), y = y0 + i / kTile;
    if (x >= a.crop_w || y >= a.crop_h) continue;
    const uint32_t r = root[k];
    const int g = y * a.crop_w + x;
    parent[g] = r == kNone ? kNone
                           : (uint32_t)((y0 + (int)(r / kTile)) * a.crop_w + x0 + (int)(r & (kTile - 1)));
    cnt[g] = r == (uint32_t)i ? size[i] : 0u;
  }
}

// ---- 2. unions across tile edges -----------------------------------------------------------
// One wave per tile: lanes 0 .. 31 take the tile's top row (neighbours N, NW, NE in the row
// above), lanes 32 .. 63 its left column (neighbours W, NW, SW in the column to the left).
// Every pair of 8-neighbours in different tiles is seen from at least one side.
__global__ __launch_bounds__(64) void k_cr_merge(CrArgs a) {
  const int b = blockIdx.z, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const uint8_t* img = a.labels + (size_t)b * a.H * a.W;
  uint32_t* parent = parent_of(a, b);
  const int t = threadIdx.x & 31;
  const bool top = threadIdx.x < 32;
  const int x = top ? x0 + t : x0, y = top ? y0 : y0 + t;
  if (x >= a.crop_w || y >= a.crop_h) return;
  if (top ? y == 0 : x == 0) return;
  const int l = img[(size_t)y * a.W + x];
  if (!served(a, l)) return;
  const uint32_t g = (uint32_t)(y * a.crop_w + x);
#pragma unroll
  for (int d = -1; d <= 1; ++d) {
    const int nx = top ? x + d : x - 1, ny = top ? y - 1 : y + d;
    if (nx < 0 || nx >= a.crop_w || ny < 0 || ny >= a.crop_h) continue;
    if (img[(size_t)ny * a.W + nx] == l) gunite(parent, g, (uint32_t)(ny * a.crop_w + nx));
  }
}

// ---- 3. component sizes at the final roots -------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_cr_count(CrArgs a) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  uint32_t* parent = parent_of(a, b);
  uint32_t* cnt = cnt_of(a, b);
  const uint32_t c = cnt[i];  // non-zero at tile-local roots only; only final roots are added to
  if (c == 0) return;
  // other threads of this launch walk through i: they meet its old parent or the root
  const uint32_t r = gfind(parent, (uint32_t)i);
  if (r == (uint32_t)i) return;
  __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(cnt + r, c);
  cnt[i] = 0;
}

// ---- 4. candidates ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_cr_gather(CrArgs a) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  const uint32_t c = cnt_of(a, b)[i];
  if (c < a.min_pixels) return;
  uint32_t* cand = cand_of(a, b);
  const uint32_t at = atomicAdd(cand, 1u);
  if (at < (uint32_t)kCandidates) {
    cand[2 + 2 * at] = c;
    cand[3 + 2 * at] = (uint32_t)i;
  }
}

// ---- 5. select and order -------------------------------------------------------------------
template <bool CONF>
__global__ __launch_bounds__(kSelThreads) void k_cr_select(CrArgs a) {
  constexpr int RW = CONF ? 7 : 6;  // words of a record
  __shared__ unsigned long long key[kCandidates];
  const int b = blockIdx.x, tid = threadIdx.x;
  uint32_t* cnt = cnt_of(a, b);
  const uint32_t* cand = cand_of(a, b);
  const uint32_t n_true = cand[0];
  const int n = (int)(n_true < (uint32_t)kCandidates ? n_true : (uint32_t)kCandidates);
  int n2 = 2;
  while (n2 < n) n2 <<= 1;
  for (int i = tid; i < n2; i += kSelThreads)  // padding sorts last: pixels >= 1
    key[i] = i < n ? ((unsigned long long)cand[2 + 2 * i] << 32) | (uint32_t)~cand[3 + 2 * i] : 0ull;
  __syncthreads();
  // bitonic sort, descending: keys are distinct (one root each), so the order is unique
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < n2; i += kSelThreads) {
        const int j = i ^ stride;
        if (j > i) {
          const unsigned long long ki = key[i], kj = key[j];
          const bool desc = (i & size) == 0;
          if (desc ? ki < kj : ki > kj) {
            key[i] = kj;
            key[j] = ki;
          }
        }
      }
      __syncthreads();
    }
  }
  uint32_t* o = a.out + (size_t)b * (4 + RW * a.K);
  uint32_t* st = stats_of(a, b);
  const uint8_t* img = a.labels + (size_t)b * a.H * a.W;
  const int kept = n < a.K ? n : a.K;
  for (int i = tid; i < kept; i += kSelThreads) {
    const unsigned long long k = key[i];
    const uint32_t root = ~(uint32_t)k, pixels = (uint32_t)(k >> 32);
    const int y = (int)(root / (uint32_t)a.crop_w), x = (int)(root - (uint32_t)y * a.crop_w);
    o[4 + RW * i] = ((uint32_t)img[(size_t)y * a.W + x] << 24) | root;
    o[4 + RW * i + 1] = pixels;
    cnt[root] = kSlotBit | (uint32_t)i;
  }
  for (int j = tid; j < kept * kBuckets; j += kSelThreads) {  // slot j / kBuckets, copy j % kBuckets
    uint32_t* s = st + kStatWords * j;
    s[0] = 0; s[1] = 0; s[2] = kNone; s[3] = kNone; s[4] = 0; s[5] = 0;
    if (CONF) csum_of(a, b)[j] = 0;
  }
  if (tid == 0) {
    o[0] = n_true;
    o[1] = (uint32_t)a.N;
    o[2] = (uint32_t)a.crop_w;
    o[3] = (uint32_t)a.crop_h;
  }
}

// ---- 6. coordinate sums and bounding boxes of the kept regions ---------------------------------
template <bool CONF>
__global__ __launch_bounds__(kThreads) void k_cr_stats(CrArgs a) {
  __shared__ uint32_t slot[kTilePix];  // per tile-local key: 0 unused, 1 used, then slot + 2 or 1
  __shared__ uint32_t acc[kStatWords + (CONF ? 1 : 0)][kTilePix];
  const int b = blockIdx.z, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const uint32_t* parent = parent_of(a, b);
  const uint32_t* cnt = cnt_of(a, b);
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads;
    slot[i] = 0;
    acc[0][i] = 0; acc[1][i] = 0; acc[2][i] = kNone; acc[3][i] = kNone; acc[4][i] = 0; acc[5][i] = 0;
    if (CONF) acc[kStatWords][i] = 0;
  }
  __syncthreads();
  // key of a pixel: its parent if that lies in this tile (its tile-local root, or for such a
  // root a smaller root of the same region), else the pixel itself. Every pixel of one key is
  // in one region, and a key is always a pixel of this tile.
  int key[kPixPerThread];
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads, x = x0 + (i & (kTile - 1)), y = y0 + i / kTile;
    key[k] = -1;
    if (x >= a.crop_w || y >= a.crop_h) continue;
    const uint32_t p = parent[y * a.crop_w + x];
    if (p == kNone) continue;
    const int py = (int)(p / (uint32_t)a.crop_w), px = (int)(p - (uint32_t)py * a.crop_w);
    const int ty = py - y0, tx = px - x0;
    key[k] = (tx >= 0 && tx < kTile && ty >= 0 && ty < kTile) ? ty * kTile + tx : i;
    slot[key[k]] = 1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads;
    if (slot[i] == 0) continue;
    const int x = x0 + (i & (kTile - 1)), y = y0 + i / kTile;
    const uint32_t c = cnt[find_plain(parent, (uint32_t)(y * a.crop_w + x))];
    slot[i] = (c & kSlotBit) ? (c & ~kSlotBit) + 2 : 1;
  }
  __syncthreads();
  // a wave holds two tile rows: the first pixel of every horizontal run of one key adds the
  // whole run in closed form
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads, lx = i & (kTile - 1);
    const uint32_t x = (uint32_t)(x0 + lx), y = (uint32_t)(y0 + i / kTile);
    const int kk = key[k];
    const int prev = __shfl_up(kk, 1, 64);  // by every lane, before any branch
    const bool head = lx == 0 || prev != kk;
    const unsigned long long heads = __ballot(head);
    uint32_t csum = 0;
    if (CONF) {
      // the codes of a run, summed into its first lane: lane + off belongs to this lane's run
      // when fewer than `rest` lanes separate them (rest: the lanes from this one to the end
      // of its run; runs are contiguous inside a tile row)
      const uint32_t rest = run_length((uint32_t)(heads >> (tid & 32)), lx);
      if (kk >= 0) csum = a.conf[((size_t)b * a.H + y) * a.W + x];
#pragma unroll
      for (int off = 1; off < kTile; off <<= 1) {  // by every lane, before any branch
        const uint32_t t = (uint32_t)__shfl_down((int)csum, off, 64);
        if ((uint32_t)off < rest) csum += t;
      }
    }
    if (!head || kk < 0 || slot[kk] < 2) continue;
    const uint32_t n = run_length((uint32_t)(heads >> (tid & 32)), lx);
    if (CONF) atomicAdd(&acc[kStatWords][kk], csum);
    atomicAdd(&acc[0][kk], n * (2 * x + n - 1) / 2); atomicAdd(&acc[1][kk], n * y);
    atomicMin(&acc[2][kk], x); atomicMin(&acc[3][kk], y);
    atomicMax(&acc[4][kk], x + n - 1); atomicMax(&acc[5][kk], y);
  }
  __syncthreads();
  uint32_t* st = stats_of(a, b) + kStatWords * ((blockIdx.y * gridDim.x + blockIdx.x) % kBuckets);
#pragma unroll
  for (int k = 0; k < kPixPerThread; ++k) {
    const int i = tid + k * kThreads;
    if (slot[i] < 2) continue;
    uint32_t* s = st + kStatWords * kBuckets * (slot[i] - 2);
    // scattered global atomics are the cost of this kernel. Both sums go in one 64-bit add
    // (8-byte aligned; sum_x < 2^32 by the geometry check, so nothing carries into sum_y).
    // A box edge that does not improve on the value read is not sent: the stored edges only
    // tighten during the launch, so a stale read can cost a needless atomic, never skip one.
    atomicAdd(reinterpret_cast<unsigned long long*>(s), ((unsigned long long)acc[1][i] << 32) | acc[0][i]);
    if (acc[2][i] < s[2]) atomicMin(s + 2, acc[2][i]);
    if (acc[3][i] < s[3]) atomicMin(s + 3, acc[3][i]);
    if (acc[4][i] > s[4]) atomicMax(s + 4, acc[4][i]);
    if (acc[5][i] > s[5]) atomicMax(s + 5, acc[5][i]);
    if (CONF)
      atomicAdd(csum_of(a, b) + kBuckets * (slot[i] - 2) + (blockIdx.y * gridDim.x + blockIdx.x) % kBuckets,
                acc[kStatWords][i]);
  }
}

// ---- 7. pack ---------------------------------------------------------------------------------
template <bool CONF>
__global__ __launch_bounds__(kMaxK) void k_cr_emit(CrArgs a) {
  constexpr int RW = CONF ? 7 : 6;
  const int b = blockIdx.x, i = threadIdx.x;
  uint32_t* o = a.out + (size_t)b * (4 + RW * a.K);
  const uint32_t n = o[0];
  if (i >= a.K || (uint32_t)i >= n) return;
  const uint32_t* s = stats_of(a, b) + kStatWords * kBuckets * i;
  uint32_t sx = 0, sy = 0, xl = kNone, yl = kNone, xh = 0, yh = 0;
#pragma unroll
  for (int c = 0; c < kBuckets; ++c, s += kStatWords) {
    sx += s[0];
    sy += s[1];
    xl = s[2] < xl ? s[2] : xl;
    yl = s[3] < yl ? s[3] : yl;
    xh = s[4] > xh ? s[4] : xh;
    yh = s[5] > yh ? s[5] : yh;
  }
  uint32_t* r = o + 4 + RW * i;
  r[2] = sx;
  r[3] = sy;
  r[4] = xl | (yl << 16);
  r[5] = xh | (yh << 16);
  if (CONF) {
    const uint32_t* c = csum_of(a, b) + kBuckets * i;
    uint32_t sc = 0;
#pragma unroll
    for (int q = 0; q < kBuckets; ++q) sc += c[q];
    r[6] = sc;
  }
}

// ---- region tracks (postprocess/tracks.py is the definition) --------------------------------
// Five launches that follow k_cr_emit in the same chain; they read what the class-region
// kernels leave (the final parent[], cnt[root] = kSlotBit | rank of the stored regions, the
// records) and change none of it. `rows` are the records of this run ([B, 4 + RW K]), `out`
// the rows with tracks ([B, 4 + (RW + 2) K]): the record's words, then track_id and age.
//   k_tr_slots    S[b][i], a uint16 plane per frame: the rank of pixel i's stored region,
//                 kNoSlot without one. Its blocks also zero the rows of the frame's overlap
//                 table that are used (n_t x K words).
//   k_tr_overlap  per frame, a pass over S[b] and the plane of the stream's previous frame:
//                 S[pred[b]] of this batch, or the stream's carried plane. The pixels are
//                 taken in flat order (an overlap count knows no geometry): one LDS atomic per
//                 run of an equal (a, b') key inside a wave (one ballot), into a hash table of
//                 the block's chunk, then one global integer atomic per key and block. A key
//                 that finds no entry within kProbes goes to the global table directly.
//   k_tr_carry    copies the plane of each stream's last frame of the batch to its state.
//   k_tr_match    one workgroup per frame: best and winner from the table, link[b][a] = the
//                 predecessor of a matched region; copies the record words to the wide rows.
//   k_tr_assign   one workgroup per stream, its frames in batch order: ids and ages from the
//                 previous frame's (LDS; first the carried state's), new ids by a ballot scan,
//                 the two words of every stored record, then the carried state.
// Per stream the state is [n, issued, pad, pad, track_id[kMaxK], age[kMaxK], label[kMaxK],
// pixels[kMaxK]] words and a plane of plane_words(N) words; all zero: no predecessor, nothing
// issued. A stream without a row in the batch keeps its state.
constexpr uint32_t kNoSlot = 0xFFFFu;
constexpr int kStateHead = 4 + 4 * kMaxK;
constexpr int kOvPix = 16;                      // pixels per thread of an overlap block
constexpr int kOvChunk = kThreads * kOvPix;
constexpr int kHash = 1024;
constexpr int kProbes = 16;

__host__ __device__ __forceinline__ size_t plane_words(size_t N) { return (N + 3) / 4 * 2; }  // 8-byte multiple
__host__ __device__ __forceinline__ size_t state_words(size_t N) { return kStateHead + plane_words(N); }

struct TrArgs {
  const uint32_t* ws;    // of class_regions, after its run
  const uint32_t* rows;  // [B, 4 + RW K]
  uint32_t* out;         // [B, 4 + (RW + 2) K]
  uint32_t* tws;         // planes [B][plane_words], then tables [B][K][K], then links [B][K]
  uint32_t* state;       // [S][state_words]
  const int* pred;       // [B]
  const int* stream;     // [B]
  const int* last;       // [S]
  int B, S, K, N, RW;
  uint32_t q;
};

__device__ __forceinline__ uint16_t* tr_plane(const TrArgs& t, int b) {
  return reinterpret_cast<uint16_t*>(t.tws + (size_t)b * plane_words((size_t)t.N));
}
__device__ __forceinline__ uint32_t* tr_table(const TrArgs& t, int b) {
  return t.tws + (size_t)t.B * plane_words((size_t)t.N) + (size_t)b * t.K * t.K;
}
__device__ __forceinline__ uint32_t* tr_state(const TrArgs& t, int s) {
  return t.state + (size_t)s * state_words((size_t)t.N);
}
__device__ __forceinline__ uint32_t tr_stored(const TrArgs& t, int b) {  // min(n_regions, K)
  const uint32_t n = t.rows[(size_t)b * (4 + t.RW * t.K)];
  return n < (uint32_t)t.K ? n : (uint32_t)t.K;
}

// The rank of pixel i's stored region from a frame's class-region workspace after its run
// (parent[N], cnt[N]), kNoSlot without one.
__device__ __forceinline__ uint16_t resolve_slot(const uint32_t* parent, int N, int i) {
  const uint32_t* cnt = parent + N;
  uint32_t slot = kNoSlot;
  if (parent[i] != kNone) {
    const uint32_t c = cnt[find_plain(parent, (uint32_t)i)];
    if (c & kSlotBit) slot = c & ~kSlotBit;
  }
  return (uint16_t)slot;
}

__global__ __launch_bounds__(kThreads) void k_tr_slots(TrArgs t) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  uint32_t* tab = tr_table(t, b);
  const uint32_t used = tr_stored(t, b) * (uint32_t)t.K;
  for (uint32_t j = (uint32_t)i; j < used; j += gridDim.x * kThreads) tab[j] = 0;
  if (i >= t.N) return;
  tr_plane(t, b)[i] = resolve_slot(t.ws + (size_t)b * frame_words((size_t)t.N), t.N, i);
}

// The slot plane alone, for a consumer without tracking (zone_presence.hip): planes[b] is a
// plane of plane_words(N) words, as tr_plane's.
__global__ __launch_bounds__(kThreads) void k_cr_slot_plane(const uint32_t* ws, uint32_t* planes, int N) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  reinterpret_cast<uint16_t*>(planes + (size_t)b * plane_words((size_t)N))[i] =
      resolve_slot(ws + (size_t)b * frame_words((size_t)N), N, i);
}

__global__ __launch_bounds__(kThreads) void k_tr_overlap(TrArgs t) {
  __shared__ uint32_t hkey[kHash];
  __shared__ uint32_t hcnt[kHash];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int p = t.pred[b];
  const uint32_t n_cur = tr_stored(t, b);
  const uint16_t* prev;
  uint32_t n_prev;
  if (p >= 0) {
    prev = tr_plane(t, p);
    n_prev = tr_stored(t, p);
  } else {
    const uint32_t* st = tr_state(t, t.stream[b]);
    prev = reinterpret_cast<const uint16_t*>(st + kStateHead);
    n_prev = st[0] < (uint32_t)t.K ? st[0] : (uint32_t)t.K;
  }
  if (n_cur == 0 || n_prev == 0) return;  // by the whole block
  for (int j = tid; j < kHash; j += kThreads) {
    hkey[j] = kNone;
    hcnt[j] = 0;
  }
  __syncthreads();
  const uint16_t* cur = tr_plane(t, b);
  uint32_t* tab = tr_table(t, b);
  const int lane = tid & 63;
  const int base = blockIdx.x * kOvChunk + (tid >> 6) * (64 * kOvPix);  // a wave: 64 x kOvPix pixels in a row
#pragma unroll 4
  for (int k = 0; k < kOvPix; ++k) {
    const int i = base + k * 64 + lane;
    uint32_t key = kNone;
    if (i < t.N) {
      const uint32_t a = cur[i], bp = prev[i];
      if (a < n_cur && bp < n_prev) key = a * (uint32_t)t.K + bp;
    }
    const uint32_t left = (uint32_t)__shfl_up((int)key, 1, 64);  // by every lane, before any branch
    const bool head = lane == 0 || left != key;
    const unsigned long long heads = __ballot(head);
    if (!head || key == kNone) continue;
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    const uint32_t n = after ? (uint32_t)__ffsll((long long)after) : (uint32_t)(64 - lane);
    uint32_t h = (key * 2654435761u) >> 22;  // kHash = 2^10
    bool done = false;
    for (int probe = 0; probe < kProbes && !done; ++probe, h = (h + 1) & (kHash - 1)) {
      const uint32_t old = atomicCAS(&hkey[h], kNone, key);
      if (old == kNone || old == key) {
        atomicAdd(&hcnt[h], n);
        done = true;
      }
    }
    if (!done) atomicAdd(tab + key, n);
  }
  __syncthreads();
  for (int j = tid; j < kHash; j += kThreads)
    if (hkey[j] != kNone) atomicAdd(tab + hkey[j], hcnt[j]);
}

__global__ __launch_bounds__(kThreads) void k_tr_carry(TrArgs t) {
  const int s = blockIdx.y;
  const int r = t.last[s];
  if (r < 0) return;
  const size_t w = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (w >= plane_words((size_t)t.N)) return;
  (tr_state(t, s) + kStateHead)[w] = (t.tws + (size_t)r * plane_words((size_t)t.N))[w];
}

// best, winner and matched of every frame, in parallel over the frames: link[b][a] = best[a] if
// a is matched, else kNone. A wave takes a region a at a time, its lanes the predecessors b'
// (coalesced table reads); (overlap, ~index) packed in 64 bits makes "largest overlap, then the
// smaller index" one maximum, over the lanes by shuffles and per b' by one LDS atomic. The frame's
// header and record words are copied to the rows with tracks here too.
__global__ __launch_bounds__(kMaxK) void k_tr_match(TrArgs t) {
  __shared__ uint32_t p_lab[kMaxK], p_pix[kMaxK], best[kMaxK];
  __shared__ unsigned long long wkey[kMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int RW = t.RW, OW = t.RW + 2;
  const uint32_t* row = t.rows + (size_t)b * (4 + RW * t.K);
  uint32_t* o = t.out + (size_t)b * (4 + OW * t.K);
  const uint32_t n_cur = tr_stored(t, b);
  const int p = t.pred[b];
  uint32_t n_prev;
  if (p >= 0) {
    const uint32_t* prow = t.rows + (size_t)p * (4 + RW * t.K);
    n_prev = tr_stored(t, p);
    if ((uint32_t)tid < n_prev) {
      p_lab[tid] = prow[4 + RW * tid] >> 24;
      p_pix[tid] = prow[4 + RW * tid + 1];
    }
  } else {
    const uint32_t* st = tr_state(t, t.stream[b]);
    n_prev = st[0] < (uint32_t)t.K ? st[0] : (uint32_t)t.K;
    if ((uint32_t)tid < n_prev) {
      p_lab[tid] = st[4 + 2 * kMaxK + tid];
      p_pix[tid] = st[4 + 3 * kMaxK + tid];
    }
  }
  wkey[tid] = 0ull;
  best[tid] = kNone;
  if (tid < 4) o[tid] = row[tid];
  for (uint32_t w = (uint32_t)tid; w < n_cur * (uint32_t)RW; w += kMaxK) {
    const uint32_t a = w / (uint32_t)RW;
    o[4 + OW * a + (w - a * RW)] = row[4 + w];
  }
  __syncthreads();
  const uint32_t* tab = tr_table(t, b);
  for (uint32_t a = (uint32_t)tid >> 6; a < n_cur; a += kMaxK / 64) {  // by whole waves
    const uint32_t lab = row[4 + RW * a] >> 24, pix = row[4 + RW * a + 1];
    unsigned long long k = 0ull;
    for (uint32_t j = (uint32_t)lane; j < n_prev; j += 64) {
      if (p_lab[j] != lab) continue;
      const uint32_t ov = tab[(size_t)a * t.K + j];
      const uint32_t lo = pix < p_pix[j] ? pix : p_pix[j];
      if (ov > 0 && 1024ull * ov >= (unsigned long long)t.q * lo) {
        const unsigned long long c = ((unsigned long long)ov << 32) | (uint32_t)~j;
        k = c > k ? c : k;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long c = (unsigned long long)__shfl_xor((long long)k, off, 64);
      k = c > k ? c : k;
    }
    if (lane == 0 && k != 0ull) {
      const uint32_t bb = ~(uint32_t)k;
      best[a] = bb;
      atomicMax(&wkey[bb], (k & 0xFFFFFFFF00000000ull) | (uint32_t)~a);
    }
  }
  __syncthreads();
  if ((uint32_t)tid < n_cur) {
    const uint32_t bb = best[tid];
    t.tws[(size_t)t.B * plane_words((size_t)t.N) + (size_t)t.B * t.K * t.K + (size_t)b * t.K + tid] =
        (bb != kNone && ~(uint32_t)wkey[bb] == (uint32_t)tid) ? bb : kNone;
  }
}

// One workgroup per stream: the short chain over its frames in batch order. Thread a takes the
// id and age of its predecessor (LDS; for the first frame the carried state's) or a new id, by
// a ballot scan over the unmatched regions, and writes the two words; then the carried state.
__global__ __launch_bounds__(kMaxK) void k_tr_assign(TrArgs t) {
  __shared__ uint32_t p_id[2][kMaxK], p_age[2][kMaxK];
  __shared__ uint32_t wave_new[2][kMaxK / 64];
  const int s = blockIdx.x, a = threadIdx.x;
  const int r1 = t.last[s];
  if (r1 < 0) return;  // no row of this stream in the batch: its state stays
  int r0 = r1;
  while (t.pred[r0] >= 0) r0 = t.pred[r0];
  uint32_t* st = tr_state(t, s);
  uint32_t issued = st[1];
  p_id[0][a] = st[4 + a];
  p_age[0][a] = st[4 + kMaxK + a];
  const uint32_t* links = t.tws + (size_t)t.B * plane_words((size_t)t.N) + (size_t)t.B * t.K * t.K;
  const int RW = t.RW, OW = t.RW + 2;
  uint32_t n_cur = tr_stored(t, r0);
  uint32_t link = (uint32_t)a < n_cur ? links[(size_t)r0 * t.K + a] : kNone;
  __syncthreads();
  int cur = 0;
  for (int r = r0; r <= r1; ++r, cur ^= 1) {  // consecutive rows (the host builds pred so)
    const bool on = (uint32_t)a < n_cur, matched = on && link != kNone, fresh = on && !matched;
    uint32_t n_next = 0, link_next = kNone;  // the next frame's, loaded under this one's work
    if (r < r1) {
      n_next = tr_stored(t, r + 1);
      if ((uint32_t)a < n_next) link_next = links[(size_t)(r + 1) * t.K + a];
    }
    const unsigned long long m = __ballot(fresh);
    if ((a & 63) == 0) wave_new[cur][a >> 6] = (uint32_t)__popcll(m);
    __syncthreads();  // one barrier a frame (the arrays alternate): also orders the previous
    uint32_t id = 0, age = 0;  // frame's ids and ages before these reads
    if (matched) {
      id = p_id[cur][link];
      age = p_age[cur][link] + 1;
    }
    uint32_t before = (uint32_t)__popcll(m & ((1ull << (a & 63)) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < kMaxK / 64; ++w) {
      if (w < (a >> 6)) before += wave_new[cur][w];
      total += wave_new[cur][w];
    }
    if (fresh) {
      id = issued + 1 + before;
      age = 1;
    }
    issued += total;
    if (on) {
      uint32_t* o = t.out + (size_t)r * (4 + OW * t.K) + 4 + OW * a + RW;
      o[0] = id;
      o[1] = age;
    }
    p_id[cur ^ 1][a] = id;
    p_age[cur ^ 1][a] = age;
    if (r < r1) {
      n_cur = n_next;
      link = link_next;
    }
  }
  __syncthreads();
  st[4 + a] = p_id[cur][a];
  st[4 + kMaxK + a] = p_age[cur][a];
  const uint32_t* row = t.rows + (size_t)r1 * (4 + RW * t.K);
  if ((uint32_t)a < n_cur) {
    st[4 + 2 * kMaxK + a] = row[4 + RW * a] >> 24;
    st[4 + 3 * kMaxK + a] = row[4 + RW * a + 1];
  }
  if (a == 0) {
    st[0] = n_cur;
    st[1] = issued;
  }
}

}  // namespace

int class_regions_tile() { return kTile; }
int class_regions_candidates() { return kCandidates; }

size_t class_regions_workspace_bytes(int B, int crop_h, int crop_w, bool conf) {
  const size_t N = (size_t)crop_h * (size_t)crop_w;
  return (size_t)B * (frame_words(N) + (conf ? (size_t)kMaxK * kBuckets : 0)) * sizeof(uint32_t);
}

void class_regions(const ClassRegionsParams& p, hipStream_t s) {
  const long long N = (long long)p.crop_h * p.crop_w;
  if (p.B <= 0 || p.B > 65535 || p.crop_h <= 0 || p.crop_w <= 0 || p.crop_h > p.H ||
      p.crop_w > p.W || N >= (1LL << 24) ||
      N * (p.crop_w > p.crop_h ? p.crop_w : p.crop_h) >= (1LL << 32) || p.K < 1 || p.K > kMaxK ||
      p.min_pixels < 1 || N / p.min_pixels > kCandidates)
    check(hipErrorInvalidValue, "class_regions: bad shape");
  CrArgs a;
  a.labels = p.labels; a.out = p.out; a.ws = p.ws;
  for (int i = 0; i < 8; ++i) a.cls[i] = p.classes[i];
  a.H = p.H; a.W = p.W; a.crop_h = p.crop_h; a.crop_w = p.crop_w; a.K = p.K; a.N = (int)N;
  a.min_pixels = (uint32_t)p.min_pixels;
  a.conf = p.conf;
  a.csum = p.conf ? p.ws + (size_t)p.B * frame_words((size_t)N) : nullptr;
  const dim3 tiles(cdiv(p.crop_w, kTile), cdiv(p.crop_h, kTile), p.B);
  hipLaunchKernelGGL(k_cr_local, tiles, dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(k_cr_merge, tiles, dim3(64), 0, s, a);
  const dim3 flat(cdiv(N, kThreads), p.B);
  hipLaunchKernelGGL(k_cr_count, flat, dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(k_cr_gather, flat, dim3(kThreads), 0, s, a);
  if (p.conf) {
    hipLaunchKernelGGL(k_cr_select<true>, dim3(p.B), dim3(kSelThreads), 0, s, a);
    hipLaunchKernelGGL(k_cr_stats<true>, tiles, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(k_cr_emit<true>, dim3(p.B), dim3(kMaxK), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_cr_select<false>, dim3(p.B), dim3(kSelThreads), 0, s, a);
    hipLaunchKernelGGL(k_cr_stats<false>, tiles, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(k_cr_emit<false>, dim3(p.B), dim3(kMaxK), 0, s, a);
  }
  check_launch("class_regions");
}

size_t region_tracks_workspace_bytes(int B, int crop_h, int crop_w, int K) {
  const size_t N = (size_t)crop_h * (size_t)crop_w;
  return ((size_t)B * plane_words(N) + (size_t)B * K * K + (size_t)B * K) * sizeof(uint32_t);
}

// the layout of the tracking workspace, for zone_presence.hip
size_t region_slot_plane_words(int crop_h, int crop_w) { return plane_words((size_t)crop_h * (size_t)crop_w); }
size_t region_tracks_planes_offset_words() { return 0; }
size_t region_tracks_links_offset_words(int B, int crop_h, int crop_w, int K) {
  return (size_t)B * plane_words((size_t)crop_h * (size_t)crop_w) + (size_t)B * K * K;
}

void class_regions_slot_planes(const uint32_t* ws, uint32_t* planes, int B, int crop_h, int crop_w,
                               hipStream_t s) {
  const long long N = (long long)crop_h * crop_w;
  if (B <= 0 || B > 65535 || crop_h <= 0 || crop_w <= 0 || N >= (1LL << 24) || !ws || !planes)
    check(hipErrorInvalidValue, "class_regions_slot_planes: bad arguments");
  hipLaunchKernelGGL(k_cr_slot_plane, dim3(cdiv(N, kThreads), B), dim3(kThreads), 0, s, ws, planes, (int)N);
  check_launch("class_regions_slot_planes");
}

size_t region_tracks_state_bytes(int streams, int crop_h, int crop_w) {
  return (size_t)streams * state_words((size_t)crop_h * (size_t)crop_w) * sizeof(uint32_t);
}

void region_tracks(const RegionTracksParams& p, hipStream_t s) {
  const long long N = (long long)p.crop_h * p.crop_w;
  if (p.B <= 0 || p.B > 65535 || p.streams <= 0 || p.streams > 65535 || p.crop_h <= 0 ||
      p.crop_w <= 0 || N >= (1LL << 24) || p.K < 1 || p.K > kMaxK ||
      (p.record_words != 6 && p.record_words != 7) || p.q < 1 || p.q > 1024 || !p.ws || !p.rows ||
      !p.out || !p.tws || !p.state || !p.pred || !p.stream || !p.last)
    check(hipErrorInvalidValue, "region_tracks: bad arguments");
  TrArgs t;
  t.ws = p.ws; t.rows = p.rows; t.out = p.out; t.tws = p.tws; t.state = p.state;
  t.pred = p.pred; t.stream = p.stream; t.last = p.last;
  t.B = p.B; t.S = p.streams; t.K = p.K; t.N = (int)N; t.RW = p.record_words; t.q = (uint32_t)p.q;
  if (p.kernels & 1) hipLaunchKernelGGL(k_tr_slots, dim3(cdiv(N, kThreads), p.B), dim3(kThreads), 0, s, t);
  if (p.kernels & 2) hipLaunchKernelGGL(k_tr_overlap, dim3(cdiv(N, kOvChunk), p.B), dim3(kThreads), 0, s, t);
  if (p.kernels & 4)
    hipLaunchKernelGGL(k_tr_carry, dim3(cdiv((long long)plane_words((size_t)N), kThreads), p.streams),
                       dim3(kThreads), 0, s, t);
  if (p.kernels & 8) hipLaunchKernelGGL(k_tr_match, dim3(p.B), dim3(kMaxK), 0, s, t);
  if (p.kernels & 16) hipLaunchKernelGGL(k_tr_assign, dim3(p.streams), dim3(kMaxK), 0, s, t);
  check_launch("region_tracks");
}

}  // namespace ssa
