// Zone occupancy of the label maps (the v2 GetZoneOccupancy RPC; the definition is
// postprocess/zones.py).
//
// A frame's crop labels[:crop_h, :crop_w] is read as one flat row-major sequence of N = crop_h *
// crop_w pixels (i = y * crop_w + x) beside the zone plane (uint32[N], bit z - 1: pixel i is in
// user zone z; shared by every frame) and, optionally, the confidence plane of the labels. With
// R = 1 + Z rows (row 0: the whole crop) and C classes, per frame out[b] = uint32[4 + R C], or
// uint32[4 + 2 R C] with confidence:
//   words 0-3       R, N, crop_w, crop_h
//   4 + r C + c     pixels[r][c]   = #{ i : L(i) == c and (r == 0 or bit r - 1 of plane[i]) }
//   4 + (R + r) C + c  sum_conf[r][c] = the sum of conf[i] over the same pixels
// Pixels whose label is >= C count nowhere. Every word is written by every run.
//
// Two launches on one stream:
//   k_zone_init   the header and zeros over the whole row of every frame
//   k_zone_count  grid (chunks of kZsChunk flat pixels, B): a workgroup-private [R][C] table in
//                 LDS (two with confidence), filled by run aggregation -- label maps and zone
//                 planes are piecewise constant, so among the 64 consecutive pixels of a wave
//                 the first lane of each run of equal (label, plane word) adds the run's length
//                 (and its code sum, from a wave prefix sum) once for row 0 and once per set
//                 zone bit -- then the non-zero counters are added to the frame's row with
//                 integer global atomics.
// Integer adds commute: the words do not depend on the arrival order, they are exact. No float
// arithmetic, no allocation, no host sync: capturable. No workspace is read or written.
#include "kernels.h"

namespace ssa {
namespace {

constexpr int kZsThreads = 256;
constexpr int kZsPix = 32;  // flat pixels per thread: 32 wave rows of 64 consecutive pixels
constexpr int kZsChunk = kZsThreads * kZsPix;
constexpr int kZsCounters = 4096;  // R * C <= this (zones.py ZONE_COUNTERS)

struct ZsArgs {
  const uint8_t* labels;
  const uint8_t* conf;
  const uint32_t* plane;
  uint32_t* out;
  int H, W, crop_h, crop_w, N, R, C, RC, row_words;
  uint32_t zmask;  // the bits of the user zones 1 .. R - 1
};

__global__ __launch_bounds__(kZsThreads) void k_zone_init(ZsArgs a) {
  const int i = blockIdx.x * kZsThreads + threadIdx.x;
  if (i >= a.row_words) return;
  uint32_t v = 0;
  if (i == 0) v = (uint32_t)a.R;
  else if (i == 1) v = (uint32_t)a.N;
  else if (i == 2) v = (uint32_t)a.crop_w;
  else if (i == 3) v = (uint32_t)a.crop_h;
  a.out[(size_t)blockIdx.y * a.row_words + i] = v;
}

template <bool CONF>
__global__ __launch_bounds__(kZsThreads) void k_zone_count(ZsArgs a) {
  __shared__ uint32_t tab[(CONF ? 2 : 1) * kZsCounters];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int used = (CONF ? 2 : 1) * a.RC;
  for (int j = tid; j < used; j += kZsThreads) tab[j] = 0;
  __syncthreads();
  const size_t img = (size_t)b * a.H * a.W;
  // a wave: kZsPix rows of 64 consecutive flat pixels
  int i = blockIdx.x * kZsChunk + (tid >> 6) * (64 * kZsPix) + lane;
  int y = i / a.crop_w, x = i - y * a.crop_w;
#pragma unroll 4
  for (int k = 0; k < kZsPix; ++k, i += 64) {
    uint32_t lab = 0xffffffffu, word = 0, code = 0;  // past the crop, or not a class: no key
    if (i < a.N) {
      const size_t at = img + (size_t)y * a.W + x;
      const uint32_t l = a.labels[at];
      if (l < (uint32_t)a.C) {
        lab = l;
        if (a.plane) word = a.plane[i] & a.zmask;
        if (CONF) code = a.conf[at];
      }
    }
    x += 64;
    if (x >= a.crop_w) {
      if (a.crop_w >= 64) {
        x -= a.crop_w;
        ++y;
      } else {
        y += x / a.crop_w;
        x %= a.crop_w;
      }
    }
    // by every lane, before any branch
    const uint32_t llab = (uint32_t)__shfl_up((int)lab, 1, 64);
    const uint32_t lword = (uint32_t)__shfl_up((int)word, 1, 64);
    const bool head = lane == 0 || llab != lab || lword != word;
    const unsigned long long heads = __ballot(head);
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    const uint32_t n = after ? (uint32_t)__ffsll((long long)after) : (uint32_t)(64 - lane);
    uint32_t csum = 0;
    if (CONF) {
      uint32_t incl = code;  // inclusive prefix sum of the codes over the wave
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += up;
      }
      const uint32_t end = (uint32_t)__shfl((int)incl, (lane + (int)n - 1) & 63, 64);
      csum = end - (incl - code);
    }
    if (!head || lab == 0xffffffffu) continue;
    atomicAdd(&tab[lab], n);
    if (CONF) atomicAdd(&tab[a.RC + lab], csum);
    while (word) {
      const int r = __ffs((int)word);  // 1-based bit: the zone's row
      word &= word - 1;
      atomicAdd(&tab[r * a.C + lab], n);
      if (CONF) atomicAdd(&tab[a.RC + r * a.C + lab], csum);
    }
  }
  __syncthreads();
  uint32_t* o = a.out + (size_t)b * a.row_words + 4;
  for (int j = tid; j < used; j += kZsThreads) {
    const uint32_t v = tab[j];
    if (v) atomicAdd(o + j, v);
  }
}

}  // namespace

int zone_stats_chunk() { return kZsChunk; }

size_t zone_stats_workspace_bytes(int, int, int, bool) { return 0; }  // atomics into `out`: none

void zone_stats(const ZoneStatsParams& p, hipStream_t s) {
  const long long N = (long long)p.crop_h * p.crop_w;
  if (p.B <= 0 || p.B > 65535 || p.crop_h <= 0 || p.crop_w <= 0 || p.crop_h > p.H || p.crop_w > p.W ||
      N >= (1LL << 24) || p.R < 1 || p.R > 33 || p.C < 1 || p.C > 256 || p.R * p.C > kZsCounters ||
      (p.R > 1) != (p.plane != nullptr) || p.labels == nullptr || p.out == nullptr)
    check(hipErrorInvalidValue, "zone_stats: bad shape");
  ZsArgs a;
  a.labels = p.labels; a.conf = p.conf; a.plane = p.plane; a.out = p.out;
  a.H = p.H; a.W = p.W; a.crop_h = p.crop_h; a.crop_w = p.crop_w; a.N = (int)N;
  a.R = p.R; a.C = p.C; a.RC = p.R * p.C;
  a.row_words = 4 + a.RC * (p.conf ? 2 : 1);
  a.zmask = p.R >= 33 ? 0xffffffffu : ((1u << (p.R - 1)) - 1u);
  hipLaunchKernelGGL(k_zone_init, dim3(cdiv(a.row_words, kZsThreads), p.B), dim3(kZsThreads), 0, s, a);
  const dim3 grid(cdiv(N, kZsChunk), p.B);
  if (p.conf)
    hipLaunchKernelGGL(k_zone_count<true>, grid, dim3(kZsThreads), 0, s, a);
  else
    hipLaunchKernelGGL(k_zone_count<false>, grid, dim3(kZsThreads), 0, s, a);
  check_launch("zone_stats");
}

}  // namespace ssa
