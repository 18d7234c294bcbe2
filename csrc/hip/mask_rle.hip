// Run-length encoder of the label maps (the v2 GetSegmentationMask RPC).
//
// A frame's mask is the letterbox-valid region labels[:crop_h, :crop_w] read as ONE flat
// row-major sequence of N = crop_h * crop_w pixels (flat index i = y * crop_w + x, so a
// run continues across a row end). Pixel i starts a run iff i == 0 or L(i) != L(i - 1).
// Per frame the output is uint32[4 + cap]:
//   word 0  n_runs (the true total; may exceed cap)   word 2  crop_w
//   word 1  N                                         word 3  crop_h
//   word 4 + k  (label << 24) | start_k   for k < min(n_runs, cap), in run order
// Words past 4 + min(n_runs, cap) are not written. Starts (not lengths) are stored, so
// no look-ahead is needed; N < 2^24 keeps a start in 24 bits (checked by the caller).
//
// Two passes over chunks of kChunk flat pixels, in the style of the two-pass post kernels:
//   k_rle_count  per chunk, the number of run starts -> ws[b][chunk]
//   k_rle_emit   per chunk: prefix = sum of ws[b][0 .. chunk), recomputed start flags,
//                an exclusive scan inside the workgroup (per-thread popcount, wave64
//                shuffle scan, wave totals through LDS), then one store per start whose
//                position is < cap. The last chunk's workgroup writes the header.
// A run's position comes from the prefix sums only, never from the arrival order of
// atomics: the output is exact and deterministic. No allocation, no host sync: capturable.
#include <algorithm>

#include "kernels.h"

namespace ssa {
namespace {

constexpr int kRleThreads = 256;
constexpr int kRlePix = 16;  // flat pixels per thread (one bit each in a 16-bit flag mask)
constexpr int kRleChunk = kRleThreads * kRlePix;
constexpr int kRleWaves = kRleThreads / 64;

struct RleArgs {
  const uint8_t* labels;
  uint32_t* out;
  uint32_t* ws;
  int H, W, crop_h, crop_w, cap, N, nchunks;
};

// The thread's 16 flat pixels (from i0; those at or past N are skipped): bit j of the
// result is set iff pixel i0 + j starts a run. lab[j] holds the labels read.
__device__ __forceinline__ unsigned rle_flags(const RleArgs& a, const uint8_t* img, int i0,
                                              uint8_t (&lab)[kRlePix]) {
  if (i0 >= a.N) return 0u;
  int y = i0 / a.crop_w, x = i0 - y * a.crop_w;
  int prev = -1;  // pixel 0 always starts a run
  if (i0 > 0) {
    const int py = x > 0 ? y : y - 1, px = x > 0 ? x - 1 : a.crop_w - 1;
    prev = img[(size_t)py * a.W + px];
  }
  const uint8_t* row = img + (size_t)y * a.W;
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < kRlePix; ++j) {
    if (i0 + j < a.N) {
      const int l = row[x];
      lab[j] = (uint8_t)l;
      m |= (unsigned)(l != prev) << j;
      prev = l;
      if (++x == a.crop_w) {
        x = 0;
        row += a.W;
      }
    }
  }
  return m;
}

// Sum of v over the workgroup, returned to every thread (red: kRleWaves words of LDS).
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* red) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read from a previous use
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  unsigned t = 0;
#pragma unroll
  for (int w = 0; w < kRleWaves; ++w) t += red[w];
  return t;
}

__global__ __launch_bounds__(kRleThreads) void k_rle_count(RleArgs a) {
  __shared__ unsigned red[kRleWaves];
  const int chunk = blockIdx.x, b = blockIdx.y;
  const uint8_t* img = a.labels + (size_t)b * a.H * a.W;
  uint8_t lab[kRlePix];
  const unsigned m = rle_flags(a, img, chunk * kRleChunk + (int)threadIdx.x * kRlePix, lab);
  const unsigned total = block_sum((unsigned)__popc(m), red);
  if (threadIdx.x == 0) a.ws[(size_t)b * a.nchunks + chunk] = total;
}

__global__ __launch_bounds__(kRleThreads) void k_rle_emit(RleArgs a) {
  __shared__ unsigned red[kRleWaves];
  __shared__ unsigned wtot[kRleWaves];
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint8_t* img = a.labels + (size_t)b * a.H * a.W;
  // runs that start before this chunk
  const uint32_t* cnt = a.ws + (size_t)b * a.nchunks;
  unsigned part = 0;
  for (int j = threadIdx.x; j < chunk; j += kRleThreads) part += cnt[j];
  const unsigned prefix = block_sum(part, red);

  const int i0 = chunk * kRleChunk + (int)threadIdx.x * kRlePix;
  uint8_t lab[kRlePix];
  unsigned m = rle_flags(a, img, i0, lab);
  const unsigned c = (unsigned)__popc(m);
  unsigned incl = c;  // inclusive scan over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  unsigned base = prefix + incl - c, total = 0;
#pragma unroll
  for (int w = 0; w < kRleWaves; ++w) {
    if (w < wave) base += wtot[w];
    total += wtot[w];
  }
  uint32_t* o = a.out + (size_t)b * (4 + a.cap);
#pragma unroll
  for (int j = 0; j < kRlePix; ++j) {  // static indices keep lab[] in registers
    if ((m >> j) & 1u) {
      if (base < (unsigned)a.cap) o[4 + base] = ((uint32_t)lab[j] << 24) | (uint32_t)(i0 + j);
      ++base;
    }
  }
  if (chunk == a.nchunks - 1 && threadIdx.x == 0) {
    o[0] = prefix + total;
    o[1] = (uint32_t)a.N;
    o[2] = (uint32_t)a.crop_w;
    o[3] = (uint32_t)a.crop_h;
  }
}

// Frame b's header and stored runs, words [0, 4 + min(n_runs, cap)), to the same offsets of
// dst (pinned host memory): the unused tail of the static buffer does not cross the bus.
__global__ __launch_bounds__(kRleThreads) void k_rle_copy_used(const uint32_t* __restrict__ src,
                                                               uint32_t* __restrict__ dst, int cap) {
  const size_t row = (size_t)blockIdx.y * (4 + cap);
  const unsigned n_runs = src[row];
  const int used = 4 + (int)(n_runs < (unsigned)cap ? n_runs : (unsigned)cap);
  for (int i = blockIdx.x * kRleThreads + threadIdx.x; i < used; i += gridDim.x * kRleThreads)
    dst[row + i] = src[row + i];
}

}  // namespace

int mask_rle_chunk() { return kRleChunk; }

size_t mask_rle_workspace_bytes(int B, int crop_h, int crop_w) {
  const long long N = (long long)crop_h * crop_w;
  return (size_t)B * (size_t)cdiv(N, kRleChunk) * sizeof(uint32_t);
}

void mask_rle(const MaskRleParams& p, hipStream_t s) {
  const long long N = (long long)p.crop_h * p.crop_w;
  if (p.B <= 0 || p.crop_h <= 0 || p.crop_w <= 0 || p.crop_h > p.H || p.crop_w > p.W ||
      N >= (1LL << 24) || p.cap < 2 || p.B > 65535)
    check(hipErrorInvalidValue, "mask_rle: bad shape");
  RleArgs a;
  a.labels = p.labels; a.out = p.out; a.ws = p.ws;
  a.H = p.H; a.W = p.W; a.crop_h = p.crop_h; a.crop_w = p.crop_w; a.cap = p.cap;
  a.N = (int)N; a.nchunks = cdiv(N, kRleChunk);
  const dim3 grid(a.nchunks, p.B);
  hipLaunchKernelGGL(k_rle_count, grid, dim3(kRleThreads), 0, s, a);
  hipLaunchKernelGGL(k_rle_emit, grid, dim3(kRleThreads), 0, s, a);
  check_launch("mask_rle");
}

void mask_rle_copy_used(const uint32_t* src, uint32_t* dst, int B, int cap, hipStream_t s) {
  if (B <= 0 || B > 65535 || cap < 2) check(hipErrorInvalidValue, "mask_rle_copy_used: bad shape");
  const int bx = std::min(16, cdiv(4 + cap, kRleThreads * 4));
  hipLaunchKernelGGL(k_rle_copy_used, dim3(bx, B), dim3(kRleThreads), 0, s, src, dst, cap);
  check_launch("mask_rle_copy_used");
}

}  // namespace ssa
