// Packed 4:2:2 camera frames (YUYV: Y0 U Y1 V, UYVY: U Y0 V Y1) -> BGR on the device, the
// first kernel of a step when the server ingests raw frames (--pixel_format yuyv | uyvy).
// Bit-identical to the host conversion (csrc/host/v4l2.cpp, px2): BT.601 limited range in
// 20-bit fixed point, int32 throughout, arithmetic shift, saturation to 0..255.
//
// A macropixel (4 bytes in, 6 bytes out: B G R B G R) does not depend on its row, so a
// contiguous (B, H, W, 2) tensor with even W is a flat stream of B * H * W / 2 macropixels.
// Memory-bound: a lane converts 8 macropixels per iteration, 32 B in as two 16-byte loads
// and 48 B out as three 16-byte stores, grid-stride over at most 2048 blocks, no LDS.
//
// Alignment. src is 4-byte aligned (a multiple of a macropixel), dst 2-byte aligned (a batch
// slice of a torch allocation starts at a multiple of 6 bytes). The 16-byte body starts after
// `head` macropixels, where both src + 4 * head and dst + 6 * head are 16-byte aligned; with
// src = 4a and dst = 2b that is head = -a (mod 4) and head = -3b (mod 8), which agree iff
// a + b = 0 (mod 4) -- always so for the same batch slice of two 16-byte-aligned allocations
// (a = iM, b = 3iM). The head, the tail past the last whole group of 8 and, when the two
// alignments disagree, the whole stream take the narrow path: one dword load and three
// 2-byte stores per macropixel.
#include <algorithm>

#include "kernels.h"

namespace ssa {

namespace {

constexpr int kCY = 1220542, kCUB = 2116026, kCUG = -409993, kCVG = -852492, kCVR = 1673527;
constexpr int kShift = 20, kHalf = 1 << (kShift - 1);
constexpr int kGroup = 8;  // macropixels per lane per iteration of the 16-byte body

// sat8(v >> kShift) of the host code, as a clamp of the unshifted sum and a logical shift (the
// same value: v < 0 -> 0, v >= 256 << kShift -> 255, else the floor). Written as shift-then-
// clamp, hipcc (ROCm 7) selects v_ashr_pk_u8_i32 for each pair of bytes and ORs its result
// into the packed dword unmasked, but on the MI355X the instruction left the destination
// register's previous upper 16 bits in place: neighbouring bytes came out ORed with stale
// bits of a sum (G0 of every odd macropixel read 255 after a negative sum).
__device__ __forceinline__ uint32_t sat8(int v) {
  return (uint32_t)min(max(v, 0), (256 << kShift) - 1) >> kShift;
}

// One macropixel (the 4 packed bytes as a little-endian dword) -> lo = B0 G0 R0 B1 (byte 0
// first), hi = G1 R1 in its low 16 bits.
template <bool UYVY>
__device__ __forceinline__ void px2(uint32_t w, uint32_t& lo, uint32_t& hi) {
  const int b0 = w & 255, b1 = (w >> 8) & 255, b2 = (w >> 16) & 255, b3 = w >> 24;
  const int y0 = UYVY ? b1 : b0, u = UYVY ? b0 : b1, y1 = UYVY ? b3 : b2, v = UYVY ? b2 : b3;
  const int du = u - 128, dv = v - 128;
  const int ruv = kHalf + kCVR * dv, guv = kHalf + kCVG * dv + kCUG * du, buv = kHalf + kCUB * du;
  const int c0 = max(y0 - 16, 0) * kCY, c1 = max(y1 - 16, 0) * kCY;
  lo = sat8(c0 + buv) | sat8(c0 + guv) << 8 | sat8(c0 + ruv) << 16 | sat8(c1 + buv) << 24;
  hi = sat8(c1 + guv) | sat8(c1 + ruv) << 8;
}

// Macropixels [0, head) and [head + 8 * nvec, n) narrow, [head, head + 8 * nvec) in groups of
// 8; src + 4 * head and dst + 6 * head are 16-byte aligned when nvec > 0.
template <bool UYVY>
__global__ __launch_bounds__(256) void yuv422_kernel(const uint8_t* __restrict__ src,
                                                     uint8_t* __restrict__ dst, size_t n, size_t head,
                                                     size_t nvec) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const uint4* __restrict__ vs = reinterpret_cast<const uint4*>(src + 4 * head);
  uint4* __restrict__ vd = reinterpret_cast<uint4*>(dst + 6 * head);
  for (size_t g = gid; g < nvec; g += stride) {
    const uint4 a = vs[2 * g], b = vs[2 * g + 1];
    const uint32_t w[kGroup] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t o[12];
#pragma unroll
    for (int p = 0; p < kGroup / 2; ++p) {  // two macropixels -> three dwords
      uint32_t lo0, hi0, lo1, hi1;
      px2<UYVY>(w[2 * p], lo0, hi0);
      px2<UYVY>(w[2 * p + 1], lo1, hi1);
      o[3 * p] = lo0;
      o[3 * p + 1] = hi0 | lo1 << 16;
      o[3 * p + 2] = lo1 >> 16 | hi1 << 16;
    }
    vd[3 * g] = make_uint4(o[0], o[1], o[2], o[3]);
    vd[3 * g + 1] = make_uint4(o[4], o[5], o[6], o[7]);
    vd[3 * g + 2] = make_uint4(o[8], o[9], o[10], o[11]);
  }
  const size_t body = kGroup * nvec, narrow = n - body;
  for (size_t t = gid; t < narrow; t += stride) {
    const size_t m = t < head ? t : t + body;
    uint32_t lo, hi;
    px2<UYVY>(*reinterpret_cast<const uint32_t*>(src + 4 * m), lo, hi);
    uint16_t* d = reinterpret_cast<uint16_t*>(dst + 6 * m);
    d[0] = (uint16_t)lo;
    d[1] = (uint16_t)(lo >> 16);
    d[2] = (uint16_t)hi;
  }
}

}  // namespace

void yuv422_to_bgr(const uint8_t* src, uint8_t* dst, size_t n_macropixels, bool uyvy, hipStream_t s) {
  const uintptr_t sa = (uintptr_t)src, da = (uintptr_t)dst;
  if (!src || !dst || sa % 4 || da % 2)
    throw std::invalid_argument("yuv422_to_bgr: src must be 4-byte and dst 2-byte aligned");
  if (n_macropixels < 1) throw std::invalid_argument("yuv422_to_bgr: no macropixels");
  const size_t n = n_macropixels;
  const unsigned a = (unsigned)(sa / 4) % 4, b = (unsigned)(da / 2) % 8;
  size_t head = 0, nvec = 0;
  if ((a + b) % 4 == 0) {  // one head aligns both streams
    head = std::min<size_t>((8 - 3 * b % 8) % 8, n);
    nvec = (n - head) / kGroup;
    if (nvec == 0) head = 0;  // all narrow
  }
  const size_t work = std::max(nvec, n - kGroup * nvec);
  const int grid = (int)std::min<size_t>(2048, (work + 255) / 256);
  if (uyvy)
    hipLaunchKernelGGL(yuv422_kernel<true>, dim3(grid), dim3(256), 0, s, src, dst, n, head, nvec);
  else
    hipLaunchKernelGGL(yuv422_kernel<false>, dim3(grid), dim3(256), 0, s, src, dst, n, head, nvec);
  check_launch("yuv422_to_bgr");
}

}  // namespace ssa
