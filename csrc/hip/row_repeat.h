// Constant letterbox rows, computed once (stem_band.hip, fused_ir_slice.hip).
//
// The letterbox pads bottom / right: model-input rows [p0, H) with lut_y == -1 are the
// constant -1 across the full width. The front layers are 3x3 pad-1 conv chains that run
// the same arithmetic for every row, so an output row whose whole vertical receptive field
// lies in [p0, H - 1] is bit-identical to the row above it. Such a run of output rows
// [z0, z1) is computed once (row z0) and stored z1 - z0 times.
//
// The zone is derived on the device from the LUT in use (the plan is keyed by the camera
// size only; the LUT arrives per call), and the band layout is made in the compressed row
// space -- the rows that still need computing, [0, z0] u [z1, OH) -- so every workgroup of
// the unchanged launch grid gets an equal share of the remaining work.
// Python mirror of the arithmetic: ops/row_repeat.py.
#pragma once
#include "common.h"

namespace ssa {

// Output rows z0 + 1 .. z0 + nrep are copies of row z0 (z0 = -1, nrep = 0: no zone).
struct RowZone {
  int z0, nrep;
};

// Start of the trailing run of pad rows: 1 + max{ y : lut_y[y] != -1 }, 0 if there is none.
// Every wave scans the whole LUT itself (H / 64 independent clamped loads per lane, issued
// back to back: one memory round trip, no LDS, no barrier); the result is wave-uniform.
__device__ __forceinline__ int pad_start(const int32_t* lut_y, int H, int lane) {
  constexpr int UN = 9;  // 9 x 64 lanes cover H <= 576 in one trip
  int m = 0;
  for (int base = 0; base < H; base += 64 * UN) {
    int v[UN], y[UN];
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      y[k] = min(base + k * 64 + lane, H - 1);  // clamped: a row counted twice changes no max
      v[k] = lut_y[y[k]];
    }
#pragma unroll
    for (int k = 0; k < UN; ++k) m = max(m, v[k] != -1 ? y[k] + 1 : 0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  return __builtin_amdgcn_readfirstlane(m);
}

// Output row o of a layer with cumulative vertical receptive field (s, a, b) reads
// model-input rows [s o - a, s o + b]; rows at or past H are zero padding, not -1, so the
// zone is the rows with s o - a >= p0 and s o + b <= H - 1. Fewer than 2 rows: no zone.
__device__ __forceinline__ RowZone row_zone(int p0, int H, int OH, int s, int a, int b) {
  RowZone z{-1, 0};
  if (s < 1 || H - 1 - b < 0) return z;
  const int z0 = (p0 + a + s - 1) / s;
  const int z1 = min(OH, (H - 1 - b) / s + 1);
  if (z1 - z0 >= 2) {
    z.z0 = z0;
    z.nrep = z1 - z0 - 1;
  }
  return z;
}

// Band by of nby takes compressed rows [by R', (by + 1) R'), R' = ceil(Nc / nby) <= R with
// Nc = OH - nrep rows to compute. Mapped back to real rows that is at most two contiguous
// segments: seg 0 = the rows up to and including z0, seg 1 = the rows from z1 on (without a
// zone everything is seg 1). y0 >= y1: the segment is empty.
struct BandSegs {
  int y0[2], y1[2];
};

__device__ __forceinline__ BandSegs band_segments(const RowZone& z, int OH, int R, int nby, int by) {
  const int nc = OH - z.nrep;
  const int rp = z.nrep ? (nc + nby - 1) / nby : R;  // no zone: the bands of R rows as they were
  const int c0 = by * rp, c1 = min(c0 + rp, nc);
  BandSegs s;
  s.y0[0] = c0;
  s.y1[0] = min(c1, z.z0 + 1);
  s.y0[1] = max(c0, z.z0 + 1) + z.nrep;
  s.y1[1] = c1 + z.nrep;
  return s;
}

}  // namespace ssa
