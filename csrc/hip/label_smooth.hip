// Spatial label smoothing (--smooth_labels; the definition is postprocess/smooth.py): a windowed
// majority filter of the label maps, the first launch of the post-processing chain.
//
// Per frame and per pixel p of the crop, over the (2R+1) x (2R+1) window clipped to the crop:
// the output is the centre's label when no label has more votes than it, else the smallest of
// the labels with the most votes. With confidence planes an unchanged pixel keeps its code and a
// changed one gets the floor mean of the codes of the winning voters. Pixels of the H x W plane
// outside the crop pass through. Out of place: a stencil cannot run in place.
//
// One launch, grid (tiles_x, tiles_y, B) over the whole plane, so every output byte is written.
// A workgroup stages its kSmTW x kSmTH tile plus an R-wide halo in LDS, the labels as 16-bit
// words: positions outside the crop hold kSmOut, which equals no label, so they neither vote nor
// become candidates. The frame stride H * W and the row stride W may be odd: the planes are
// read and written byte by byte, a wave a row segment of 64 consecutive bytes.
//   uniform tile    every staged crop pixel carries one label (ballot, one LDS flag): the tile
//                   is copied through with no per-pixel pass.
//   majority window the centre's label has at least half of the window's votes (a uniform
//                   window is the common case): the centre stays, nothing else is counted.
//   counting        the window sits in registers; the labels still present are taken in
//                   ascending order (a min over the window), counted and struck out, and a label
//                   replaces the best only with strictly more votes -- the centre first, so it
//                   wins its ties and the smallest label wins the others. The walk ends as soon
//                   as the votes left cannot beat the best.
// A thread owns a column of kSmRows outputs. Integer only, no atomics, no allocation, no host
// sync: capturable.
#include "kernels.h"

namespace ssa {
namespace {

constexpr int kSmThreads = 256;
constexpr int kSmTW = 64, kSmTH = 32;
constexpr int kSmRows = kSmTH / (kSmThreads / kSmTW);  // outputs per thread, one below the other
constexpr uint32_t kSmOut = 0x100;                     // staged outside the crop: no uint8 label

struct SmArgs {
  const uint8_t* lin;
  uint8_t* lout;
  const uint8_t* cin;
  uint8_t* cout;
  int H, W, crop_h, crop_w;
};

template <int R, bool CONF>
__global__ __launch_bounds__(kSmThreads) void k_label_smooth(SmArgs a) {
  constexpr int SW = kSmTW + 2 * R, SH = kSmTH + 2 * R, D = 2 * R + 1, NW = D * D;
  __shared__ uint16_t sl[SH * SW];
  __shared__ uint8_t sk[CONF ? SH * SW : 1];
  __shared__ int mixed;
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kSmTW, ty0 = blockIdx.y * kSmTH;
  const size_t base = (size_t)blockIdx.z * (size_t)a.H * (size_t)a.W;
  const uint8_t* lin = a.lin + base;
  uint8_t* lout = a.lout + base;
  const uint8_t* cin = CONF ? a.cin + base : nullptr;
  uint8_t* cout = CONF ? a.cout + base : nullptr;
  const bool has_crop = tx0 < a.crop_w && ty0 < a.crop_h;  // else every pixel of the tile is pad

  if (tid == 0) mixed = 0;
  __syncthreads();
  if (has_crop) {
    const uint32_t ref = lin[(size_t)ty0 * a.W + tx0];  // the tile's first pixel: inside the crop
    bool diff = false;
    for (int i = tid; i < SH * SW; i += kSmThreads) {
      const int ry = i / SW, rx = i - ry * SW;
      const int gy = ty0 - R + ry, gx = tx0 - R + rx;
      uint32_t v = kSmOut, k = 0;
      if ((unsigned)gy < (unsigned)a.crop_h && (unsigned)gx < (unsigned)a.crop_w) {
        const size_t o = (size_t)gy * a.W + gx;
        v = lin[o];
        if (CONF) k = cin[o];
        diff |= v != ref;
      }
      sl[i] = (uint16_t)v;
      if (CONF) sk[i] = (uint8_t)k;
    }
    if (__ballot(diff) != 0ull && (tid & 63) == 0) mixed = 1;
  }
  __syncthreads();
  const bool mix = mixed != 0;

  const int lx = tid % kSmTW, ly0 = (tid / kSmTW) * kSmRows;
  const int gx = tx0 + lx;
  if (gx >= a.W) return;
  const int nx = min(gx + R, a.crop_w - 1) - max(gx - R, 0) + 1;  // window columns inside the crop
#pragma unroll 1
  for (int r = 0; r < kSmRows; ++r) {
    const int ly = ly0 + r, gy = ty0 + ly;
    if (gy >= a.H) break;
    const size_t o = (size_t)gy * a.W + gx;
    if (gx >= a.crop_w || gy >= a.crop_h) {  // a pad pixel passes
      lout[o] = lin[o];
      if (CONF) cout[o] = cin[o];
      continue;
    }
    const int ci = (ly + R) * SW + lx + R;
    const uint32_t c0 = sl[ci];
    uint32_t out = c0, kout = CONF ? sk[ci] : 0u;
    if (mix) {
      uint32_t w[NW];
#pragma unroll
      for (int dy = 0; dy < D; ++dy)
#pragma unroll
        for (int dx = 0; dx < D; ++dx) w[dy * D + dx] = sl[ci + (dy - R) * SW + (dx - R)];
      const uint32_t nvalid = (uint32_t)(nx * (min(gy + R, a.crop_h - 1) - max(gy - R, 0) + 1));
      uint32_t vc = 0;
#pragma unroll
      for (int i = 0; i < NW; ++i) vc += w[i] == c0 ? 1u : 0u;
      if (2 * vc < nvalid) {  // otherwise no label can have more votes than the centre's
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = w[i] == c0 ? kSmOut : w[i];
        uint32_t best_v = vc, best_c = c0, rem = nvalid - vc;
        while (rem > best_v) {
          uint32_t c = kSmOut;  // the smallest label still present
#pragma unroll
          for (int i = 0; i < NW; ++i) c = min(c, w[i]);
          uint32_t v = 0;
#pragma unroll
          for (int i = 0; i < NW; ++i) {
            const bool e = w[i] == c;
            v += e ? 1u : 0u;
            w[i] = e ? kSmOut : w[i];
          }
          rem -= min(v, rem);
          if (v > best_v) {
            best_v = v;
            best_c = c;
          }
        }
        if (best_c != c0) {
          out = best_c;
          if (CONF) {  // the floor mean of the winning voters' codes
            uint32_t sum = 0;
#pragma unroll
            for (int dy = 0; dy < D; ++dy)
#pragma unroll
              for (int dx = 0; dx < D; ++dx) {
                const int q = ci + (dy - R) * SW + (dx - R);
                sum += sl[q] == best_c ? (uint32_t)sk[q] : 0u;
              }
            kout = sum / best_v;
          }
        }
      }
    }
    lout[o] = (uint8_t)out;
    if (CONF) cout[o] = (uint8_t)kout;
  }
}

template <int R>
void launch(const SmArgs& a, bool conf, dim3 grid, hipStream_t s) {
  if (conf)
    hipLaunchKernelGGL((k_label_smooth<R, true>), grid, dim3(kSmThreads), 0, s, a);
  else
    hipLaunchKernelGGL((k_label_smooth<R, false>), grid, dim3(kSmThreads), 0, s, a);
}

}  // namespace

int label_smooth_tile_w() { return kSmTW; }
int label_smooth_tile_h() { return kSmTH; }

void label_smooth(const LabelSmoothParams& p, hipStream_t s) {
  const long long HW = (long long)p.H * p.W;
  if (p.B <= 0 || p.B > 65535 || p.H <= 0 || p.W <= 0 || p.crop_h <= 0 || p.crop_w <= 0 ||
      p.crop_h > p.H || p.crop_w > p.W || HW >= (1LL << 31) || cdiv(p.H, kSmTH) > 65535 ||
      p.R < 1 || p.R > 3 || p.labels_in == nullptr || p.labels_out == nullptr ||
      p.labels_in == p.labels_out || (p.conf_in == nullptr) != (p.conf_out == nullptr) ||
      (p.conf_in != nullptr && p.conf_in == p.conf_out))
    check(hipErrorInvalidValue, "label_smooth: bad shape");
  SmArgs a;
  a.lin = p.labels_in; a.lout = p.labels_out; a.cin = p.conf_in; a.cout = p.conf_out;
  a.H = p.H; a.W = p.W; a.crop_h = p.crop_h; a.crop_w = p.crop_w;
  const dim3 grid(cdiv(p.W, kSmTW), cdiv(p.H, kSmTH), p.B);
  const bool conf = p.conf_in != nullptr;
  if (p.R == 1) launch<1>(a, conf, grid, s);
  else if (p.R == 2) launch<2>(a, conf, grid, s);
  else launch<3>(a, conf, grid, s);
  check_launch("label_smooth");
}

}  // namespace ssa
