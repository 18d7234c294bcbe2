// Temporal label stabilisation (--stable_labels; the definition is postprocess/stable.py): a
// per-pixel debounce of the label maps at the head of the post-processing chain.
//
// Per stream and per flat pixel i = y * crop_w + x of the crop the state word is
// s | c << 8 | n << 16 | h << 24: the stable label, the candidate, the consecutive frames the
// candidate has been seen (0 <= n < N) and the confidence code with which s last won. A frame
// with raw label r and raw code k (0 without confidence planes) updates it in this order:
//   stream not started   s = c = r, n = 0, h = k
//   r == s               c = s, n = 0, h = k
//   g > 0 and k < g      a doubtful observation: nothing changes
//   otherwise            r == c ? ++n : (c = r, n = 1); at n >= N: s = c = r, n = 0, h = k
// and the frame's output is (s, h) after the update. Pixels of the H x W plane outside the crop
// have no state and pass through.
//
// state: per stream [header | N words], 1 + N words a stream; header bit 0: started, all zero: a
// reset. One launch, grid (pixel chunks, streams). A thread owns kLsPix consecutive crop pixels:
// it loads their words once, walks the stream's rows of the batch (first[s], count[s] of the
// device table, the layout of feeder.split_batch) in order with the fields in registers, and
// stores the words once. The byte loads do not depend on the state, only the few integer
// operations of the update chain do: the frames go in groups of kLsFrames, and the loads of the
// next group are issued before the updates and stores of this one (two register buffers), so the
// walk waits for memory once per group and not once per frame. The frame stride H * W and the
// row stride W may be odd, so the planes are read and written byte by byte; a thread reads its
// bytes of a frame before it writes them, and no thread reads another's, so out may be in. Out
// of place, further chunks copy the pad pixels.
//
// The header: every workgroup reads `started` when it begins. The one that takes the stream's
// last ticket (the header's upper bits, one atomic add per workgroup after its walk) stores
// header = 1, so `started` cannot change under a workgroup of the same launch that is scheduled
// late. A stream with no row in the batch touches nothing.
// Integer only, no LDS, no allocation, no host sync: capturable.
#include "kernels.h"

namespace ssa {
namespace {

constexpr int kLsThreads = 256;
constexpr int kLsPix = 2;     // consecutive crop pixels per thread
constexpr int kLsChunk = kLsThreads * kLsPix;
constexpr int kLsFrames = 4;  // frames per group; two groups' bytes are in flight (see the walk)

struct LsArgs {
  const uint8_t* lin;
  uint8_t* lout;
  const uint8_t* cin;
  uint8_t* cout;
  uint32_t* state;
  const int* tables;  // first[S] | count[S]
  int B, S, H, W, crop_h, crop_w, N, frames, g, crop_chunks, pad;
};

struct __attribute__((aligned(4))) LsWords { uint32_t w[kLsPix]; };  // words are 4-byte aligned

template <bool CONF>
__global__ __launch_bounds__(kLsThreads) void k_label_stable(LsArgs a) {
  const int s = blockIdx.y;
  const int first = a.tables[s], cnt = a.tables[a.S + s];
  if (cnt <= 0 || first < 0 || first > a.B - cnt) return;  // no row: nothing is touched
  uint32_t* hdr = a.state + (size_t)s * (size_t)(1 + a.N);
  const bool started = (__atomic_load_n(hdr, __ATOMIC_RELAXED) & 1u) != 0;
  const size_t HW = (size_t)a.H * a.W;
  const size_t base = (size_t)first * HW;
  const int tid = threadIdx.x;

  if ((int)blockIdx.x < a.crop_chunks) {
    const int i0 = blockIdx.x * kLsChunk + tid * kLsPix;
    if (i0 < a.N) {
      const int nv = min(kLsPix, a.N - i0);
      uint32_t* wp = hdr + 1 + i0;
      uint32_t sv[kLsPix], cv[kLsPix], nn[kLsPix], hv[kLsPix];
      int off[kLsPix];
      LsWords w;
      if (nv == kLsPix) {
        w = *reinterpret_cast<const LsWords*>(wp);
      } else {
#pragma unroll
        for (int p = 0; p < kLsPix; ++p) w.w[p] = p < nv ? wp[p] : 0u;
      }
      int y = i0 / a.crop_w, x = i0 - y * a.crop_w;
#pragma unroll
      for (int p = 0; p < kLsPix; ++p) {
        sv[p] = w.w[p] & 0xffu;
        cv[p] = (w.w[p] >> 8) & 0xffu;
        nn[p] = (w.w[p] >> 16) & 0xffu;
        hv[p] = w.w[p] >> 24;
        off[p] = y * a.W + x;  // pixels past nv: an address inside the crop, never used
        if (p + 1 < nv && ++x == a.crop_w) {
          x = 0;
          ++y;
        }
      }
      bool st = started;
      // the bytes of the group of frames from t0 on; frames past the stream's rows: zeros, unread
      auto load = [&](uint32_t (&r)[kLsFrames][kLsPix], uint32_t (&k)[kLsFrames][kLsPix], int t0) {
#pragma unroll
        for (int f = 0; f < kLsFrames; ++f) {
          const size_t at = base + (size_t)(t0 + f) * HW;
#pragma unroll
          for (int p = 0; p < kLsPix; ++p) {
            const bool on = t0 + f < cnt && p < nv;
            r[f][p] = on ? a.lin[at + off[p]] : 0u;
            k[f][p] = CONF && on ? a.cin[at + off[p]] : 0u;
          }
        }
      };
      // the updates of that group in frame order, and its outputs
      auto update = [&](const uint32_t (&r)[kLsFrames][kLsPix], const uint32_t (&k)[kLsFrames][kLsPix],
                        int t0) {
#pragma unroll
        for (int f = 0; f < kLsFrames; ++f) {
          if (t0 + f >= cnt) break;
          const size_t at = base + (size_t)(t0 + f) * HW;
#pragma unroll
          for (int p = 0; p < kLsPix; ++p) {
            const uint32_t rr = r[f][p], kk = k[f][p];
            if (!st) {
              sv[p] = cv[p] = rr; nn[p] = 0; hv[p] = kk;
            } else if (rr == sv[p]) {
              cv[p] = rr; nn[p] = 0; hv[p] = kk;
            } else if (!(a.g > 0 && kk < (uint32_t)a.g)) {
              if (rr == cv[p]) {
                ++nn[p];
              } else {
                cv[p] = rr; nn[p] = 1;
              }
              if (nn[p] >= (uint32_t)a.frames) {
                sv[p] = rr; nn[p] = 0; hv[p] = kk;
              }
            }
            if (p < nv) {
              a.lout[at + off[p]] = (uint8_t)sv[p];
              if (CONF) a.cout[at + off[p]] = (uint8_t)hv[p];
            }
          }
          st = true;
        }
      };
      // two register buffers: the next group's loads are in flight under this group's updates
      // and stores (other frames, so in place is safe)
      uint32_t ra[kLsFrames][kLsPix], ka[kLsFrames][kLsPix], rb[kLsFrames][kLsPix], kb[kLsFrames][kLsPix];
      load(ra, ka, 0);
      for (int t0 = 0; t0 < cnt; t0 += 2 * kLsFrames) {
        load(rb, kb, t0 + kLsFrames);
        update(ra, ka, t0);
        load(ra, ka, t0 + 2 * kLsFrames);
        update(rb, kb, t0 + kLsFrames);
      }
#pragma unroll
      for (int p = 0; p < kLsPix; ++p) w.w[p] = sv[p] | cv[p] << 8 | nn[p] << 16 | hv[p] << 24;
      if (nv == kLsPix) {
        *reinterpret_cast<LsWords*>(wp) = w;
      } else {
#pragma unroll
        for (int p = 0; p < kLsPix; ++p)
          if (p < nv) wp[p] = w.w[p];
      }
    }
  } else {
    // out of place only: the pad pixels, right of the crop first, then the rows below it
    const int right = a.crop_h * (a.W - a.crop_w);
    const int j0 = ((int)blockIdx.x - a.crop_chunks) * kLsChunk + tid * kLsPix;
#pragma unroll
    for (int p = 0; p < kLsPix; ++p) {
      const int j = j0 + p;
      if (j >= a.pad) break;
      int o;
      if (j < right) {
        const int y = j / (a.W - a.crop_w);
        o = y * a.W + a.crop_w + (j - y * (a.W - a.crop_w));
      } else {
        o = a.crop_h * a.W + (j - right);
      }
      for (int t = 0; t < cnt; ++t) {
        const size_t at = base + (size_t)t * HW + o;
        a.lout[at] = a.lin[at];
        if (CONF) a.cout[at] = a.cin[at];
      }
    }
  }
  __syncthreads();  // every thread of the workgroup has read the header
  if (tid == 0) {
    const uint32_t old = atomicAdd(hdr, 2u);
    if ((old >> 1) == gridDim.x - 1) atomicExch(hdr, 1u);  // the last ticket: started, no tickets
  }
}

}  // namespace

int label_stable_chunk() { return kLsChunk; }

size_t label_stable_state_bytes(int streams, int crop_h, int crop_w) {
  return (size_t)streams * (1 + (size_t)crop_h * crop_w) * 4;
}

void label_stable(const LabelStableParams& p, hipStream_t s) {
  const long long N = (long long)p.crop_h * p.crop_w, HW = (long long)p.H * p.W;
  if (p.B <= 0 || p.streams <= 0 || p.streams > 65535 || p.crop_h <= 0 || p.crop_w <= 0 ||
      p.crop_h > p.H || p.crop_w > p.W || HW >= (1LL << 31) || p.frames < 2 || p.frames > 255 ||
      p.g < 0 || p.g > 255 || p.labels_in == nullptr || p.labels_out == nullptr ||
      (p.conf_in == nullptr) != (p.conf_out == nullptr) || (p.g > 0 && p.conf_in == nullptr) ||
      p.state == nullptr || p.tables == nullptr)
    check(hipErrorInvalidValue, "label_stable: bad shape");
  const bool copy = p.labels_out != p.labels_in || p.conf_out != p.conf_in;
  LsArgs a;
  a.lin = p.labels_in; a.lout = p.labels_out; a.cin = p.conf_in; a.cout = p.conf_out;
  a.state = p.state; a.tables = p.tables;
  a.B = p.B; a.S = p.streams; a.H = p.H; a.W = p.W; a.crop_h = p.crop_h; a.crop_w = p.crop_w;
  a.N = (int)N; a.frames = p.frames; a.g = p.g;
  a.crop_chunks = (int)cdiv(N, kLsChunk);
  a.pad = copy ? (int)(HW - N) : 0;
  const dim3 grid(a.crop_chunks + (int)cdiv(a.pad, kLsChunk), p.streams);
  if (p.conf_in)
    hipLaunchKernelGGL(k_label_stable<true>, grid, dim3(kLsThreads), 0, s, a);
  else
    hipLaunchKernelGGL(k_label_stable<false>, grid, dim3(kLsThreads), 0, s, a);
  check_launch("label_stable");
}

}  // namespace ssa
