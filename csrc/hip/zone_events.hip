// Zone events: the enter / leave edges of the zone-presence state between consecutive frames of
// a stream (the v2 GetZoneEvents RPC; the definition is postprocess/events.py).
//
// After zone_presence with tracking on the same stream. rows[f] = uint32[4 + U K], U = 2 + 2 R,
// is the presence row that run wrote for frame f; prev of frame f is row pred[f] of the same
// buffer, or for a stream's first row of the batch (pred[f] < 0) the stream's carried state: a
// copy of the presence row of its last processed frame (all zero: no predecessor). Per frame
// out[f] = uint32[4 + 4 E]:
//   words 0-3    n_events (the true total), N, crop_w, crop_h
//   4 + 4 j      event j < min(n_events, E): slot | r << 8 | kind << 16 | edge << 24, track_id,
//                (label << 24) | root, pixels inside (ENTER, kind 1) or frames stayed (LEAVE, 2)
// Every word is written by every run, zeros past the stored events.
//
// The launches, on one stream:
//   k_ze_events   grid B, one workgroup of 256 threads (four waves) a frame; the frames are
//                 independent because k_zp_dwell has already resolved D. The track ids of both
//                 frames are staged in LDS and succ[b] is found there by a compare loop (K <= 256:
//                 at most 256 broadcast reads a thread). The candidates are the prev.n R LEAVE
//                 slots (b, r) followed by the cur.n R ENTER slots (a, r), at most 16896; the
//                 output order is the candidate order.
//                 Candidates map to lanes in 64-wide groups: wave w owns the w-th quarter of the
//                 groups, a group is 64 consecutive candidates, one a lane, so a group's reads
//                 of D are consecutive words. A group's flags are one __ballot; a lane's rank in
//                 the group is the popcount of the ballot below its lane, a wave's running offset
//                 the popcounts of its earlier groups. Pass 1 only counts: each wave's total goes
//                 to LDS, one barrier, and the exclusive sum of the four totals is the wave's
//                 base. Pass 2 re-evaluates the groups and stores the events whose position is
//                 below E. This order (rather than a contiguous chunk a thread) keeps the loads
//                 coalesced, needs two barriers a frame however many candidates there are, and a
//                 frame without an event -- almost every frame -- skips pass 2 altogether. No
//                 atomic cursor: positions depend on the candidate index alone.
//   k_ze_save     grid S, after k_ze_events (a second launch: one workgroup's read of the state
//                 and another's write of it would race inside one): the header and the n entries
//                 of the stream's last row of the batch become its state. A stream without a row
//                 keeps its state.
// Integer only, no allocation, no host sync: capturable.
#include "kernels.h"

namespace ssa {
namespace {

constexpr int kZeThreads = 256;
constexpr int kZeWaves = kZeThreads / 64;
constexpr int kZeMaxK = 256;
constexpr int kZeMaxR = 33;
constexpr int kZeMaxE = 4096;

struct ZeArgs {
  const uint32_t* rows;  // presence rows [B, 4 + U K]
  uint32_t* out;         // [B, 4 + 4 E]
  uint32_t* state;       // [S, 4 + U K]
  const int* pred;
  const int* stream;
  const int* last;
  int B, S, K, R, U, E, row_words;
};

struct ZeFrame {
  const uint32_t* prev;
  const uint32_t* cur;
  const int* succ;
  uint32_t R, U, nleave, total;
};

// candidate c of the frame: is it an event, and its four words
__device__ __forceinline__ bool ze_candidate(const ZeFrame& f, uint32_t c, uint32_t (&w)[4]) {
  if (c >= f.total) return false;
  if (c < f.nleave) {
    const uint32_t b = c / f.R, r = c - b * f.R;
    const uint32_t* e = f.prev + 4 + (size_t)f.U * b;
    const uint32_t d = e[2 + f.R + r];
    if (d == 0) return false;
    const int s = f.succ[b];
    if (s >= 0 && f.cur[4 + (size_t)f.U * s + 2 + f.R + r] != 0) return false;
    w[0] = b | r << 8 | 2u << 16 | (s < 0 ? 1u << 24 : 0u);
    w[1] = e[1]; w[2] = e[0]; w[3] = d;
    return true;
  }
  const uint32_t j = c - f.nleave, a = j / f.R, r = j - a * f.R;
  const uint32_t* e = f.cur + 4 + (size_t)f.U * a;
  if (e[2 + f.R + r] != 1) return false;
  w[0] = a | r << 8 | 1u << 16 | (e[2 + f.R] == 1 ? 1u << 24 : 0u);
  w[1] = e[1]; w[2] = e[0]; w[3] = e[2 + r];
  return true;
}

__global__ __launch_bounds__(kZeThreads) void k_ze_events(ZeArgs a) {
  __shared__ uint32_t cur_id[kZeMaxK];
  __shared__ int succ[kZeMaxK];
  __shared__ uint32_t wave_total[kZeWaves];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* cur = a.rows + (size_t)f * a.row_words;
  const int p = a.pred[f], st = a.stream[f];
  const uint32_t* prev = nullptr;  // null: no predecessor (a layout the host never builds)
  if (p >= 0 && p < a.B) prev = a.rows + (size_t)p * a.row_words;
  else if (p < 0 && st >= 0 && st < a.S) prev = a.state + (size_t)st * a.row_words;
  const uint32_t K = (uint32_t)a.K;
  const uint32_t cn = cur[0] < K ? cur[0] : K;
  const uint32_t pn = prev ? (prev[0] < K ? prev[0] : K) : 0u;
  if ((uint32_t)tid < cn) cur_id[tid] = cur[4 + (size_t)a.U * tid + 1];
  __syncthreads();
  if ((uint32_t)tid < pn) {
    const uint32_t id = prev[4 + (size_t)a.U * tid + 1];
    int s = -1;
    for (uint32_t k = 0; k < cn; ++k)
      if (cur_id[k] == id) s = (int)k;
    succ[tid] = s;
  }
  __syncthreads();
  ZeFrame fr;
  fr.prev = prev; fr.cur = cur; fr.succ = succ;
  fr.R = (uint32_t)a.R; fr.U = (uint32_t)a.U; fr.nleave = pn * fr.R; fr.total = (pn + cn) * fr.R;
  // wave w: groups [w g, (w + 1) g) of 64 candidates
  const uint32_t groups = (fr.total + 63u) / 64u, g = (groups + kZeWaves - 1) / kZeWaves;
  const uint32_t c0 = (uint32_t)wave * g * 64u + (uint32_t)lane;
  uint32_t w[4];
  uint32_t count = 0;
  for (uint32_t k = 0; k < g; ++k)  // by whole waves: every lane reaches the ballot
    count += (uint32_t)__popcll(__ballot(ze_candidate(fr, c0 + k * 64u, w)));
  if (lane == 0) wave_total[wave] = count;
  __syncthreads();
  uint32_t off = 0, n_events = 0;
  for (int k = 0; k < kZeWaves; ++k) {
    if (k < wave) off += wave_total[k];
    n_events += wave_total[k];
  }
  const uint32_t E = (uint32_t)a.E;
  uint32_t* o = a.out + (size_t)f * (4 + 4 * (size_t)a.E);
  if (n_events) {
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t k = 0; k < g && off < E; ++k) {  // off is the wave's: a uniform exit
      const bool ev = ze_candidate(fr, c0 + k * 64u, w);
      const unsigned long long m = __ballot(ev);
      const uint32_t pos = off + (uint32_t)__popcll(m & below);
      if (ev && pos < E) {
        uint32_t* d = o + 4 + 4 * (size_t)pos;
        d[0] = w[0]; d[1] = w[1]; d[2] = w[2]; d[3] = w[3];
      }
      off += (uint32_t)__popcll(m);
    }
  }
  // the header, and zeros over the words no event was stored to
  const uint32_t stored = n_events < E ? n_events : E;
  if (tid < 4) o[tid] = tid == 0 ? n_events : cur[tid];
  for (uint32_t i = 4 + 4 * stored + (uint32_t)tid; i < 4 + 4 * E; i += kZeThreads) o[i] = 0;
}

__global__ __launch_bounds__(kZeThreads) void k_ze_save(ZeArgs a) {
  const int s = blockIdx.x;
  const int l = a.last[s];
  if (l < 0 || l >= a.B) return;  // no row of this stream in the batch: its state stays
  const uint32_t* src = a.rows + (size_t)l * a.row_words;
  uint32_t* dst = a.state + (size_t)s * a.row_words;
  const uint32_t n = src[0] < (uint32_t)a.K ? src[0] : (uint32_t)a.K;
  const uint32_t used = 4 + (uint32_t)a.U * n;
  for (uint32_t i = threadIdx.x; i < used; i += kZeThreads) dst[i] = i == 0 ? n : src[i];
}

// Frame b's header and stored events, words [0, 4 + 4 min(n_events, E)), to the same offsets of
// dst (pinned host memory): a quiet frame moves four words.
__global__ __launch_bounds__(kZeThreads) void k_ze_copy_used(const uint32_t* __restrict__ src,
                                                              uint32_t* __restrict__ dst, int E) {
  const size_t row = (size_t)blockIdx.y * (4 + 4 * (size_t)E);
  const uint32_t n = src[row];
  const int used = 4 + 4 * (int)(n < (uint32_t)E ? n : (uint32_t)E);
  for (int i = blockIdx.x * kZeThreads + threadIdx.x; i < used; i += gridDim.x * kZeThreads)
    dst[row + i] = src[row + i];
}

}  // namespace

size_t zone_events_state_bytes(int streams, int K, int R) {
  return (size_t)streams * (4 + (size_t)(2 + 2 * R) * K) * sizeof(uint32_t);
}

void zone_events(const ZoneEventsParams& p, hipStream_t s) {
  if (p.B <= 0 || p.B > 65535 || p.streams <= 0 || p.streams > 65535 || p.K < 1 || p.K > kZeMaxK ||
      p.R < 1 || p.R > kZeMaxR || p.E < 1 || p.E > kZeMaxE || p.rows == nullptr || p.out == nullptr ||
      p.state == nullptr || p.pred == nullptr || p.stream == nullptr || p.last == nullptr ||
      p.out == p.rows)
    check(hipErrorInvalidValue, "zone_events: bad arguments");
  ZeArgs a;
  a.rows = p.rows; a.out = p.out; a.state = p.state; a.pred = p.pred; a.stream = p.stream; a.last = p.last;
  a.B = p.B; a.S = p.streams; a.K = p.K; a.R = p.R; a.U = 2 + 2 * p.R; a.E = p.E;
  a.row_words = 4 + a.U * p.K;
  hipLaunchKernelGGL(k_ze_events, dim3(p.B), dim3(kZeThreads), 0, s, a);
  hipLaunchKernelGGL(k_ze_save, dim3(p.streams), dim3(kZeThreads), 0, s, a);
  check_launch("zone_events");
}

void zone_events_copy_used(const uint32_t* src, uint32_t* dst, int B, int E, hipStream_t s) {
  if (B <= 0 || B > 65535 || E < 1 || E > kZeMaxE || src == nullptr || dst == nullptr)
    check(hipErrorInvalidValue, "zone_events_copy_used: bad shape");
  const int bx = std::min(16, cdiv(4 + 4 * E, kZeThreads * 4));
  hipLaunchKernelGGL(k_ze_copy_used, dim3(bx, B), dim3(kZeThreads), 0, s, src, dst, E);
  check_launch("zone_events_copy_used");
}

}  // namespace ssa
