// Zone presence of the stored class regions (the v2 GetZonePresence RPC; the definition is
// postprocess/presence.py).
//
// After class_regions (and, with tracking, region_tracks) on the same stream. S[b][i] is the
// uint16 slot plane of frame b: the rank of the stored region that holds flat crop pixel i,
// 0xFFFF for none. With n = min(n_regions, K) stored regions, R = 1 + Z zone rows (row 0: the
// whole crop) and the zone plane (uint32[N], bit z - 1: pixel i is in user zone z; shared by the
// frames), per frame out[b] = uint32[4 + U K], U = 2 + R, or 2 + 2 R with tracking:
//   words 0-3            n, N, crop_w, crop_h
//   4 + U a              (label << 24) | root of stored region a < n (its record's first word)
//   4 + U a + 1          track_id (0 without tracking)
//   4 + U a + 2 + r      P[a][r] = #{ i : S[i] == a and (r == 0 or bit r - 1 of plane[i]) }
//   4 + U a + 2 + R + r  D[a][r], with tracking: the dwell of a's track in row r
// Every word is written by every run, zeros past entry n.
//
// The launches, on one stream:
//   (slot planes)  with tracking they are the ones k_tr_slots wrote; without, class_regions.hip
//                  resolves them from its workspace into this file's own workspace
//   k_zp_init      header, first entry words and zeros over the whole row of every frame
//   k_zp_count     grid (chunks of kZpChunk flat pixels, B): a workgroup-private [n][R] table in
//                  LDS, filled by run aggregation as in zone_stats.hip with the slot as the key
//                  -- among the 64 consecutive pixels of a wave the first lane of each run of
//                  equal (slot, plane word) adds the run's length once for row 0 and once per
//                  set zone bit -- then the non-zero counters are added to the frame's row with
//                  integer global atomics. Pixels without a slot have no key.
//   k_zp_dwell     with tracking: one workgroup per stream, its frames in batch order, one
//                  barrier a frame; the threads run over the (a, r) pairs. D of a frame is read
//                  from the previous frame's row of `out` (for the first frame of the batch: the
//                  stream's carried state [K][R]); the last frame's D becomes the state. A stream
//                  without a row in the batch keeps its state; all zero is a reset.
// Integer adds commute: the words are exact. No float arithmetic, no allocation, no host sync:
// capturable.
#include "kernels.h"

namespace ssa {
namespace {

constexpr int kZpThreads = 256;
constexpr int kZpPix = 32;  // flat pixels per thread: 32 wave rows of 64 consecutive pixels
constexpr int kZpChunk = kZpThreads * kZpPix;
constexpr int kZpMaxK = 256;
constexpr int kZpMaxR = 33;
constexpr uint32_t kZpNone = 0xFFFFFFFFu;

struct ZpArgs {
  const uint32_t* rows;   // region rows [B, 4 + RW K]
  const uint16_t* slots;  // [B][slot_stride]
  const uint32_t* plane;
  const uint32_t* links;  // [B][K], tracking only
  uint32_t* out;
  uint32_t* state;        // [S][K][R], tracking only
  const int* pred;
  const int* last;
  size_t slot_stride;     // uint16 elements between the planes of two frames
  int K, R, U, RW, N, crop_w, crop_h, row_words;
  uint32_t zmask, q;
};

__device__ __forceinline__ uint32_t zp_stored(const ZpArgs& a, int b) {  // min(n_regions, K)
  const uint32_t n = a.rows[(size_t)b * (4 + a.RW * a.K)];
  return n < (uint32_t)a.K ? n : (uint32_t)a.K;
}

__global__ __launch_bounds__(kZpThreads) void k_zp_init(ZpArgs a) {
  const int i = blockIdx.x * kZpThreads + threadIdx.x, b = blockIdx.y;
  if (i >= a.row_words) return;
  const uint32_t n = zp_stored(a, b);
  uint32_t v = 0;
  if (i == 0) v = n;
  else if (i == 1) v = (uint32_t)a.N;
  else if (i == 2) v = (uint32_t)a.crop_w;
  else if (i == 3) v = (uint32_t)a.crop_h;
  else {
    const uint32_t e = (uint32_t)(i - 4) / (uint32_t)a.U;
    if ((uint32_t)(i - 4) == e * (uint32_t)a.U && e < n)
      v = a.rows[(size_t)b * (4 + a.RW * a.K) + 4 + (size_t)a.RW * e];
  }
  a.out[(size_t)b * a.row_words + i] = v;
}

__global__ __launch_bounds__(kZpThreads) void k_zp_count(ZpArgs a) {
  __shared__ uint32_t tab[kZpMaxK * kZpMaxR];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const uint32_t n = zp_stored(a, b);
  if (n == 0) return;  // by the whole block
  const int used = (int)n * a.R;
  for (int j = tid; j < used; j += kZpThreads) tab[j] = 0;
  __syncthreads();
  const uint16_t* S = a.slots + (size_t)b * a.slot_stride;
  // a wave: kZpPix rows of 64 consecutive flat pixels
  int i = blockIdx.x * kZpChunk + (tid >> 6) * (64 * kZpPix) + lane;
#pragma unroll 4
  for (int k = 0; k < kZpPix; ++k, i += 64) {
    uint32_t slot = kZpNone, word = 0;  // past the crop, or in no stored region: no key
    if (i < a.N) {
      const uint32_t s = S[i];
      if (s < n) {
        slot = s;
        if (a.plane) word = a.plane[i] & a.zmask;
      }
    }
    // by every lane, before any branch
    const uint32_t lslot = (uint32_t)__shfl_up((int)slot, 1, 64);
    const uint32_t lword = (uint32_t)__shfl_up((int)word, 1, 64);
    const bool head = lane == 0 || lslot != slot || lword != word;
    const unsigned long long heads = __ballot(head);
    if (!head || slot == kZpNone) continue;
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    const uint32_t len = after ? (uint32_t)__ffsll((long long)after) : (uint32_t)(64 - lane);
    uint32_t* t = tab + slot * (uint32_t)a.R;
    atomicAdd(t, len);
    while (word) {
      const int r = __ffs((int)word);  // 1-based bit: the zone's row
      word &= word - 1;
      atomicAdd(t + r, len);
    }
  }
  __syncthreads();
  uint32_t* o = a.out + (size_t)b * a.row_words + 4 + 2;
  for (int j = tid; j < used; j += kZpThreads) {
    const uint32_t v = tab[j];
    if (v) {
      const uint32_t e = (uint32_t)j / (uint32_t)a.R, r = (uint32_t)j - e * (uint32_t)a.R;
      atomicAdd(o + (size_t)e * a.U + r, v);
    }
  }
}

__global__ __launch_bounds__(kZpThreads) void k_zp_dwell(ZpArgs a) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const int r1 = a.last[s];
  if (r1 < 0) return;  // no row of this stream in the batch: its state stays
  int r0 = r1;
  while (a.pred[r0] >= 0) r0 = a.pred[r0];
  uint32_t* st = a.state + (size_t)s * a.K * a.R;
  const uint32_t R = (uint32_t)a.R, U = (uint32_t)a.U;
  uint32_t n = 0;
  for (int f = r0; f <= r1; ++f) {  // consecutive rows (the host builds pred so)
    n = zp_stored(a, f);
    const uint32_t* rec = a.rows + (size_t)f * (4 + a.RW * a.K) + 4;
    const uint32_t* link = a.links + (size_t)f * a.K;
    uint32_t* o = a.out + (size_t)f * a.row_words + 4;
    // D of the previous frame: its entries' D block, or the carried state
    const uint32_t* prev = f == r0 ? st : a.out + (size_t)(f - 1) * a.row_words + 4 + 2 + R;
    const uint32_t pstride = f == r0 ? R : U;
    for (uint32_t j = (uint32_t)tid; j < n * R; j += kZpThreads) {
      const uint32_t e = j / R, r = j - e * R;
      const uint32_t pix = rec[(size_t)a.RW * e + 1], P = o[(size_t)e * U + 2 + r];
      const bool in = r == 0 || (P > 0 && 1024ull * P >= (unsigned long long)a.q * pix);
      uint32_t d = 0;
      if (in) {
        const uint32_t l = link[e];
        d = (l != kZpNone ? prev[(size_t)l * pstride + r] : 0u) + 1u;
      }
      o[(size_t)e * U + 2 + R + r] = d;
      if (r == 0) o[(size_t)e * U + 1] = rec[(size_t)a.RW * e + a.RW - 2];  // track_id
    }
    __syncthreads();  // one barrier a frame: this frame's D before the next frame's (or the state's) reads
  }
  const uint32_t* o = a.out + (size_t)r1 * a.row_words + 4 + 2 + R;
  for (uint32_t j = (uint32_t)tid; j < n * R; j += kZpThreads) {
    const uint32_t e = j / R, r = j - e * R;
    st[j] = o[(size_t)e * U + r];
  }
}

// Frame b's header and entries, words [0, 4 + U n), to the same offsets of dst (pinned host
// memory): the unused tail of the static buffer does not cross the bus.
__global__ __launch_bounds__(kZpThreads) void k_zp_copy_used(const uint32_t* __restrict__ src,
                                                              uint32_t* __restrict__ dst, int row_words,
                                                              int U) {
  const size_t row = (size_t)blockIdx.y * row_words;
  const long long want = 4 + (long long)U * src[row];
  const int used = (int)(want < row_words ? want : row_words);
  for (int i = blockIdx.x * kZpThreads + threadIdx.x; i < used; i += gridDim.x * kZpThreads)
    dst[row + i] = src[row + i];
}

}  // namespace

int zone_presence_chunk() { return kZpChunk; }

size_t zone_presence_workspace_bytes(int B, int crop_h, int crop_w, bool tracks) {
  // without tracking: the slot planes; with it they are region_tracks'
  return tracks ? 0 : (size_t)B * region_slot_plane_words(crop_h, crop_w) * sizeof(uint32_t);
}

size_t zone_presence_state_bytes(int streams, int K, int R) {
  return (size_t)streams * K * R * sizeof(uint32_t);
}

void zone_presence(const ZonePresenceParams& p, hipStream_t s) {
  const long long N = (long long)p.crop_h * p.crop_w;
  const bool tracks = p.tws != nullptr;
  const int rw_lo = tracks ? 8 : 6;
  if (p.B <= 0 || p.B > 65535 || p.crop_h <= 0 || p.crop_w <= 0 || N >= (1LL << 24) || p.K < 1 ||
      p.K > kZpMaxK || p.R < 1 || p.R > kZpMaxR || (p.R > 1) != (p.plane != nullptr) ||
      (p.record_words != rw_lo && p.record_words != rw_lo + 1) || p.rows == nullptr || p.out == nullptr ||
      (tracks ? (p.state == nullptr || p.pred == nullptr || p.last == nullptr || p.streams <= 0 ||
                 p.streams > 65535 || p.q < 1 || p.q > 1024)
              : (p.cr_ws == nullptr || p.ws == nullptr)))
    check(hipErrorInvalidValue, "zone_presence: bad arguments");
  const size_t pw = region_slot_plane_words(p.crop_h, p.crop_w);
  ZpArgs a;
  a.rows = p.rows; a.plane = p.plane; a.out = p.out; a.state = p.state; a.pred = p.pred; a.last = p.last;
  a.slot_stride = 2 * pw;
  a.K = p.K; a.R = p.R; a.U = 2 + p.R * (tracks ? 2 : 1); a.RW = p.record_words; a.N = (int)N;
  a.crop_w = p.crop_w; a.crop_h = p.crop_h; a.row_words = 4 + a.U * p.K;
  a.zmask = p.R >= 33 ? 0xffffffffu : ((1u << (p.R - 1)) - 1u);
  a.q = (uint32_t)p.q;
  if (tracks) {
    a.slots = reinterpret_cast<const uint16_t*>(p.tws + region_tracks_planes_offset_words());
    a.links = p.tws + region_tracks_links_offset_words(p.B, p.crop_h, p.crop_w, p.K);
  } else {
    class_regions_slot_planes(p.cr_ws, p.ws, p.B, p.crop_h, p.crop_w, s);
    a.slots = reinterpret_cast<const uint16_t*>(p.ws);
    a.links = nullptr;
  }
  hipLaunchKernelGGL(k_zp_init, dim3(cdiv(a.row_words, kZpThreads), p.B), dim3(kZpThreads), 0, s, a);
  hipLaunchKernelGGL(k_zp_count, dim3(cdiv(N, kZpChunk), p.B), dim3(kZpThreads), 0, s, a);
  if (tracks) hipLaunchKernelGGL(k_zp_dwell, dim3(p.streams), dim3(kZpThreads), 0, s, a);
  check_launch("zone_presence");
}

void zone_presence_copy_used(const uint32_t* src, uint32_t* dst, int B, int K, int U, hipStream_t s) {
  if (B <= 0 || B > 65535 || K < 1 || K > kZpMaxK || U < 3 || U > 2 + 2 * kZpMaxR)
    check(hipErrorInvalidValue, "zone_presence_copy_used: bad shape");
  const int row_words = 4 + U * K;
  const int bx = std::min(16, cdiv(row_words, kZpThreads * 4));
  hipLaunchKernelGGL(k_zp_copy_used, dim3(bx, B), dim3(kZpThreads), 0, s, src, dst, row_words, U);
  check_launch("zone_presence_copy_used");
}

}  // namespace ssa
