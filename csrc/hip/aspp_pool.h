// ASPP image-pooling branch: the device functions behind gap_partial_kernel and
// aspp_pool_kernel (model_ops.hip), shared with the pool work item of the grouped branch
// GEMM (conv_gemm.hip), which runs the same arithmetic inside one workgroup per image.
//
// Every output keeps ONE order of float operations wherever it is computed:
//   slice sl of the pixels is [HW * sl / 32, HW * (sl + 1) / 32); inside it chain wid
//   (0..3) sums pixels p0 + wid, p0 + wid + 4, ... in that order; the slice partial is
//   chain0 + chain1 + chain2 + chain3; gap = (sum of the slices q = 0..31) * (1 / HW);
//   the MLP runs the 1024-thread K split (nks = 1024 / (N / 4), per = ceil(K / nks)),
//   pool_slice's two accumulators, and the j = 1..nks-1 combine.
#pragma once
#include "common.h"

namespace ssa {

constexpr int kGapSlices = 32;
constexpr int kPoolMaxC = 2048, kPoolMaxN = 512;
constexpr int kPoolVT = 1024;  // thread count whose K split the image-pooling MLP runs

__device__ __forceinline__ void gap_slice_range(int HW, int sl, int& p0, int& p1) {
  p0 = (int)((long long)HW * sl / kGapSlices);
  p1 = (int)((long long)HW * (sl + 1) / kGapSlices);
}

// NCH neighbouring pixel chains of one 8-channel group: chain c adds pixels p + c,
// p + c + 4, ... (< p1) into acc[c], in that order. base: the image's channel group
// (+ cg * 8), C: channels per pixel. U steps of every chain are loaded before their adds
// (NCH * U 16-byte loads in flight); no chain's adds are reordered.
template <int NCH, int U>
__device__ __forceinline__ void gap_chains(const bf16* __restrict__ base, int C, int p, int p1,
                                           float (&acc)[NCH][8]) {
  for (; p + 4 * (U - 1) + NCH - 1 < p1; p += 4 * U) {
    bf16x8 v[U][NCH];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < NCH; ++c) v[u][c] = ld8(base + (long long)(p + 4 * u + c) * C);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[c][q] += (float)v[u][c][q];
  }
  for (; p < p1; p += 4) {
    bf16x8 v[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) v[c] = ld8(base + (long long)(p + c < p1 ? p + c : p) * C);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (p + c < p1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[c][q] += (float)v[c][q];
      }
  }
}

__device__ __forceinline__ float4 pool_slice(const float* __restrict__ wt, const float* s_x, int k0,
                                             int k1, int N, int q) {
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
  int k = k0;
  for (; k + 2 <= k1; k += 2) {
    const float4 w0 = *reinterpret_cast<const float4*>(wt + (size_t)k * N + 4 * q);
    const float4 w1 = *reinterpret_cast<const float4*>(wt + (size_t)(k + 1) * N + 4 * q);
    const float x0 = s_x[k], x1 = s_x[k + 1];
    a0.x += w0.x * x0; a0.y += w0.y * x0; a0.z += w0.z * x0; a0.w += w0.w * x0;
    a1.x += w1.x * x1; a1.y += w1.y * x1; a1.z += w1.z * x1; a1.w += w1.w * x1;
  }
  if (k < k1) {
    const float4 w0 = *reinterpret_cast<const float4*>(wt + (size_t)k * N + 4 * q);
    const float x0 = s_x[k];
    a0.x += w0.x * x0; a0.y += w0.y * x0; a0.z += w0.z * x0; a0.w += w0.w * x0;
  }
  return make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
}

// The branch after the slice partials, for one image, by one workgroup of nthr threads
// (nthr >= N / 4): part[kGapSlices][C] (global memory or LDS) -> out[N].
// The K split is that of VT threads whatever nthr is: a smaller workgroup walks the VT
// virtual thread ids. s_gap[C], s_pool[N], s_red[VT]: LDS. dimg / dv: debug dumps
// (scripts/debug_pool.py: per image [C gap | N pool | 4 x VT float4 stage views]) or null.
template <int VT>
__device__ __forceinline__ void aspp_pool_mlp(const float* __restrict__ part,
                                              const float* __restrict__ w1t,
                                              const float* __restrict__ b1,
                                              const float* __restrict__ w2t, float* __restrict__ out,
                                              int HW, int C, int N, float* s_gap, float* s_pool,
                                              float4* s_red, int tid, int nthr, float* dimg, float4* dv) {
  const float inv = 1.f / (float)HW;
  for (int k = tid; k < C; k += nthr) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < kGapSlices; ++q) s += part[(size_t)q * C + k];
    s_gap[k] = s * inv;
  }
  const int nq = N >> 2;        // float4 output columns
  const int nks = VT / nq;      // K slices
  __syncthreads();
  if (dimg)
    for (int k = tid; k < C; k += nthr) dimg[k] = s_gap[k];
  {
    const int per = (C + nks - 1) / nks;
    for (int vt = tid; vt < VT; vt += nthr) {
      const int q = vt % nq, ks = vt / nq;
      const int k0 = min(C, ks * per), k1 = min(C, k0 + per);
      if (ks < nks) {
        const float4 r = pool_slice(w1t, s_gap, k0, k1, N, q);
        s_red[ks * nq + q] = r;
        if (dv) dv[vt] = r;
      }
    }
  }
  __syncthreads();
  if (tid < nq) {
    float4 s = s_red[tid];
    if (dv) dv[VT + tid] = s;
    for (int j = 1; j < nks; ++j) {
      const float4 v = s_red[j * nq + tid];
      if (dv) dv[VT + j * nq + tid] = v;
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    s_pool[4 * tid + 0] = fmaxf(s.x + b1[4 * tid + 0], 0.f);
    s_pool[4 * tid + 1] = fmaxf(s.y + b1[4 * tid + 1], 0.f);
    s_pool[4 * tid + 2] = fmaxf(s.z + b1[4 * tid + 2], 0.f);
    s_pool[4 * tid + 3] = fmaxf(s.w + b1[4 * tid + 3], 0.f);
  }
  __syncthreads();
  if (dimg)
    for (int k = tid; k < N; k += nthr) dimg[C + k] = s_pool[k];
  {
    const int per = (N + nks - 1) / nks;
    for (int vt = tid; vt < VT; vt += nthr) {
      const int q = vt % nq, ks = vt / nq;
      const int k0 = min(N, ks * per), k1 = min(N, k0 + per);
      if (ks < nks) {
        const float4 r = pool_slice(w2t, s_pool, k0, k1, N, q);
        s_red[ks * nq + q] = r;
        if (dv) dv[2 * VT + vt] = r;
      }
    }
  }
  __syncthreads();
  if (tid < nq) {
    float4 s = s_red[tid];
    if (dv) dv[3 * VT + tid] = s;
    for (int j = 1; j < nks; ++j) {
      const float4 v = s_red[j * nq + tid];
      if (dv) dv[3 * VT + j * nq + tid] = v;
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(out + 4 * tid) = s;
  }
}

// LDS bytes of a pool work item: [kGapSlices][C] partials, gap[C], pooled[N], s_red[kPoolVT]
__host__ __device__ constexpr size_t pool_item_lds(int C, int N) {
  return ((size_t)(kGapSlices + 1) * C + N) * 4 + (size_t)kPoolVT * 16;
}

// One image's whole pooling branch by one workgroup of NTHR threads: the 32 slice
// partials (each thread owns a (slice, 8-channel group) and its 4 chains, 8 loads in
// flight) into LDS, then the MLP; out[N] is written with plain vector stores.
// smem: pool_item_lds(C, N) bytes, 16-byte aligned. Reached workgroup-uniformly.
template <int NTHR>
__device__ __forceinline__ void aspp_pool_item(const bf16* __restrict__ in /* image b */,
                                               const float* __restrict__ w1t,
                                               const float* __restrict__ b1,
                                               const float* __restrict__ w2t, float* __restrict__ out,
                                               int HW, int C, int N, char* smem) {
  float* s_part = reinterpret_cast<float*>(smem);
  float* s_gap = s_part + (size_t)kGapSlices * C;
  float* s_pool = s_gap + C;
  float4* s_red = reinterpret_cast<float4*>(s_pool + N);  // (33 C + N) * 4 bytes: 16-aligned
  const int tid = threadIdx.x;
  const int CG = C >> 3;
  for (int it = tid; it < kGapSlices * CG; it += NTHR) {
    const int sl = it / CG, cg = it - sl * CG;
    int p0, p1;
    gap_slice_range(HW, sl, p0, p1);
    float acc[4][8];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[c][q] = 0.f;
    gap_chains<4, 2>(in + cg * 8, C, p0, p1, acc);
    float* dst = s_part + (size_t)sl * C + cg * 8;
#pragma unroll
    for (int q = 0; q < 8; ++q) dst[q] = acc[0][q] + acc[1][q] + acc[2][q] + acc[3][q];
  }
  __syncthreads();
  aspp_pool_mlp<kPoolVT>(s_part, w1t, b1, w2t, out, HW, C, N, s_gap, s_pool, s_red, tid, NTHR,
                         nullptr, nullptr);
}

}  // namespace ssa
