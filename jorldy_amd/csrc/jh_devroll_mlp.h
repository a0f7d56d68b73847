// The two trunk layers of the device-resident rollout kernels (jh_devroll.hip, jh_devroll_q.hip, jh_devroll_ac.hip), stated ONCE: one
// workgroup of 4 waves carries one 16-row MFMA tile from the float64 env state in LDS through  head.l (S -> H, relu)  and  l (H -> N2, relu).
// Both run on v_mfma_f32_16x16x4_f32; every sum runs in an order fixed by k alone, and no sum crosses a wave.  Neither function ends in a
// barrier: the caller places one behind each.
#pragma once
#include <hip/hip_runtime.h>

namespace jh_roll {
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kRows = 16, kThreads = 256, kWaves = 4;
constexpr int kG1 = 8;  // column tiles of layer 1 a wave carries at once
constexpr int kU2 = 8;  // k chunks of W2 per block of layer 2: 32 MFMAs against one L2 round trip

// ---- layer 1: es float64 [16][S] (LDS) -> out [16][ld] (LDS) = relu(es W1^T + b1), W1 [H][S] from L2 (4-byte loads: S need not be a multiple
// of 4).  Lane supplies A[row r][k] and B[k][unit r] for k = 4 ks + kq; holds C[row 4 kq + i][unit r].  A wave takes its column tiles v, v + 4,
// ... kG1 at a time: one observation fragment feeds all of them, and their W1 pieces of the NEXT k step are in flight during the MFMAs
__device__ __forceinline__ void layer1(const float* W1, const float* b1, const double* es, int S, int H, float* out, int ld) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
  const int tiles = H / 16;
  const int nks = (S + 3) / 4;  // (all four k groups make the same number of trips: the MFMA is wave-wide)
  for (int g0 = wave; g0 < tiles; g0 += kWaves * kG1) {
    f32x4 acc[kG1];
    float bw[kG1], bn[kG1];
#pragma unroll
    for (int j = 0; j < kG1; ++j) {
      acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int ct = g0 + kWaves * j;
      bw[j] = (ct < tiles && kq < S) ? W1[(size_t)(ct * 16 + r) * S + kq] : 0.f;
    }
    for (int ks = 0; ks < nks; ++ks) {
      const int k = 4 * ks + kq;
#pragma unroll
      for (int j = 0; j < kG1; ++j) {
        const int ct = g0 + kWaves * j;
        bn[j] = (ct < tiles && k + 4 < S) ? W1[(size_t)(ct * 16 + r) * S + k + 4] : 0.f;
      }
      const float av = k < S ? (float)es[r * S + k] : 0.f;
#pragma unroll
      for (int j = 0; j < kG1; ++j) {
        if (g0 + kWaves * j < tiles) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[j], acc[j], 0, 0, 0);  // (uniform)
        bw[j] = bn[j];
      }
    }
#pragma unroll
    for (int j = 0; j < kG1; ++j) {
      const int unit = (g0 + kWaves * j) * 16 + r;
      if (unit < H) {
        const float b = b1[unit];
#pragma unroll
        for (int i = 0; i < 4; ++i) out[(4 * kq + i) * ld + unit] = fmaxf(acc[j][i] + b, 0.f);
      }
    }
  }
}

// ---- layer 2: in [16][ld_in] (LDS, H columns) -> out [16][ld_out] (LDS) = relu(in W2^T + b2) over `ot` output column tiles, W2 [16 ot][H]
// from L2.  Wave v computes the column tiles v, v + 4, ... over the WHOLE k range.  Its work is a flat sequence of (column tile, block of
// kU2 k chunks); while the 4 kU2 MFMAs of one block issue (about an L2 round trip), the kU2 16-byte pieces of W2 of the NEXT block -- of the
// next column tile at a tile's end -- are in flight, and two accumulator chains keep the matrix pipe from waiting on its own result
__device__ __forceinline__ void layer2(const float* W2, const float* b2, const float* in, int ld_in, int H, int ot, float* out, int ld_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
  const int kt = H / 16;
  const int nblk = (kt + kU2 - 1) / kU2, my_tiles = wave < ot ? (ot - wave + kWaves - 1) / kWaves : 0;
  const float* hp = in + r * ld_in + kq * 4;
  float4 cur[kU2], nxt[kU2];
  auto fetch = [&](int ct, int blk, float4* dst) {
    const float* wp = W2 + (size_t)(ct * 16 + r) * H + kq * 4;
#pragma unroll
    for (int u = 0; u < kU2; ++u) {
      const int c = blk * kU2 + u;
      dst[u] = c < kt ? *reinterpret_cast<const float4*>(wp + c * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  if (my_tiles) fetch(wave, 0, cur);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int ti = 0; ti < my_tiles; ++ti) {
    const int ct = wave + kWaves * ti;
    for (int blk = 0; blk < nblk; ++blk) {
      const bool last = blk + 1 == nblk;
      if (!last || ti + 1 < my_tiles) fetch(last ? ct + kWaves : ct, last ? 0 : blk + 1, nxt);
#pragma unroll
      for (int u = 0; u < kU2; ++u) {
        const int c = blk * kU2 + u;
        if (c < kt) {  // (uniform)
          const float4 av = *reinterpret_cast<const float4*>(hp + c * 16);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, cur[u].x, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, cur[u].y, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, cur[u].z, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, cur[u].w, acc1, 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < kU2; ++u) cur[u] = nxt[u];
    }
    const int unit = ct * 16 + r;
    const float b = b2[unit];
#pragma unroll
    for (int i = 0; i < 4; ++i) out[(4 * kq + i) * ld_out + unit] = fmaxf((acc0[i] + acc1[i]) + b, 0.f);
    acc0 = f32x4{0.f, 0.f, 0.f, 0.f}; acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}
}  // namespace jh_roll
