// What the translation units for head dimensions 129 .. 256 share (attention_wide.hip: the rule; attention_wide_forward.hip: the
// forward pass; attention_wide_backward.hip: its gradient from the saved lse): the widths, the carried-chain tile products, the
// loader of a column half and the host plan.  The scheme they serve -- resident operands at full width, visiting ones in column
// halves of 128 -- stands at the head of attention_wide.hip.
#pragma once
#include "attention_common.h"

namespace vivit {

constexpr int ATT_WIDE_D_MIN = 129, ATT_WIDE_D_MAX = 256;
constexpr int ATT_WIDE_HALF = 128;   // columns of a half
using AttWF = AttCfg<16>;            // a block at full width
using AttWH = AttCfg<8>;             // a column half of a block

// att_tile_nt over nc columns (a multiple of 4) of one half, its two chains carried by the caller: A in a block of pitch LDA, B in a
// block of pitch LDB, both at the half's first column.  After half 0 (nc = 128) and half 1 (nc = dk - 128), acc0 + acc1 has the
// bits of att_tile_nt<16> over dk columns.
template <int LDA, int LDB>
__device__ __forceinline__ void att_wide_tile_nt(const float *__restrict__ A, const float *__restrict__ B, int nc, int lane,
                                                 att_f32x4 &acc0, att_f32x4 &acc1) {
  const float *a = A + (lane & 15) * LDA + (lane >> 4), *b = B + (lane & 15) * LDB + (lane >> 4);
  int c = 0;
  for (; c + 8 <= nc; c += 8) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[c], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c + 4], b[c + 4], acc1, 0, 0, 0);
  }
  if (c < nc) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[c], acc0, 0, 0, 0);
}

// The same product for the dP tiles, in FOUR interleaved chains (step c / 4 into chain (c / 4) mod 4, at the end (0 + 1) + (2 + 3)): dS =
// P o (dP - D) subtracts two sums over up to 256 columns that nearly cancel, so what is left of them carries their rounding errors
// at full size; four chains of at most 16 steps over partial sums a quarter as large halve the error of two chains of 32.  dP is
// compared with nothing (S is: its two chains are those of the lse launch), and 128 = 32 steps, so half 1 starts at chain 0 again.
template <int LDA, int LDB>
__device__ __forceinline__ void att_wide_tile_nt4(const float *__restrict__ A, const float *__restrict__ B, int nc, int lane,
                                                  att_f32x4 (&acc)[4]) {
  const float *a = A + (lane & 15) * LDA + (lane >> 4), *b = B + (lane & 15) * LDB + (lane >> 4);
  int c = 0;
  for (; c + 16 <= nc; c += 16) {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c + 4 * u], b[c + 4 * u], acc[u], 0, 0, 0);
  }
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (c + 4 * u < nc) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c + 4 * u], b[c + 4 * u], acc[u], 0, 0, 0);
}

// columns 128 half .. of rows r0 .. r0 + 31 of a [T][stride] matrix -> dst[32][132]; rows beyond T and columns beyond d are zero
__device__ __forceinline__ void att_wide_load_half(float *__restrict__ dst, const float *__restrict__ src, int64_t stride, int r0, int T,
                                                   int d, bool vec, int half) {
  att_load_block<8>(dst, src + ATT_WIDE_HALF * half, stride, r0, T, d - ATT_WIDE_HALF * half, vec);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static AttPlan attention_wide_plan(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d) {
  AttPlan p = attention_plan(V, N, T, H, Hkv, d, ATT_WIDE_D_MAX);
  if (p.status == VIVIT_OK && d < ATT_WIDE_D_MIN) p.status = VIVIT_E_UNSUPPORTED;   // (the narrow entries' head dimensions)
  return p;
}

} // namespace vivit
