// Scaled dot-product self-attention, the BACKWARD pass from the forward's saved statistics for head dimensions 129 .. 256
// (vivit_attention_wide_backward_f32): the gradient of the function of attention_wide_forward.hip for ONE row dO [N, T, H d], given
// qkv, out and lse [N, H, T] as that unit wrote them.  The formulas, the results, the workspace (D [N, H, T] alone) and the contract
// are those at the head of attention_backward.hip; the owners are those of attention_wide.hip -- resident operands at full width
// (pitch 260), visiting ones in column halves of 128 (pitch 132), pass 1 for the score tiles and pass 2 for the results -- cut to
// one factor row and driven by the saved lse: no lse launch, no row-dot launch, no second row of dO, dS and accumulators.  Two
// launches on one stream:
//   attn_wide_bwd_dq_kernel   the QUERY-block owner of one (n, h, block of 32 queries).  Q and dO resident.  Before the walk the out
//                             block of its queries goes through the two half slots and D_i = sum_c dO_ic out_ic of its 32 rows is
//                             formed in the order of att_row_dot8 (attention_backward.hip: eight lanes per row, lane `sub` the chain
//                             over c = sub, sub + 8, .. ascending -- 128 is a multiple of 8, so the chain runs on into half 1 --
//                             folded by the butterfly), kept in LDS and written to the workspace.  Per key block jb_lo .. jb_hi:
//                             PASS 1 over the halves of K and V: S in the two carried chains of att_wide_tile_nt (the bits of the
//                             forward's logits), dP in the four of att_wide_tile_nt4, dZ = w (dP - D) into ONE LDS tile;
//                             PASS 2 dQ_c += dZ K_c over half 1 (still in LDS), then half 0 of K reloaded.
//   attn_wide_bwd_dkv_kernel  the KEY-block owner of one (n, kv head, block of 32 keys), behind the first.  K and V resident.  It walks
//                             the query heads of the group and the query blocks ib_lo .. ib_hi of each in ascending order; per step
//                             pass 1 over the halves of Q and dO (with lse and D of the block), one P and one dZ tile, pass 2
//                             dV_c += P^T dO_c and dK_c += dZ^T Q_c over half 1, then half 0 reloaded: eight accumulator tiles per
//                             wave each.
// LDS: query owner 2 x 33 280 (Q, dO) + 2 x 16 896 (K, V halves) + 4 608 (dZ) + 256 = 105 216 bytes; key owner 2 x 33 280 (K, V) +
// 2 x 16 896 (Q, dO halves) + 2 x 4 608 (P, dZ) + 256 = 109 824 bytes: one workgroup per CU either way, as for the rule's owners
// (143 232 and 131 456 bytes).  What this unit saves over the rule on one row is its two extra launches, the copies of an unused
// second factor row and two thirds of the workspace -- not occupancy.
// SUMMATION ORDER of an output element: that of attention_backward.hip (dQ: key blocks ascending, k ascending within a block; dK,
// dV: heads of the group, then query blocks, then k, ascending); the halves split columns of the results, never a sum.  No
// atomics.  DEAD POSITIONS: no row of dO, qkv, out, lse or D of one is read; their rows of dqkv are +0.  Every row of dqkv has
// exactly one writer.
#include "attention_wide_common.h"

namespace vivit {

constexpr int ATT_WIDE_BWD_DQ_FLOATS = 2 * AttWF::BLK + 2 * AttWH::BLK + AttWF::TILE + 2 * ATT_B;        // Q, dO; K, V halves; dZ; lse, D
constexpr int ATT_WIDE_BWD_DKV_FLOATS = 2 * AttWF::BLK + 2 * AttWH::BLK + 2 * AttWF::TILE + 2 * ATT_B;   // K, V; Q, dO halves; P, dZ; lse, D
static_assert(ATT_WIDE_BWD_DQ_FLOATS * 4 == 105216 && ATT_WIDE_BWD_DKV_FLOATS * 4 == 109824, "the LDS count at the head");
static_assert(AttWH::DP == ATT_WIDE_HALF && AttWH::TPW == 4, "a half is eight column tiles: four 16 x 16 tiles per wave");

// one wave's part of dZ = w (dP - D) from the four chains of its dP tile
__device__ __forceinline__ float att_wide_dz(float w, const att_f32x4 (&dp)[4], int e, float D) {
  return w * (((dp[0][e] + dp[1][e]) + (dp[2][e] + dp[3][e])) - D);
}

// ---- query-block owner: D and dQ ----------------------------------------------------------------------------------------------------
template <class Mod>
__global__ __launch_bounds__(256) void attn_wide_bwd_dq_kernel(const float *__restrict__ dO, const float *__restrict__ qkv,
                                                               const float *__restrict__ out, const float *__restrict__ lse,
                                                               float *__restrict__ Dws, float *__restrict__ G, AttGeom g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  constexpr int FL = AttWF::LD, FBLK = AttWF::BLK, HL = AttWH::LD, HBLK = AttWH::BLK;
  float *sQ = att_smem, *sdO = sQ + FBLK, *sK = sdO + FBLK, *sV = sK + HBLK, *sdS = sV + HBLK, *sL = sdS + AttWF::TILE, *sD = sL + ATT_B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t nh = blockIdx.x / g.KB;
  const int ib = (int)(blockIdx.x - nh * g.KB), i0 = ib * ATT_B;
  const int64_t n = nh / g.H;
  const int h = (int)(nh - n * g.H), dk = (g.d + 3) & ~3, T = g.T;
  const int64_t pitch = g.pitch, E = (int64_t)g.H * g.d;
  const float *base = att_q_rows(g, qkv, n), *kbase = base + g.koff + (int64_t)(h / g.R) * g.d;
  const AttLive L = att_live(g, n);
  // the key blocks this query block sees; a dead query block has none, loads nothing and stores its zeros
  const int KBn = (L.k + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int jb_lo = max(ib - wb, 0), jb_hi = i0 < L.q ? (att_causal(g) ? ib : min(ib + wb, KBn - 1)) : -1;
  if (jb_lo <= jb_hi) {
    const int64_t at = n * T * E + (int64_t)h * g.d;
    att_load_block<16>(sQ, base + (int64_t)h * g.d, pitch, i0, L.q, g.d, g.vec);
    att_load_block<16>(sdO, dO + at, E, i0, L.q, g.d, g.vec);
    att_wide_load_half(sK, out + at, E, i0, L.q, g.d, g.vec, 0);   // (the out block, until the walk's first K and V)
    att_wide_load_half(sV, out + at, E, i0, L.q, g.d, g.vec, 1);
    if (tid < ATT_B) sL[tid] = i0 + tid < L.q ? lse[nh * T + i0 + tid] : 0.f;
    __syncthreads();
    const int row = tid >> 3, sub = tid & 7;
    const float *a = sdO + row * FL;
    float x = 0.f;   // (rows >= L.q: zeros, D = +0)
    for (int c = sub; c < ATT_WIDE_HALF; c += 8) x = fmaf(a[c], sK[row * HL + c], x);
    for (int c = ATT_WIDE_HALF + sub; c < g.d; c += 8) x = fmaf(a[c], sV[row * HL + c - ATT_WIDE_HALF], x);
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) x += __shfl_xor(x, off, 64);
    if (sub == 0) {
      sD[row] = x;
      if (i0 + row < L.q) Dws[nh * T + i0 + row] = x;
    }
  }
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  const float *brow = att_bias_row(mod, T, h);
  const att_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  att_f32x4 accQ[2][4];   // [half][tile of the wave]
#pragma unroll
  for (int hp = 0; hp < 2; ++hp)
#pragma unroll
    for (int u = 0; u < 4; ++u) accQ[hp][u] = zero;
  for (int jb = jb_lo; jb <= jb_hi; ++jb) {
    const int j0 = jb * ATT_B;
    att_f32x4 s0 = zero, s1 = zero, dp[4] = {zero, zero, zero, zero};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      __syncthreads();   // what stood in the half slots (before the first: the out block) and, at half 0, in the tile has been read; sD is written
      att_wide_load_half(sK, kbase, pitch, j0, L.k, g.d, g.vec, half);
      att_wide_load_half(sV, kbase + att_k_to_v(g), pitch, j0, L.k, g.d, g.vec, half);
      __syncthreads();
      const int nc = half == 0 ? ATT_WIDE_HALF : dk - ATT_WIDE_HALF;
      att_wide_tile_nt<FL, HL>(sQ + 16 * ri * FL + ATT_WIDE_HALF * half, sK + 16 * cj * HL, nc, lane, s0, s1);
      att_wide_tile_nt4<FL, HL>(sdO + 16 * ri * FL + ATT_WIDE_HALF * half, sV + 16 * cj * HL, nc, lane, dp);
    }
    att_f32x4 w;   // (P alone is not used here)
    att_p_of(s0 + s1, sL, g.scale, lane, ri, cj, mod, brow, j0 - i0, w, [&](int r, int c) { return att_valid(g, L, i0 + r, j0 + c); });
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * ri + 4 * kq + e;
      sdS[r * ATT_LDP + 16 * cj + j] = att_wide_dz(w[e], dp, e, sD[r]);
    }
#pragma unroll
    for (int hp = 1; hp >= 0; --hp) {
      __syncthreads();   // dZ is written (hp = 1); half 1 of K has been read (hp = 0)
      if (hp == 0) {
        att_wide_load_half(sK, kbase, pitch, j0, L.k, g.d, g.vec, 0);
        __syncthreads();
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
        if (ATT_WIDE_HALF * hp + 16 * ct < g.d) accQ[hp][u] = att_acc_nn<8>(sdS, sK, rt, ct, lane, accQ[hp][u]);
      }
    }
  }
#pragma unroll
  for (int hp = 0; hp < 2; ++hp)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = ATT_WIDE_HALF * hp + 16 * ct + j;
      if (c < g.d) {
        float *gq = att_q_rows(g, G, n) + (int64_t)h * g.d + c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = i0 + 16 * rt + 4 * kq + e;
          if (r < T) gq[(int64_t)r * pitch] = r < L.q ? g.scale * accQ[hp][u][e] : 0.f;   // (a dead query's row: +0)
        }
      }
    }
}

// ---- key-block owner: dK and dV -----------------------------------------------------------------------------------------------------
template <class Mod>
__global__ __launch_bounds__(256) void attn_wide_bwd_dkv_kernel(const float *__restrict__ dO, const float *__restrict__ qkv,
                                                                const float *__restrict__ lse, const float *__restrict__ Dws,
                                                                float *__restrict__ G, AttGeom g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  constexpr int FL = AttWF::LD, FBLK = AttWF::BLK, HL = AttWH::LD, HBLK = AttWH::BLK, TILE = AttWF::TILE;
  float *sK = att_smem, *sV = sK + FBLK, *sQ = sV + FBLK, *sdO = sQ + HBLK, *sP = sdO + HBLK, *sdS = sP + TILE, *sL = sdS + TILE, *sD = sL + ATT_B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ng = blockIdx.x / g.KB;
  const int jb = (int)(blockIdx.x - ng * g.KB), j0 = jb * ATT_B;
  const int64_t n = ng / g.Hkv;
  const int kv = (int)(ng - n * g.Hkv), dk = (g.d + 3) & ~3, T = g.T;
  const int64_t pitch = g.pitch, E = (int64_t)g.H * g.d;
  const float *base = att_q_rows(g, qkv, n);
  const AttLive L = att_live(g, n);
  // the query blocks that see this key block; a dead key block has none, loads nothing and stores its zeros
  const int KBn = (L.q + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int ib_lo = att_causal(g) ? jb : max(jb - wb, 0), ib_hi = min(jb + wb, KBn - 1);
  const int per_head = j0 < L.k ? ib_hi - ib_lo + 1 : 0;
  if (per_head > 0) {
    att_load_block<16>(sK, base + g.koff + (int64_t)kv * g.d, pitch, j0, L.k, g.d, g.vec);
    att_load_block<16>(sV, base + g.voff + (int64_t)kv * g.d, pitch, j0, L.k, g.d, g.vec);
  }
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  // att_valid for the lane's key, the same in every tile of the walk, as the range of the queries that see it
  int q_lo, q_hi;
  att_query_range(g, L, j0 + 16 * cj + j, q_lo, q_hi);
  const att_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  att_f32x4 accK[2][4], accV[2][4];   // [half][tile of the wave]
#pragma unroll
  for (int hp = 0; hp < 2; ++hp)
#pragma unroll
    for (int u = 0; u < 4; ++u) accK[hp][u] = accV[hp][u] = zero;
  // the group's query heads in ascending order, the query blocks of each in ascending order: one chain of sums per output element
  for (int h = kv * g.R; per_head > 0 && h < (kv + 1) * g.R; ++h)
  for (int ib = ib_lo; ib <= ib_hi; ++ib) {
    const int i0 = ib * ATT_B;
    const int64_t nh = n * g.H + h;
    const float *qh = base + (int64_t)h * g.d, *doh = dO + n * T * E + (int64_t)h * g.d;
    att_f32x4 s0 = zero, s1 = zero, dp[4] = {zero, zero, zero, zero};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      __syncthreads();   // what stood in the half slots (and, at half 0, in the tiles and the statistics) has been read
      att_wide_load_half(sQ, qh, pitch, i0, L.q, g.d, g.vec, half);
      att_wide_load_half(sdO, doh, E, i0, L.q, g.d, g.vec, half);
      if (half == 0) {
        if (tid < ATT_B) sL[tid] = i0 + tid < L.q ? lse[nh * T + i0 + tid] : 0.f;
        else if (tid < 2 * ATT_B) sD[tid - ATT_B] = i0 + tid - ATT_B < L.q ? Dws[nh * T + i0 + tid - ATT_B] : 0.f;
      }
      __syncthreads();
      const int nc = half == 0 ? ATT_WIDE_HALF : dk - ATT_WIDE_HALF;
      att_wide_tile_nt<HL, FL>(sQ + 16 * ri * HL, sK + 16 * cj * FL + ATT_WIDE_HALF * half, nc, lane, s0, s1);
      att_wide_tile_nt4<HL, FL>(sdO + 16 * ri * HL, sV + 16 * cj * FL + ATT_WIDE_HALF * half, nc, lane, dp);
    }
    att_f32x4 w;
    const att_f32x4 p = att_p_of(s0 + s1, sL, g.scale, lane, ri, cj, mod, att_bias_row(mod, T, h), j0 - i0, w,
                                 [&](int r, int) { return i0 + r >= q_lo && i0 + r <= q_hi; });
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * ri + 4 * kq + e;
      sP[r * ATT_LDP + 16 * cj + j] = p[e];
      sdS[r * ATT_LDP + 16 * cj + j] = att_wide_dz(w[e], dp, e, sD[r]);
    }
    // pass 2: the columns of half 1, whose Q and dO are in LDS, then those of half 0
#pragma unroll
    for (int hp = 1; hp >= 0; --hp) {
      __syncthreads();   // P and dZ are written (hp = 1); half 1 has been read (hp = 0)
      if (hp == 0) {
        att_wide_load_half(sQ, qh, pitch, i0, L.q, g.d, g.vec, 0);
        att_wide_load_half(sdO, doh, E, i0, L.q, g.d, g.vec, 0);
        __syncthreads();
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
        if (ATT_WIDE_HALF * hp + 16 * ct < g.d) {
          accV[hp][u] = att_acc_tn<8>(sP, sdO, rt, ct, lane, accV[hp][u]);
          accK[hp][u] = att_acc_tn<8>(sdS, sQ, rt, ct, lane, accK[hp][u]);
        }
      }
    }
  }
  const int k_to_v = att_k_to_v(g);
#pragma unroll
  for (int hp = 0; hp < 2; ++hp)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = ATT_WIDE_HALF * hp + 16 * ct + j;
      if (c < g.d) {
        float *gk = att_q_rows(g, G, n) + g.koff + (int64_t)kv * g.d + c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = j0 + 16 * rt + 4 * kq + e;
          if (r < T) {   // (a dead key's row: +0 whatever the sign of the scale)
            gk[(int64_t)r * pitch] = r < L.k ? g.scale * accK[hp][u][e] : 0.f;
            gk[(int64_t)r * pitch + k_to_v] = r < L.k ? accV[hp][u][e] : 0.f;
          }
        }
      }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
template <class Mod>
static int attention_wide_backward_launch(const float *dO, const float *qkv, const float *out, const float *lse, float *G, float *Dws,
                                          const AttGeom &g, const Mod &mod, hipStream_t s) {
  static unsigned long long attr_done = 0;
  constexpr int dq_lds = ATT_WIDE_BWD_DQ_FLOATS * 4, dkv_lds = ATT_WIDE_BWD_DKV_FLOATS * 4;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
  if (!ensure_dynamic_lds(reinterpret_cast<const void *>(attn_wide_bwd_dq_kernel<Mod>), dq_lds, attr_done) ||
      !ensure_dynamic_lds(reinterpret_cast<const void *>(attn_wide_bwd_dkv_kernel<Mod>), dkv_lds, attr_done))
    return VIVIT_E_LAUNCH;
  attr_done |= 1ull << (dev & 63);
  attn_wide_bwd_dq_kernel<Mod><<<(unsigned)((int64_t)g.N * g.H * g.KB), 256, dq_lds, s>>>(dO, qkv, out, lse, Dws, G, g, mod);
  attn_wide_bwd_dkv_kernel<Mod><<<(unsigned)((int64_t)g.N * g.Hkv * g.KB), 256, dkv_lds, s>>>(dO, qkv, lse, Dws, G, g, mod);
  return launch_status();
}

// the workspace of an accepted plan with V = 1: D [N, H, T]
static size_t attention_wide_backward_bytes(const AttPlan &p) { return p.bytes - p.lse_bytes; }

} // namespace vivit

using namespace vivit;

extern "C" {

size_t vivit_attention_wide_backward_f32_workspace_bytes(int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d) {
  const AttPlan p = attention_wide_plan(1, N, T, H, Hkv, d);
  return p.status == VIVIT_OK ? attention_wide_backward_bytes(p) : 0;
}

// the arguments and the refusals of vivit_attention_backward_f32, in its order, for 128 < d <= 256
int vivit_attention_wide_backward_f32(const float *dout, const float *qkv, const float *out, const float *lse, float *dqkv, int64_t N,
                                      int64_t T, int64_t H, int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths,
                                      int64_t window, float softcap, const float *bias, void *workspace, size_t workspace_bytes,
                                      void *stream) {
  if (!(softcap >= 0.f) || isinf(softcap)) return VIVIT_E_BADARG;   // (negative, NaN, inf)
  if (!dout || !qkv || !out || !lse || !dqkv || window < 0) return VIVIT_E_BADARG;
  const AttPlan p = attention_wide_plan(1, N, T, H, Hkv, d);
  if (p.status != VIVIT_OK) return p.status;
  if (!workspace || workspace_bytes < attention_wide_backward_bytes(p)) return VIVIT_E_WORKSPACE;
  AttGeom g = attention_self_geom(dout, qkv, N, T, H, Hkv, d, p.KB, scale, causal, lengths, window);
  g.vec = g.vec && att_aligned16(out);
  float *Dws = static_cast<float *>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (softcap == 0.f && !bias) return attention_wide_backward_launch(dout, qkv, out, lse, dqkv, Dws, g, AttPlain{}, s);
  return attention_wide_backward_launch(dout, qkv, out, lse, dqkv, Dws, g, AttScoreMod{softcap, bias}, s);
}

} // extern "C"
