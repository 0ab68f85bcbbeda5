// Scaled dot-product attention, the BACKWARD pass from the forward's saved statistics (vivit_attention_backward_f32,
// vivit_attention_cross_backward_f32): the gradient of the function of attention_forward.hip for ONE row dO [N, Tq, H d], given the
// forward's inputs, its out [N, Tq, H d] and its lse [N, H, Tq] as attn_fwd_kernel wrote them.  The layouts, the mask, the dead
// positions, the block ranges, the two geometries and the score function are those at the head of attention.hip; the formulas are
// its rule's with V = 1:
//   P = exp(s - lse),  D_i = sum_c dO_ic O_ic,  dP = dO V_g^T,  dS = P o (dP - D),  dZ = dS o (1 - t^2) behind a cap (else dS),
//   dQ_h = scale dZ K_g,   dK_g = scale sum_{h in g} dZ_h^T Q_h,   dV_g = sum_{h in g} P_h^T dO_h.
// Results: dqkv [N, T, (H + 2 Hkv) d] = dQ | dK | dV, or dq [N, Tq, H d] and dkv [N, Tk, 2 Hkv d] = dK | dV for cross-attention
// (either may be left out).  They may be uninitialised memory: every row has exactly one writer.  Workspace: D [N, H, Tq] floats and
// nothing else.  The rule's kernels (attention.hip) are built for V >= 2 factor rows: they recompute lse, launch a row-dot kernel
// and carry VC = 2 or 4 rows of dO, dS and accumulators per workgroup.  Here there is no lse launch, no separate row-dot launch, one
// row of everything, no atomics and no T x T datum in memory.  Two launches on one stream:
//   attn_bwd_dq_kernel   the QUERY-block owner of one (n, h, block of 32 queries).  Q, dO and lse of its queries go to LDS once; the
//                        out block of its queries goes into the slot the walk reuses for K, and D_i of its 32 rows is formed from
//                        the two LDS blocks (att_row_dot8: eight lanes per row, lane `sub` the chain over the columns sub, sub + 8,
//                        ... ascending, the eight chains folded by the butterfly of the online softmax), kept in LDS and written to
//                        the workspace for the key owner.  Then it walks the key blocks jb_lo .. jb_hi of attn_dq_kernel in
//                        ascending order: K and V of the block into LDS; the S and dP tiles of the wave together (att_tile_nt2:
//                        four independent MFMA chains issued alternately); dZ = w (dP - D) into ONE LDS tile; dQ += dZ K in TPW
//                        accumulator tiles (att_acc_nn).
//   attn_bwd_dkv_kernel  the KEY-block owner of one (n, g, block of 32 keys), launched behind the first: K and V of its keys stay in
//                        LDS; it walks the query heads of the group in ascending order and the query blocks ib_lo .. ib_hi of each
//                        in ascending order, reloads Q, dO, lse and D per step, keeps one P tile and one dZ tile and one set of
//                        accumulators each for dK and dV (att_acc_tn).
// Where dq is not wanted (cross-attention with a frozen query side) the query owner is not launched and attn_bwd_d_kernel writes D
// with the chains of att_row_dot8 from global memory -- the bytes of D, and with them those of dkv, are the same either way (the
// rule's attn_rowdot_kernel is one chain per row: other bytes).  Where dkv is not wanted the key owner is not launched.
// LDS (AttBwdCfg; Q, K, V, dO blocks of pitch 16 NT + 4, the tiles of pitch 36, lse and D): the query owner 14.8 / 22.8 / 38.8 /
// 70.8 KiB, the key owner 19.2 / 27.2 / 43.2 / 75.2 KiB for NT = 1 / 2 / 4 / 8 -- against 96.4 KiB of a rule owner at NT = 8: two
// workgroups of either kernel share a CU's 160 KiB at d = 128.
// SUMMATION ORDER of an output element.  dQ: key blocks ascending, inside a block k ascending in steps of four.  dK, dV: the query
// heads of the group ascending, inside a head the query blocks ascending, inside a block k ascending.  The S and dP tiles: two
// interleaved chains each, even and odd steps of four, added at the end (att_tile_nt's).  D: above.
// BYTES.  The bytes of sample n's rows depend on (T, H, Hkv, d, scale, causal; the length of n, the window, the cap, the table) and
// the data of sample n only.  PADDED SAMPLES: with lengths, rows < Tn of sample n have the bytes of the sample cut to Tn (every
// operand, lse included) and run alone, with the table's middle slice.  DEAD POSITIONS are never loaded -- no row of dO, qkv / q / kv,
// out, lse or D of a dead position is read (the workspace has no D there at all), so NaN there reaches nothing -- and their rows of
// the results are +0.
#include "attention_common.h"

namespace vivit {

template <int NT> struct AttBwdCfg {
  using C = AttCfg<NT>;
  static constexpr int DQ_FLOATS = 4 * C::BLK + C::TILE + 2 * ATT_B;        // K (first: out), V, Q, dO; dZ; lse, D
  static constexpr int DKV_FLOATS = 4 * C::BLK + 2 * C::TILE + 2 * ATT_B;   // K, V, Q, dO; P, dZ; lse, D
};
static_assert(AttBwdCfg<4>::DKV_FLOATS * 4 <= 64 * 1024, "only the NT = 8 instances ask for more than the default dynamic LDS limit");
static_assert(2 * AttBwdCfg<8>::DKV_FLOATS * 4 <= 160 * 1024, "two key owners share a CU at d = 128");

// C1 = A1 B1^T and C2 = A2 B2^T, one 16 x 16 tile each (att_tile_nt's operands, twice): the two chains of each product and the two
// products alternate, so four MFMAs are in flight and none waits for its predecessor's result.  Each result has the order, and the
// bytes, att_tile_nt gives it.
template <int NT>
__device__ __forceinline__ void att_tile_nt2(const float *__restrict__ A1, const float *__restrict__ B1, const float *__restrict__ A2,
                                             const float *__restrict__ B2, int dk, int lane, att_f32x4 &c1, att_f32x4 &c2) {
  constexpr int LD = AttCfg<NT>::LD;
  const int off = (lane & 15) * LD + (lane >> 4);
  const float *a1 = A1 + off, *b1 = B1 + off, *a2 = A2 + off, *b2 = B2 + off;
  att_f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, p0 = s0, p1 = s0;
  int c = 0;
  for (; c + 8 <= dk; c += 8) {
    s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[c], b1[c], s0, 0, 0, 0);
    p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[c], b2[c], p0, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[c + 4], b1[c + 4], s1, 0, 0, 0);
    p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[c + 4], b2[c + 4], p1, 0, 0, 0);
  }
  if (c < dk) {
    s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[c], b1[c], s0, 0, 0, 0);
    p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[c], b2[c], p0, 0, 0, 0);
  }
  c1 = s0 + s1, c2 = p0 + p1;
}

// sum_{c < d} a[c] b[c] of one row by its eight lanes (sub = 0 .. 7, consecutive lanes of a wave, all of them here): lane `sub` is
// the chain over c = sub, sub + 8, ... ascending; the eight are folded by a butterfly and every lane returns the sum.  The bytes do
// not depend on where a and b live (LDS in the query owner, global memory in attn_bwd_d_kernel).
__device__ __forceinline__ float att_row_dot8(const float *__restrict__ a, const float *__restrict__ b, int d, int sub) {
  float x = 0.f;
  for (int c = sub; c < d; c += 8) x = fmaf(a[c], b[c], x);
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// ---- D alone, for a call without dq: eight lanes per live row (n, h, i) ----------------------------------------------------------------
template <class Geo>
__global__ __launch_bounds__(256) void attn_bwd_d_kernel(const float *__restrict__ dO, const float *__restrict__ O, float *__restrict__ D,
                                                         int64_t rows, Geo g) {
  const int sub = threadIdx.x & 7;
  const int64_t T = att_Tq(g), E = (int64_t)g.H * g.d;
  // (a row's eight lanes share every condition below, so the butterfly always has its eight)
  for (int64_t e = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3); e < rows; e += (int64_t)gridDim.x * 32) {
    const int64_t nh = e / T, n = nh / g.H;
    const int t = (int)(e - nh * T), h = (int)(nh - n * g.H);
    if (t >= att_live(g, n).q) continue;   // a dead row: D is never read there
    const int64_t at = (n * T + t) * E + (int64_t)h * g.d;
    const float x = att_row_dot8(dO + at, O + at, g.d, sub);
    if (sub == 0) D[e] = x;
  }
}

// ---- query-block owner: D and dQ ----------------------------------------------------------------------------------------------------------
template <int NT, class Geo, class Mod>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float *__restrict__ dO, const float *__restrict__ qkv,
                                                          const float *__restrict__ out, const float *__restrict__ lse,
                                                          float *__restrict__ Dws, float *__restrict__ G, Geo g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  using C = AttCfg<NT>;
  float *sK = att_smem, *sV = sK + C::BLK, *sQ = sV + C::BLK, *sdO = sQ + C::BLK, *sdS = sdO + C::BLK, *sL = sdS + C::TILE, *sD = sL + ATT_B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t nh = blockIdx.x / att_KBq(g);
  const int ib = (int)(blockIdx.x - nh * att_KBq(g)), i0 = ib * ATT_B;
  const int64_t n = nh / g.H;
  const int h = (int)(nh - n * g.H), dk = (g.d + 3) & ~3, Tq = att_Tq(g);
  const int64_t qpitch = att_qpitch(g), kpitch = att_kpitch(g), E = (int64_t)g.H * g.d;
  const float *base = att_q_rows(g, qkv, n), *kbase = att_k_rows(g, base, n) + (int64_t)(h / g.R) * g.d;
  const AttLive L = att_live(g, n);
  // the key blocks this query block sees (the head of attention.hip); a dead query block (i0 >= L.q) has none, loads nothing and
  // stores its zeros
  const int KBn = (L.k + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int jb_lo = max(ib - wb, 0), jb_hi = i0 < L.q ? (att_causal(g) ? ib : min(ib + wb, KBn - 1)) : -1;
  if (jb_lo <= jb_hi) {
    const int64_t at = n * Tq * E + (int64_t)h * g.d;
    att_load_block<NT>(sQ, base + (int64_t)h * g.d, qpitch, i0, L.q, g.d, g.vec);
    att_load_block<NT>(sdO, dO + at, E, i0, L.q, g.d, g.vec);
    att_load_block<NT>(sK, out + at, E, i0, L.q, g.d, g.vec);   // (the out block, until the walk's first K)
    if (tid < ATT_B) sL[tid] = i0 + tid < L.q ? lse[nh * Tq + i0 + tid] : 0.f;
    __syncthreads();
    const int row = tid >> 3, sub = tid & 7;
    const float x = att_row_dot8(sdO + row * C::LD, sK + row * C::LD, g.d, sub);   // (rows >= L.q: zeros, D = +0)
    if (sub == 0) {
      sD[row] = x;
      if (i0 + row < L.q) Dws[nh * Tq + i0 + row] = x;
    }
  }
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  const float *brow = att_bias_row(mod, Tq, h);
  att_f32x4 accQ[C::TPW];
#pragma unroll
  for (int u = 0; u < C::TPW; ++u) accQ[u] = (att_f32x4){0.f, 0.f, 0.f, 0.f};
  for (int jb = jb_lo; jb <= jb_hi; ++jb) {
    const int j0 = jb * ATT_B;
    __syncthreads();   // the previous key block's tile and operands (before the first: the out block) have been read, sD is written
    att_load_block<NT>(sK, kbase, kpitch, j0, L.k, g.d, g.vec);
    att_load_block<NT>(sV, kbase + att_k_to_v(g), kpitch, j0, L.k, g.d, g.vec);
    __syncthreads();
    att_f32x4 s, dp, w;   // (P alone is not used here)
    att_tile_nt2<NT>(sQ + 16 * ri * C::LD, sK + 16 * cj * C::LD, sdO + 16 * ri * C::LD, sV + 16 * cj * C::LD, dk, lane, s, dp);
    att_p_of(s, sL, g.scale, lane, ri, cj, mod, brow, j0 - i0, w, [&](int r, int c) { return att_valid(g, L, i0 + r, j0 + c); });
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * ri + 4 * kq + e;
      sdS[r * ATT_LDP + 16 * cj + j] = w[e] * (dp[e] - sD[r]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < C::TPW; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
      if (t < 2 * NT && 16 * ct < g.d) accQ[u] = att_acc_nn<NT>(sdS, sK, rt, ct, lane, accQ[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < C::TPW; ++u) {
    const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = 16 * ct + j;
    if (t < 2 * NT && c < g.d) {
      float *gq = att_q_rows(g, G, n) + (int64_t)h * g.d + c;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = i0 + 16 * rt + 4 * kq + e;
        if (r < Tq) gq[(int64_t)r * qpitch] = r < L.q ? g.scale * accQ[u][e] : 0.f;   // (a dead query's row: +0)
      }
    }
  }
}

// ---- key-block owner: dK and dV -----------------------------------------------------------------------------------------------------------
template <int NT, class Geo, class Mod>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const float *__restrict__ dO, const float *__restrict__ qkv,
                                                           const float *__restrict__ lse, const float *__restrict__ Dws,
                                                           float *__restrict__ G, Geo g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  using C = AttCfg<NT>;
  float *sK = att_smem, *sV = sK + C::BLK, *sQ = sV + C::BLK, *sdO = sQ + C::BLK;
  float *sP = sdO + C::BLK, *sdS = sP + C::TILE, *sL = sdS + C::TILE, *sD = sL + ATT_B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ng = blockIdx.x / att_KBk(g);
  const int jb = (int)(blockIdx.x - ng * att_KBk(g)), j0 = jb * ATT_B;
  const int64_t n = ng / g.Hkv;
  const int kv = (int)(ng - n * g.Hkv), dk = (g.d + 3) & ~3, Tq = att_Tq(g);
  const int64_t qpitch = att_qpitch(g), kpitch = att_kpitch(g), E = (int64_t)g.H * g.d;
  const float *base = att_q_rows(g, qkv, n);
  const AttLive L = att_live(g, n);
  // the query blocks that see this key block (the head of attention.hip); a dead key block (j0 >= L.k) has none, loads nothing and
  // stores its zeros
  const int KBn = (L.q + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int ib_lo = att_causal(g) ? jb : max(jb - wb, 0), ib_hi = min(jb + wb, KBn - 1);
  const int per_head = j0 < L.k ? ib_hi - ib_lo + 1 : 0;
  if (per_head > 0) {
    att_load_block<NT>(sK, att_k_rows(g, base, n) + (int64_t)kv * g.d, kpitch, j0, L.k, g.d, g.vec);
    att_load_block<NT>(sV, att_v_rows(g, base, n) + (int64_t)kv * g.d, kpitch, j0, L.k, g.d, g.vec);
  }
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  // att_valid for the lane's key, the same in every tile of the walk, as the range of the queries that see it (attn_dkv_kernel)
  int q_lo, q_hi;
  att_query_range(g, L, j0 + 16 * cj + j, q_lo, q_hi);
  att_f32x4 accK[C::TPW], accV[C::TPW];
#pragma unroll
  for (int u = 0; u < C::TPW; ++u) accK[u] = accV[u] = (att_f32x4){0.f, 0.f, 0.f, 0.f};
  // the group's query heads in ascending order, the query blocks of each in ascending order: one chain of sums per output element
  for (int step = 0; step < g.R * per_head; ++step) {
    const int hr = step / per_head, ib = ib_lo + step - hr * per_head;
    const int h = kv * g.R + hr, i0 = ib * ATT_B;
    const int64_t nh = n * g.H + h;
    __syncthreads();   // the previous query block's tiles and operands have been read
    att_load_block<NT>(sQ, base + (int64_t)h * g.d, qpitch, i0, L.q, g.d, g.vec);
    att_load_block<NT>(sdO, dO + n * Tq * E + (int64_t)h * g.d, E, i0, L.q, g.d, g.vec);
    if (tid < ATT_B) sL[tid] = i0 + tid < L.q ? lse[nh * Tq + i0 + tid] : 0.f;
    else if (tid < 2 * ATT_B) sD[tid - ATT_B] = i0 + tid - ATT_B < L.q ? Dws[nh * Tq + i0 + tid - ATT_B] : 0.f;
    __syncthreads();
    att_f32x4 s, dp, w;
    att_tile_nt2<NT>(sQ + 16 * ri * C::LD, sK + 16 * cj * C::LD, sdO + 16 * ri * C::LD, sV + 16 * cj * C::LD, dk, lane, s, dp);
    const att_f32x4 p = att_p_of(s, sL, g.scale, lane, ri, cj, mod, att_bias_row(mod, Tq, h), j0 - i0, w,
                                 [&](int r, int) { return i0 + r >= q_lo && i0 + r <= q_hi; });
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * ri + 4 * kq + e;
      sP[r * ATT_LDP + 16 * cj + j] = p[e];
      sdS[r * ATT_LDP + 16 * cj + j] = w[e] * (dp[e] - sD[r]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < C::TPW; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
      if (t < 2 * NT && 16 * ct < g.d) {
        accV[u] = att_acc_tn<NT>(sP, sdO, rt, ct, lane, accV[u]);
        accK[u] = att_acc_tn<NT>(sdS, sQ, rt, ct, lane, accK[u]);
      }
    }
  }
  const int k_to_v = att_k_to_v(g);
#pragma unroll
  for (int u = 0; u < C::TPW; ++u) {
    const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = 16 * ct + j;
    if (t < 2 * NT && c < g.d) {
      float *gk = att_gk_rows(g, att_q_rows(g, G, n), n) + (int64_t)kv * g.d + c;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = j0 + 16 * rt + 4 * kq + e;
        if (r < att_Tk(g)) {   // (a dead key's row: +0 whatever the sign of the scale)
          gk[(int64_t)r * kpitch] = r < L.k ? g.scale * accK[u][e] : 0.f;
          gk[(int64_t)r * kpitch + k_to_v] = r < L.k ? accV[u][e] : 0.f;
        }
      }
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
// `G`: the result of the query owner (null: D comes from attn_bwd_d_kernel), `Gkv`: whether the key owner runs (self-attention: the
// packed tensor G again; cross-attention: g.Gkv)
template <int NT, class Geo, class Mod>
static int attention_backward_launch(const float *dO, const float *qkv, const float *out, const float *lse, float *G, const float *Gkv,
                                     float *Dws, const Geo &g, const Mod &mod, int64_t Tq, int64_t KBq, int64_t KBk, hipStream_t s) {
  using B = AttBwdCfg<NT>;
  static unsigned long long attr_done = 0;
  constexpr int dq_lds = B::DQ_FLOATS * 4, dkv_lds = B::DKV_FLOATS * 4;
  if (dkv_lds > 64 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
    if (!ensure_dynamic_lds(reinterpret_cast<const void *>(attn_bwd_dq_kernel<NT, Geo, Mod>), dq_lds, attr_done) ||
        !ensure_dynamic_lds(reinterpret_cast<const void *>(attn_bwd_dkv_kernel<NT, Geo, Mod>), dkv_lds, attr_done))
      return VIVIT_E_LAUNCH;
    attr_done |= 1ull << (dev & 63);
  }
  const int64_t NH = (int64_t)g.N * g.H, rows = NH * Tq, d_blocks = cdiv(rows, 32);
  if (G)
    attn_bwd_dq_kernel<NT, Geo, Mod><<<(unsigned)(NH * KBq), 256, dq_lds, s>>>(dO, qkv, out, lse, Dws, G, g, mod);
  else
    attn_bwd_d_kernel<Geo><<<(unsigned)(d_blocks < 0x7fffffffLL ? d_blocks : 0x7fffffffLL), 256, 0, s>>>(dO, out, Dws, rows, g);
  if (Gkv) attn_bwd_dkv_kernel<NT, Geo, Mod><<<(unsigned)((int64_t)g.N * g.Hkv * KBk), 256, dkv_lds, s>>>(dO, qkv, lse, Dws, G, g, mod);
  return launch_status();
}

template <class Geo, class Mod>
static int attention_backward_launch_d(const float *dO, const float *qkv, const float *out, const float *lse, float *G, const float *Gkv,
                                       float *Dws, const Geo &g, const Mod &mod, int64_t Tq, int64_t KBq, int64_t KBk, hipStream_t s) {
  if (g.d <= 16) return attention_backward_launch<1>(dO, qkv, out, lse, G, Gkv, Dws, g, mod, Tq, KBq, KBk, s);
  if (g.d <= 32) return attention_backward_launch<2>(dO, qkv, out, lse, G, Gkv, Dws, g, mod, Tq, KBq, KBk, s);
  if (g.d <= 64) return attention_backward_launch<4>(dO, qkv, out, lse, G, Gkv, Dws, g, mod, Tq, KBq, KBk, s);
  return attention_backward_launch<8>(dO, qkv, out, lse, G, Gkv, Dws, g, mod, Tq, KBq, KBk, s);
}

// the workspace of an accepted plan with V = 1: D [N, H, Tq]
static size_t attention_backward_bytes(const AttPlan &p) { return p.bytes - p.lse_bytes; }

} // namespace vivit

using namespace vivit;

extern "C" {

size_t vivit_attention_backward_f32_workspace_bytes(int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d) {
  const AttPlan p = attention_plan(1, N, T, H, Hkv, d, ATT_D_MAX);
  return p.status == VIVIT_OK ? attention_backward_bytes(p) : 0;
}

// the refusals of vivit_attention_forward_f32, in its order, then the workspace; softcap > 0 or 0 (none), bias [H, 2 T - 1] or null
int vivit_attention_backward_f32(const float *dout, const float *qkv, const float *out, const float *lse, float *dqkv, int64_t N,
                                 int64_t T, int64_t H, int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths,
                                 int64_t window, float softcap, const float *bias, void *workspace, size_t workspace_bytes,
                                 void *stream) {
  if (!(softcap >= 0.f) || isinf(softcap)) return VIVIT_E_BADARG;   // (negative, NaN, inf)
  if (!dout || !qkv || !out || !lse || !dqkv || window < 0) return VIVIT_E_BADARG;
  const AttPlan p = attention_plan(1, N, T, H, Hkv, d, ATT_D_MAX);
  if (p.status != VIVIT_OK) return p.status;
  if (!workspace || workspace_bytes < attention_backward_bytes(p)) return VIVIT_E_WORKSPACE;
  AttGeom g = attention_self_geom(dout, qkv, N, T, H, Hkv, d, p.KB, scale, causal, lengths, window);
  g.vec = g.vec && att_aligned16(out);
  float *Dws = static_cast<float *>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (softcap == 0.f && !bias) return attention_backward_launch_d(dout, qkv, out, lse, dqkv, dqkv, Dws, g, AttPlain{}, T, p.KB, p.KB, s);
  return attention_backward_launch_d(dout, qkv, out, lse, dqkv, dqkv, Dws, g, AttScoreMod{softcap, bias}, T, p.KB, p.KB, s);
}

size_t vivit_attention_cross_backward_f32_workspace_bytes(int64_t N, int64_t Tq, int64_t Tk, int64_t H, int64_t Hkv, int64_t d) {
  int64_t KBk = 0;
  const AttPlan p = attention_cross_plan(1, N, Tq, Tk, H, Hkv, d, KBk);
  return p.status == VIVIT_OK ? attention_backward_bytes(p) : 0;
}

// the refusals of vivit_attention_cross_forward_f32, in its order, then the workspace; dq or dkv may be null, not both
int vivit_attention_cross_backward_f32(const float *dout, const float *q, const float *kv, const float *out, const float *lse, float *dq,
                                       float *dkv, int64_t N, int64_t Tq, int64_t Tk, int64_t H, int64_t Hkv, int64_t d, float scale,
                                       const int32_t *q_lengths, const int32_t *k_lengths, void *workspace, size_t workspace_bytes,
                                       void *stream) {
  if (!dout || !q || !kv || !out || !lse || (!dq && !dkv)) return VIVIT_E_BADARG;
  int64_t KBk = 0;
  const AttPlan p = attention_cross_plan(1, N, Tq, Tk, H, Hkv, d, KBk);
  if (p.status != VIVIT_OK) return p.status;
  if (!workspace || workspace_bytes < attention_backward_bytes(p)) return VIVIT_E_WORKSPACE;
  AttGeomX g = attention_cross_geom(dout, q, kv, dkv, N, Tq, Tk, H, Hkv, d, p.KB, KBk, scale, q_lengths, k_lengths);
  g.vec = g.vec && att_aligned16(out);
  return attention_backward_launch_d(dout, q, out, lse, dq, dkv, static_cast<float *>(workspace), g, AttPlain{}, Tq, p.KB, KBk,
                                     static_cast<hipStream_t>(stream));
}

} // extern "C"
