// Scaled dot-product self-attention for head dimensions 129 .. 256: the rule, the mask, the score modifiers and the contract of
// attention.hip (its head; nothing is restated here), with owners whose work split fits a CU's 160 KB of LDS at this width.
//
// The score tiles S = Q K^T and dP = dO V^T contract over all d columns but are 32 x 32; the results dQ, dK and dV are independent
// per column.  So an owner keeps its RESIDENT operands in LDS at full width (pitch 260) and streams the VISITING ones in column
// HALVES of 128 (pitch 132):
//   attn_wide_dkv_kernel   key-block owner of one (n, kv head): K and V of its 32 keys resident; per (query head, query block) step
//                          PASS 1  half 0 then half 1 of Q and of the dO of its VC factor rows: the wave's S tile and its VC dP tiles
//                                  are accumulated IN REGISTERS across the halves (dP in four chains: att_wide_tile_nt4), then P and dS go
//                                  to the 32 x 36 LDS tiles;
//                          PASS 2  half 1 (still in LDS), then half 0 reloaded: dV_c += P^T dO_c, dK_c += dS^T Q_c for the columns c of
//                                  that half.
//   attn_wide_dq_kernel    query-block owner of one (n, h): Q and the dO of its VC factor rows resident; per key block pass 1 over the
//                          halves of K and V, pass 2 dQ_c += dS K_c over half 1, then half 0 of K reloaded (V is read once).
// Q and dO (K for the query owner) are therefore read 1.5 times.  The lse launch is the instance attn_lse_kernel<16, ...> of
// attention_common.h; the row dots D are attn_rowdot_kernel with its chain in fp64 (the launch, below).
// THE S TILE HAS THE BITS OF att_tile_nt<16>: that function runs two interleaved chains, steps c = 0, 8, 16 .. into the first and
// c = 4, 12, .. into the second, a last odd step of four into the first, and adds them; att_wide_tile_nt carries the two chains
// across the halves, and 128 is a multiple of 8, so every MFMA has the operands, the accumulator and the place in its chain that
// it has in the lse launch: exp(s - lse) sees the very s that lse summed.
// SUMMATION ORDER of an output element: that of attention.hip (heads, then blocks, then k within the block, ascending); the halves
// split columns of the results, never a sum.  No atomics; dead positions are never loaded; their rows of G are written as +0.
// LDS (VC = 2): key owner 2 x 33 280 (K, V) + 16 896 (Q half) + 2 x 16 896 (dO halves) + 3 x 4 608 (P, dS) + 384 = 131 456 bytes;
// query owner 3 x 33 280 (Q, dO) + 2 x 16 896 (K, V halves) + 2 x 4 608 (dS) + 384 = 143 232 bytes: one workgroup of four waves
// per CU either way.
#include "attention_wide_common.h"

namespace vivit {

constexpr int ATT_WIDE_VC = AttWF::VC;
static_assert(ATT_WIDE_VC == 2 && AttWH::VC == ATT_WIDE_VC && AttWH::DP == ATT_WIDE_HALF && AttWH::TPW == 4, "the halves of the wide owners");
constexpr int ATT_WIDE_DKV_FLOATS = 2 * AttWF::BLK + (1 + ATT_WIDE_VC) * AttWH::BLK + (1 + ATT_WIDE_VC) * AttWF::TILE + ATT_B + ATT_WIDE_VC * ATT_B;
constexpr int ATT_WIDE_DQ_FLOATS = (1 + ATT_WIDE_VC) * AttWF::BLK + 2 * AttWH::BLK + ATT_WIDE_VC * AttWF::TILE + ATT_B + ATT_WIDE_VC * ATT_B;
static_assert(ATT_WIDE_DKV_FLOATS * 4 <= 160 * 1024 && ATT_WIDE_DQ_FLOATS * 4 <= 160 * 1024, "a CU has 160 KB of LDS");

// half `half` of the dO blocks of the workgroup's factor rows for the query block at i0
__device__ __forceinline__ void att_wide_load_factor_half(float *__restrict__ sdO, const float *__restrict__ M, const AttGeom &g, int Tn,
                                                          int64_t v0, int nv, int64_t n, int h, int i0, int half) {
  const int64_t E = (int64_t)g.H * g.d;
#pragma unroll
  for (int vi = 0; vi < ATT_WIDE_VC; ++vi)
    if (vi < nv)
      att_wide_load_half(sdO + vi * AttWH::BLK, M + ((v0 + vi) * g.N + n) * g.T * E + (int64_t)h * g.d, E, i0, Tn, g.d, g.vec, half);
}

// lse and D of the workgroup's factor rows for the query block at i0 (rows >= Tn: zero)
__device__ __forceinline__ void att_wide_load_stats(float *__restrict__ sL, float *__restrict__ sD, const float *__restrict__ lse,
                                                    const float *__restrict__ Dws, const AttGeom &g, int Tn, int64_t v0, int nv, int64_t n,
                                                    int h, int i0) {
  const int tid = threadIdx.x;
  if (tid < ATT_B) {
    sL[tid] = i0 + tid < Tn ? lse[(n * g.H + h) * g.T + i0 + tid] : 0.f;
#pragma unroll
    for (int vi = 0; vi < ATT_WIDE_VC; ++vi)
      if (vi < nv) sD[vi * ATT_B + tid] = i0 + tid < Tn ? Dws[(((v0 + vi) * g.N + n) * g.H + h) * g.T + i0 + tid] : 0.f;
  }
}

// ---- key-block owner: dK and dV ---------------------------------------------------------------------------------------------------
template <class Mod>
__global__ __launch_bounds__(256) void attn_wide_dkv_kernel(const float *__restrict__ M, const float *__restrict__ qkv,
                                                            const float *__restrict__ lse, const float *__restrict__ Dws,
                                                            float *__restrict__ G, int64_t V, AttGeom g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  constexpr int VC = ATT_WIDE_VC, FL = AttWF::LD, HL = AttWH::LD, HBLK = AttWH::BLK, TILE = AttWF::TILE;
  float *sK = att_smem, *sV = sK + AttWF::BLK, *sQ = sV + AttWF::BLK, *sdO = sQ + HBLK;
  float *sP = sdO + VC * HBLK, *sdS = sP + TILE, *sL = sdS + VC * TILE, *sD = sL + ATT_B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ng = blockIdx.x / g.KB;
  const int jb = (int)(blockIdx.x - ng * g.KB), j0 = jb * ATT_B;
  const int64_t n = ng / g.Hkv;
  const int kv = (int)(ng - n * g.Hkv), dk = (g.d + 3) & ~3;
  const int64_t pitch = g.pitch;
  const int64_t v0 = (int64_t)blockIdx.y * VC;
  const int nv = V - v0 < VC ? (int)(V - v0) : VC;
  const float *base = att_q_rows(g, qkv, n);
  const AttLive L = att_live(g, n);
  // the query blocks that see this key block (the head of attention.hip); a dead key block has none, loads nothing and stores zeros
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
  att_f32x4 accK[VC][2][4], accV[VC][2][4];   // [factor row][half][tile of the wave]
#pragma unroll
  for (int vi = 0; vi < VC; ++vi)
#pragma unroll
    for (int hp = 0; hp < 2; ++hp)
#pragma unroll
      for (int u = 0; u < 4; ++u) accK[vi][hp][u] = accV[vi][hp][u] = zero;
  for (int step = 0; step < g.R * per_head; ++step) {
    const int hr = step / per_head, ib = ib_lo + step - hr * per_head;
    const int h = kv * g.R + hr, i0 = ib * ATT_B;
    const float *qh = base + (int64_t)h * g.d;
    // pass 1: S and dP of the wave's 16 x 16 part, in registers across the halves
    att_f32x4 s0 = zero, s1 = zero, dp[VC][4];
#pragma unroll
    for (int vi = 0; vi < VC; ++vi)
#pragma unroll
      for (int u = 0; u < 4; ++u) dp[vi][u] = zero;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      __syncthreads();   // what stood in the half blocks (and, at half 0, in the tiles) has been read
      att_wide_load_half(sQ, qh, pitch, i0, L.q, g.d, g.vec, half);
      att_wide_load_factor_half(sdO, M, g, L.q, v0, nv, n, h, i0, half);
      if (half == 0) att_wide_load_stats(sL, sD, lse, Dws, g, L.q, v0, nv, n, h, i0);
      __syncthreads();
      const int nc = half == 0 ? ATT_WIDE_HALF : dk - ATT_WIDE_HALF;
      att_wide_tile_nt<HL, FL>(sQ + 16 * ri * HL, sK + 16 * cj * FL + ATT_WIDE_HALF * half, nc, lane, s0, s1);
#pragma unroll
      for (int vi = 0; vi < VC; ++vi)
        if (vi < nv)
          att_wide_tile_nt4<HL, FL>(sdO + vi * HBLK + 16 * ri * HL, sV + 16 * cj * FL + ATT_WIDE_HALF * half, nc, lane, dp[vi]);
    }
    const att_f32x4 s = s0 + s1;
    const float *brow = att_bias_row(mod, g.T, h);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * ri + 4 * kq + e, c = 16 * cj + j;
      float keep = 1.f;
      const float p = i0 + r >= q_lo && i0 + r <= q_hi ? expf(att_logit(mod, s[e], g.scale, brow, j0 - i0 + c - r, keep) - sL[r]) : 0.f;
      const float w = att_dz_weight(mod, p, keep);
      sP[r * ATT_LDP + c] = p;
#pragma unroll
      for (int vi = 0; vi < VC; ++vi)
        if (vi < nv) sdS[vi * TILE + r * ATT_LDP + c] = w * (((dp[vi][0][e] + dp[vi][1][e]) + (dp[vi][2][e] + dp[vi][3][e])) - sD[vi * ATT_B + r]);
    }
    // pass 2: the columns of half 1, whose Q and dO are in LDS, then those of half 0
#pragma unroll
    for (int hp = 1; hp >= 0; --hp) {
      __syncthreads();   // P and dS are written (hp = 1); half 1 has been read (hp = 0)
      if (hp == 0) {
        att_wide_load_half(sQ, qh, pitch, i0, L.q, g.d, g.vec, 0);
        att_wide_load_factor_half(sdO, M, g, L.q, v0, nv, n, h, i0, 0);
        __syncthreads();
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
        if (ATT_WIDE_HALF * hp + 16 * ct < g.d) {
#pragma unroll
          for (int vi = 0; vi < VC; ++vi)
            if (vi < nv) {
              accV[vi][hp][u] = att_acc_tn<8>(sP, sdO + vi * HBLK, rt, ct, lane, accV[vi][hp][u]);
              accK[vi][hp][u] = att_acc_tn<8>(sdS + vi * TILE, sQ, rt, ct, lane, accK[vi][hp][u]);
            }
        }
      }
    }
  }
#pragma unroll
  for (int hp = 0; hp < 2; ++hp)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = ATT_WIDE_HALF * hp + 16 * ct + j;
      if (c < g.d) {
#pragma unroll
        for (int vi = 0; vi < VC; ++vi)
          if (vi < nv) {
            float *gk = att_q_rows(g, G, (v0 + vi) * g.N + n) + g.koff + (int64_t)kv * g.d + c;
            const int k_to_v = att_k_to_v(g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = j0 + 16 * rt + 4 * kq + e;
              if (r < g.T) {   // (a dead key's row: +0 whatever the sign of the scale)
                gk[(int64_t)r * pitch] = r < L.k ? g.scale * accK[vi][hp][u][e] : 0.f;
                gk[(int64_t)r * pitch + k_to_v] = r < L.k ? accV[vi][hp][u][e] : 0.f;
              }
            }
          }
      }
    }
}

// ---- query-block owner: dQ --------------------------------------------------------------------------------------------------------
template <class Mod>
__global__ __launch_bounds__(256) void attn_wide_dq_kernel(const float *__restrict__ M, const float *__restrict__ qkv,
                                                           const float *__restrict__ lse, const float *__restrict__ Dws,
                                                           float *__restrict__ G, int64_t V, AttGeom g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  constexpr int VC = ATT_WIDE_VC, FL = AttWF::LD, FBLK = AttWF::BLK, HL = AttWH::LD, HBLK = AttWH::BLK, TILE = AttWF::TILE;
  float *sQ = att_smem, *sdO = sQ + FBLK, *sK = sdO + VC * FBLK, *sV = sK + HBLK;
  float *sdS = sV + HBLK, *sL = sdS + VC * TILE, *sD = sL + ATT_B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t nh = blockIdx.x / g.KB;
  const int ib = (int)(blockIdx.x - nh * g.KB), i0 = ib * ATT_B;
  const int64_t n = nh / g.H;
  const int h = (int)(nh - n * g.H), dk = (g.d + 3) & ~3;
  const int64_t pitch = g.pitch;
  const int64_t v0 = (int64_t)blockIdx.y * VC;
  const int nv = V - v0 < VC ? (int)(V - v0) : VC;
  const float *base = att_q_rows(g, qkv, n), *kbase = base + g.koff + (int64_t)(h / g.R) * g.d;
  const AttLive L = att_live(g, n);
  // the key blocks this query block sees; a dead query block has none, loads nothing and stores its zeros
  const int KBn = (L.k + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int jb_lo = max(ib - wb, 0), jb_hi = i0 < L.q ? (att_causal(g) ? ib : min(ib + wb, KBn - 1)) : -1;
  if (jb_lo <= jb_hi) {
    const int64_t E = (int64_t)g.H * g.d;
    att_load_block<16>(sQ, base + (int64_t)h * g.d, pitch, i0, L.q, g.d, g.vec);
#pragma unroll
    for (int vi = 0; vi < VC; ++vi)
      if (vi < nv)
        att_load_block<16>(sdO + vi * FBLK, M + ((v0 + vi) * g.N + n) * g.T * E + (int64_t)h * g.d, E, i0, L.q, g.d, g.vec);
    att_wide_load_stats(sL, sD, lse, Dws, g, L.q, v0, nv, n, h, i0);
  }
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  const float *brow = att_bias_row(mod, g.T, h);
  const att_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  att_f32x4 accQ[VC][2][4];   // [factor row][half][tile of the wave]
#pragma unroll
  for (int vi = 0; vi < VC; ++vi)
#pragma unroll
    for (int hp = 0; hp < 2; ++hp)
#pragma unroll
      for (int u = 0; u < 4; ++u) accQ[vi][hp][u] = zero;
  for (int jb = jb_lo; jb <= jb_hi; ++jb) {
    const int j0 = jb * ATT_B;
    att_f32x4 s0 = zero, s1 = zero, dp[VC][4];
#pragma unroll
    for (int vi = 0; vi < VC; ++vi)
#pragma unroll
      for (int u = 0; u < 4; ++u) dp[vi][u] = zero;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      __syncthreads();   // what stood in the half blocks (and, at half 0, in the tiles) has been read
      att_wide_load_half(sK, kbase, pitch, j0, L.k, g.d, g.vec, half);
      att_wide_load_half(sV, kbase + att_k_to_v(g), pitch, j0, L.k, g.d, g.vec, half);
      __syncthreads();
      const int nc = half == 0 ? ATT_WIDE_HALF : dk - ATT_WIDE_HALF;
      att_wide_tile_nt<FL, HL>(sQ + 16 * ri * FL + ATT_WIDE_HALF * half, sK + 16 * cj * HL, nc, lane, s0, s1);
#pragma unroll
      for (int vi = 0; vi < VC; ++vi)
        if (vi < nv)
          att_wide_tile_nt4<FL, HL>(sdO + vi * FBLK + 16 * ri * FL + ATT_WIDE_HALF * half, sV + 16 * cj * HL, nc, lane, dp[vi]);
    }
    const att_f32x4 s = s0 + s1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * ri + 4 * kq + e, c = 16 * cj + j;
      float keep = 1.f;
      const float p = att_valid(g, L, i0 + r, j0 + c) ? expf(att_logit(mod, s[e], g.scale, brow, j0 - i0 + c - r, keep) - sL[r]) : 0.f;
      const float w = att_dz_weight(mod, p, keep);
#pragma unroll
      for (int vi = 0; vi < VC; ++vi)
        if (vi < nv) sdS[vi * TILE + r * ATT_LDP + c] = w * (((dp[vi][0][e] + dp[vi][1][e]) + (dp[vi][2][e] + dp[vi][3][e])) - sD[vi * ATT_B + r]);
    }
#pragma unroll
    for (int hp = 1; hp >= 0; --hp) {
      __syncthreads();   // dS is written (hp = 1); half 1 of K has been read (hp = 0)
      if (hp == 0) {
        att_wide_load_half(sK, kbase, pitch, j0, L.k, g.d, g.vec, 0);
        __syncthreads();
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
        if (ATT_WIDE_HALF * hp + 16 * ct < g.d) {
#pragma unroll
          for (int vi = 0; vi < VC; ++vi)
            if (vi < nv) accQ[vi][hp][u] = att_acc_nn<8>(sdS + vi * TILE, sK, rt, ct, lane, accQ[vi][hp][u]);
        }
      }
    }
  }
#pragma unroll
  for (int hp = 0; hp < 2; ++hp)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = ATT_WIDE_HALF * hp + 16 * ct + j;
      if (c < g.d) {
#pragma unroll
        for (int vi = 0; vi < VC; ++vi)
          if (vi < nv) {
            float *gq = att_q_rows(g, G, (v0 + vi) * g.N + n) + (int64_t)h * g.d + c;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = i0 + 16 * rt + 4 * kq + e;
              if (r < g.T) gq[(int64_t)r * pitch] = r < L.q ? g.scale * accQ[vi][hp][u][e] : 0.f;   // (a dead query's row: +0)
            }
          }
      }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
template <class Mod>
static int attention_wide_launch(const float *M, const float *qkv, const float *out, float *G, float *lse, float *Dws, int64_t V,
                                 const AttGeom &g, const Mod &mod, hipStream_t s) {
  static unsigned long long attr_done = 0;
  constexpr int lse_lds = AttWF::LSE_FLOATS * 4, dkv_lds = ATT_WIDE_DKV_FLOATS * 4, dq_lds = ATT_WIDE_DQ_FLOATS * 4;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
  if (!ensure_dynamic_lds(reinterpret_cast<const void *>(attn_lse_kernel<16, AttGeom, Mod>), lse_lds, attr_done) ||
      !ensure_dynamic_lds(reinterpret_cast<const void *>(attn_wide_dkv_kernel<Mod>), dkv_lds, attr_done) ||
      !ensure_dynamic_lds(reinterpret_cast<const void *>(attn_wide_dq_kernel<Mod>), dq_lds, attr_done))
    return VIVIT_E_LAUNCH;
  attr_done |= 1ull << (dev & 63);
  const int64_t NH = (int64_t)g.N * g.H, total = V * NH * g.T;
  const unsigned blocks = (unsigned)(NH * g.KB), kv_blocks = (unsigned)((int64_t)g.N * g.Hkv * g.KB);
  const unsigned chunks = (unsigned)cdiv(V, ATT_WIDE_VC);
  attn_lse_kernel<16, AttGeom, Mod><<<blocks, 256, lse_lds, s>>>(qkv, lse, g, mod);
  // D in fp64, rounded once: dS = P o (dP - D) subtracts two sums over up to 256 columns that nearly cancel (att_wide_tile_nt4), and
  // one fp32 chain of d steps carries several times the error of the chains of dP.  The launch is bound by reading M and O.
  attn_rowdot_kernel<AttGeom, double><<<(unsigned)cdiv(total, 256), 256, 0, s>>>(M, out, Dws, total, g);
  attn_wide_dkv_kernel<Mod><<<dim3(kv_blocks, chunks), 256, dkv_lds, s>>>(M, qkv, lse, Dws, G, V, g, mod);
  attn_wide_dq_kernel<Mod><<<dim3(blocks, chunks), 256, dq_lds, s>>>(M, qkv, lse, Dws, G, V, g, mod);
  return launch_status();
}

} // namespace vivit

using namespace vivit;

extern "C" {

size_t vivit_attention_wide_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d) {
  const AttPlan p = attention_wide_plan(V, N, T, H, Hkv, d);
  return p.status == VIVIT_OK ? p.bytes : 0;
}

// the arguments, their meaning and the order of the refusals of vivit_attention_scoremod_jac_t_f32, for 128 < d <= 256
int vivit_attention_wide_jac_t_f32(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T,
                                   int64_t H, int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths, int64_t window,
                                   float softcap, const float *bias, void *workspace, size_t workspace_bytes, void *stream) {
  if (!(softcap >= 0.f) || isinf(softcap)) return VIVIT_E_BADARG;   // (negative, NaN, inf)
  if (!M || !qkv || !out || !G || window < 0) return VIVIT_E_BADARG;
  const AttPlan p = attention_wide_plan(V, N, T, H, Hkv, d);
  if (p.status != VIVIT_OK) return p.status;
  if (!workspace || workspace_bytes < p.bytes) return VIVIT_E_WORKSPACE;
  const AttGeom g = attention_self_geom(M, qkv, N, T, H, Hkv, d, p.KB, scale, causal, lengths, window);
  float *lse = static_cast<float *>(workspace);
  float *Dws = reinterpret_cast<float *>(static_cast<char *>(workspace) + p.lse_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (softcap == 0.f && !bias) return attention_wide_launch(M, qkv, out, G, lse, Dws, V, g, AttPlain{}, s);
  return attention_wide_launch(M, qkv, out, G, lse, Dws, V, g, AttScoreMod{softcap, bias}, s);
}

} // extern "C"
