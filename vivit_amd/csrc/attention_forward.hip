// Scaled dot-product attention, the FORWARD pass (vivit_attention_forward_f32, vivit_attention_cross_forward_f32): the function whose
// transposed Jacobian attention.hip applies, flash-style, on the helpers of attention_common.h.  The layouts, the mask, the dead
// positions, the block ranges, the two geometries and the score function are those at the head of attention.hip.  Per sample n and
// query head h of group g = h / R, with z = scale q k^T:
//   u = c tanh(z / c)  (no cap: u = z),   s_ij = u + B[h, j - i + T - 1]  (no table: s = u),   then the mask (att_valid),
//   P = softmax_rows(s),   out[n, i, h d ..] = P V_g,   lse[n, h, i] = log sum_j exp(s_ij)  (where the caller asks for it).
// No T x T (or Tq x Tk) datum is written to memory, there is no workspace, there are no atomics.  One launch:
//   attn_fwd_kernel   the QUERY-block owner of one (n, h, block of 32 queries) -- the grid of attn_lse_kernel: Q of its queries stays
//                     in LDS, it walks the key blocks jb_lo .. jb_hi of head h / R in ascending order (BLOCK RANGES at the head of
//                     attention.hip: no other tile is visited) and, per key block,
//                       1. loads K and V of the 32 keys into LDS (rows beyond the live keys: zeros, never read from memory),
//                       2. S tile: one 16 x 16 tile per wave on v_mfma_f32_16x16x4_f32 (att_tile_nt), the logit of every visible
//                          pair (att_logit) and -inf for the others into the LDS tile sP [32][ATT_LDP],
//                       3. online softmax, eight lanes per row and four columns per lane, the running (m, l) of the row in the
//                          registers of its eight lanes: m_new = max(m, tile), p = exp(s - m_new) back into the lane's own four
//                          words of sP, alpha = exp(m - m_new) into sR[row], l = l alpha + sum p   (a row with nothing unmasked so
//                          far subtracts 0 instead of -inf, as attn_lse_kernel does: every term is then exp(-inf) = 0),
//                       4. the output accumulator [32][16 NT], TPW 16 x 16 tiles per wave in MFMA accumulator registers across the
//                          whole walk, is multiplied by alpha of its rows and then O += P V (att_acc_nn).
//                     After the walk O / l is written for the columns < d of the live rows and lse = m + log l.
// LDS: Q, K and V blocks [32][16 NT + 4], the tile and the 32 row factors -- 12.1, 18.1, 30.1 and 54.1 KB for NT = 1, 2, 4, 8.  K and V
// are NOT double-buffered: at d = 128 a second pair would take the workgroup to 88 KB and the CU (160 KB) to ONE workgroup, whose four
// waves then wait at each of the four barriers of a key block with nothing else to run; single-buffered, two workgroups (NT = 8) to
// five and more (NT <= 4) share a CU and one's loads run under another's products.
// SUMMATION ORDER of an output element: key blocks ascending, inside a block k ascending in steps of four (att_acc_nn); l: the eight
// lanes' partial sums of four, folded by a butterfly, block after block.  So the bytes of out[n] and lse[n] depend on (T, H, Hkv, d,
// scale, causal, the length of n, the window, the cap, the table) and the data of sample n only; with lengths, out[n, :Tn] has the
// bytes of the sample cut to Tn and run alone (masked pairs are p = +0 times a zero row of V: they add +0).
// DEAD POSITIONS: no operand row of a dead position is loaded; rows of dead queries are written as +0 in out and in lse (a block
// with no live query loads nothing at all).  A live query sees itself (self-attention) or every live key (cross-attention: Lk > 0),
// so l > 0 where the division happens.  Every row < T of out has exactly one writer: out may be uninitialised memory.
#include "attention_common.h"

namespace vivit {

template <int NT> struct AttFwdCfg {
  using C = AttCfg<NT>;
  static constexpr int FLOATS = 3 * C::BLK + C::TILE + ATT_B;   // Q, K, V; the tile S -> P; the row factors alpha, then l
};
static_assert(AttFwdCfg<8>::FLOATS * 4 <= 64 * 1024, "no instance asks for more than the default dynamic LDS limit");

template <int NT, class Geo, class Mod>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float *__restrict__ qkv, float *__restrict__ out, float *__restrict__ lse,
                                                       Geo g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  using C = AttCfg<NT>;
  float *sQ = att_smem, *sK = sQ + C::BLK, *sV = sK + C::BLK, *sP = sV + C::BLK, *sR = sP + C::TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t nh = blockIdx.x / att_KBq(g);
  const int ib = (int)(blockIdx.x - nh * att_KBq(g)), i0 = ib * ATT_B;
  const int64_t n = nh / g.H;
  const int h = (int)(nh - n * g.H), dk = (g.d + 3) & ~3, Tq = att_Tq(g);
  const int64_t E = (int64_t)g.H * g.d;
  const AttLive L = att_live(g, n);
  float *orow = out + (n * Tq + i0) * E + (int64_t)h * g.d;   // row 0 of the block, column 0 of the head
  float *lrow = lse ? lse + nh * Tq + i0 : nullptr;
  if (i0 >= L.q) {   // a block with no live query: nothing is loaded, its rows are +0
    for (int idx = tid; idx < ATT_B * g.d; idx += 256) {
      const int r = idx / g.d, c = idx - r * g.d;
      if (i0 + r < Tq) orow[(int64_t)r * E + c] = 0.f;
    }
    if (lrow && tid < ATT_B && i0 + tid < Tq) lrow[tid] = 0.f;
    return;
  }
  const float *base = att_q_rows(g, qkv, n), *kbase = att_k_rows(g, base, n) + (int64_t)(h / g.R) * g.d;
  att_load_block<NT>(sQ, base + (int64_t)h * g.d, att_qpitch(g), i0, L.q, g.d, g.vec);
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  const int row = tid >> 3, sub = tid & 7;
  float m = -INFINITY, l = 0.f;
  att_f32x4 acc[C::TPW];
#pragma unroll
  for (int u = 0; u < C::TPW; ++u) acc[u] = (att_f32x4){0.f, 0.f, 0.f, 0.f};
  const float *brow = att_bias_row(mod, Tq, h);
  const int KBn = (L.k + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int jb_lo = max(ib - wb, 0), jb_hi = att_causal(g) ? ib : min(ib + wb, KBn - 1);
  for (int jb = jb_lo; jb <= jb_hi; ++jb) {
    const int j0 = jb * ATT_B;
    __syncthreads();   // the previous key block's reads of sK, sV, sP and sR are done
    att_load_block<NT>(sK, kbase, att_kpitch(g), j0, L.k, g.d, g.vec);
    att_load_block<NT>(sV, kbase + att_k_to_v(g), att_kpitch(g), j0, L.k, g.d, g.vec);
    __syncthreads();
    const att_f32x4 s = att_tile_nt<NT>(sQ + 16 * ri * C::LD, sK + 16 * cj * C::LD, dk, lane);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * ri + 4 * kq + e, c = 16 * cj + j;
      float keep;
      sP[r * ATT_LDP + c] = att_valid(g, L, i0 + r, j0 + c) ? att_logit(mod, s[e], g.scale, brow, j0 - i0 + c - r, keep) : -INFINITY;
    }
    __syncthreads();
    // eight lanes per row, four columns each; every lane of a row keeps the same (m, l)
    float *prow = sP + row * ATT_LDP + 4 * sub;
    const att_f32x4 x = *reinterpret_cast<const att_f32x4 *>(prow);
    float tm = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) tm = fmaxf(tm, __shfl_xor(tm, off, 64));
    const float mn = fmaxf(m, tm);
    const float mref = mn == -INFINITY ? 0.f : mn;   // (a row with nothing unmasked so far: every term below is exp(-inf) = 0)
    const att_f32x4 p = {expf(x[0] - mref), expf(x[1] - mref), expf(x[2] - mref), expf(x[3] - mref)};
    *reinterpret_cast<att_f32x4 *>(prow) = p;
    float ts = ((p[0] + p[1]) + p[2]) + p[3];
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) ts += __shfl_xor(ts, off, 64);
    const float alpha = expf(m - mref);
    if (sub == 0) sR[row] = alpha;
    l = l * alpha + ts;
    m = mn;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < C::TPW; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
      if (t < 2 * NT && 16 * ct < g.d) {
        const att_f32x4 a = *reinterpret_cast<const att_f32x4 *>(sR + 16 * rt + 4 * kq);
        acc[u] = att_acc_nn<NT>(sP, sV, rt, ct, lane, acc[u] * a);
      }
    }
  }
  __syncthreads();   // the last key block's reads of sR are done
  if (sub == 0) {
    sR[row] = l;
    if (lrow && i0 + row < Tq) lrow[row] = i0 + row < L.q ? m + logf(l) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < C::TPW; ++u) {
    const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = 16 * ct + j;
    if (t < 2 * NT && c < g.d) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 16 * rt + 4 * kq + e;
        if (i0 + r < Tq) orow[(int64_t)r * E + c] = i0 + r < L.q ? acc[u][e] / sR[r] : 0.f;   // (a dead query's row: +0)
      }
    }
  }
}

template <int NT, class Geo, class Mod>
static int attention_forward_launch(const float *qkv, float *out, float *lse, const Geo &g, const Mod &mod, int64_t KBq, hipStream_t s) {
  const unsigned blocks = (unsigned)((int64_t)g.N * g.H * KBq);
  attn_fwd_kernel<NT, Geo, Mod><<<blocks, 256, AttFwdCfg<NT>::FLOATS * 4, s>>>(qkv, out, lse, g, mod);
  return launch_status();
}

template <class Geo, class Mod>
static int attention_forward_launch_d(const float *qkv, float *out, float *lse, const Geo &g, const Mod &mod, int64_t KBq, hipStream_t s) {
  if (g.d <= 16) return attention_forward_launch<1>(qkv, out, lse, g, mod, KBq, s);
  if (g.d <= 32) return attention_forward_launch<2>(qkv, out, lse, g, mod, KBq, s);
  if (g.d <= 64) return attention_forward_launch<4>(qkv, out, lse, g, mod, KBq, s);
  return attention_forward_launch<8>(qkv, out, lse, g, mod, KBq, s);
}

} // namespace vivit

using namespace vivit;

extern "C" {

// the refusals of vivit_attention_scoremod_jac_t_f32 with V = 1, in its order; softcap > 0 or 0 (none), bias [H, 2 T - 1] or null
int vivit_attention_forward_f32(const float *qkv, float *out, float *lse, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d,
                                float scale, int causal, const int32_t *lengths, int64_t window, float softcap, const float *bias,
                                void *stream) {
  if (!(softcap >= 0.f) || isinf(softcap)) return VIVIT_E_BADARG;   // (negative, NaN, inf)
  if (!qkv || !out || window < 0) return VIVIT_E_BADARG;
  const AttPlan p = attention_plan(1, N, T, H, Hkv, d, ATT_D_MAX);
  if (p.status != VIVIT_OK) return p.status;
  const AttGeom g = attention_self_geom(qkv, qkv, N, T, H, Hkv, d, p.KB, scale, causal, lengths, window);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (softcap == 0.f && !bias) return attention_forward_launch_d(qkv, out, lse, g, AttPlain{}, p.KB, s);
  return attention_forward_launch_d(qkv, out, lse, g, AttScoreMod{softcap, bias}, p.KB, s);
}

// the refusals of vivit_attention_cross_jac_t_f32 with V = 1, in its order
int vivit_attention_cross_forward_f32(const float *q, const float *kv, float *out, float *lse, int64_t N, int64_t Tq, int64_t Tk,
                                      int64_t H, int64_t Hkv, int64_t d, float scale, const int32_t *q_lengths,
                                      const int32_t *k_lengths, void *stream) {
  if (!q || !kv || !out) return VIVIT_E_BADARG;
  int64_t KBk = 0;
  const AttPlan p = attention_cross_plan(1, N, Tq, Tk, H, Hkv, d, KBk);
  if (p.status != VIVIT_OK) return p.status;
  const AttGeomX g = attention_cross_geom(q, q, kv, nullptr, N, Tq, Tk, H, Hkv, d, p.KB, KBk, scale, q_lengths, k_lengths);
  return attention_forward_launch_d(q, out, lse, g, AttPlain{}, p.KB, static_cast<hipStream_t>(stream));
}

} // extern "C"
