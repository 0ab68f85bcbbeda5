// Scaled dot-product self-attention: the transposed input Jacobian applied to the sqrt-GGN factor (f1).  The module input is the
// packed projection qkv [N, T, (H + 2 Hkv) d] (q | k | v: H query heads of d columns, then Hkv key heads, then Hkv value heads),
// its output O [N, T, E], E = H d.  Query head h attends to key / value head g = h / R, R = H / Hkv consecutive query heads per
// group (grouped-query attention; Hkv == H is multi-head attention with three equal thirds, Hkv == 1 multi-query attention).
// Per factor row v, sample n and query head h of group g, with dO = M[v, n, :, h]:
//   S = scale Q_h K_g^T (+ mask),  P = softmax_rows(S),  D_i = sum_c dO_ic O_ic,
//   dP = dO V_g^T,  dS = P o (dP - D),  dQ_h = scale dS K_g,
//   dV_g = sum_{h in g} P_h^T dO_h,  dK_g = scale sum_{h in g} dS_h^T Q_h,                     G[v, n] = dQ | dK | dV (packed).
// No T x T data leaves the chip.  Four launches:
//   attn_lse_kernel    lse[n, h, i] = log sum_j exp(S_ij), online over key blocks with the running row maximum subtracted
//   attn_rowdot_kernel D[v, n, h, i]
//   attn_dkv_kernel    the KEY-block owner of one (n, kv head g): K and V of its 32 keys stay in LDS, it walks the query heads
//                      h = g R .. g R + R - 1 in ascending order and, inside each head, the query blocks in ascending order (Q, lse,
//                      dO and D of that head are reloaded), and accumulates dK and dV of the group in the same registers
//   attn_dq_kernel     the QUERY-block owner of one (n, h): Q and dO of its 32 queries stay in LDS, it walks the key blocks of
//                      head h / R and accumulates dQ
// A workgroup (256 threads, four waves) owns one block of one (n, h) -- of one (n, g) for dK and dV -- for VC factor rows at a
// time: the tile P = exp(S - lse) of a (query block, key block) pair is recomputed ONCE per workgroup and multiplies the dO of all
// VC rows; the accumulators of the VC rows live in registers, which is what limits VC.  All products run on
// v_mfma_f32_16x16x4_f32 from LDS tiles whose edges (rows beyond T, columns beyond d) are zero.  No atomics and no second pass.
// SUMMATION ORDER of an output element: head, then block, then k within the block -- for dK and dV the query heads of the group in
// ascending order, inside a head the query blocks in ascending order, inside a block k in ascending order; for dQ (one head) the
// key blocks in ascending order (the S and dP tiles: two interleaved chains, even and odd steps of four, added at the end).  So
// the bytes of G[v, n] depend on (T, H, Hkv, d, scale, causal; the length of n and the window, below) and the data of (v, n) only.
// With Hkv == H the walk over heads has one step: the order, and the bytes, of multi-head attention.
//
// THE MASK.  Sample n has the length Tn = min(max(lengths[n], 0), T) (no lengths: Tn = T; right padding), and a window W >= 1 may
// be given (W = 0: none).  Query i and key j of sample n see each other iff
//   i < Tn and j < Tn,   j <= i when causal,   i - j < W and j - i < W when W > 0                                   (att_valid).
// Positions >= Tn are DEAD: no operand row >= Tn is ever loaded (att_load_block, the lse and D loads zero-fill by Tn; T is the
// stride only), so whatever stands there -- NaN included -- reaches nothing, and rows Tn .. T - 1 of G[v, n] are written as +0.
// BLOCK RANGES.  KBn = ceil(Tn / 32) live blocks, WB = floor((W + 30) / 32).  A tile (query block ib, key block jb), both < KBn, has
// a visible pair iff
//   causal:  jb <= ib  (the pair (32 ib, 32 jb) of block starts; both are live);
//   window:  the smallest i - j of the tile is 32 ib - (32 jb + 31), reached at a live pair when jb < ib (block jb is then full
//            and 32 ib < Tn); it is < W iff 32 (ib - jb) <= W + 30 iff ib - jb <= floor((W + 30) / 32) = WB.  By symmetry the smallest
//            j - i is < W iff jb - ib <= WB.  (W = 1: WB = 0, the diagonal alone.  W = 2 .. 33: WB = 1, since query 32 ib sees key
//            32 ib - 1 from W = 2 on and key 32 ib - 33 of block ib - 2 from W = 34 on, where WB = 2.)
// So the query-block owners (lse, dQ) walk   jb_lo = max(0, ib - WB) .. jb_hi = causal ? ib : min(KBn - 1, ib + WB),
// and the key-block owner walks, per head,    ib_lo = causal ? jb : max(0, jb - WB) .. ib_hi = min(KBn - 1, jb + WB),
// with WB = KBn where W = 0 (no tile is cut).  Every tile outside these ranges is all zero and every tile inside has a visible
// pair, so the sums have the terms and the order they had: with no lengths and no window the bytes of the unmasked kernels, and
// G[v, n, :Tn] has the bytes of the sample cut to Tn and run alone with T = Tn.  A workgroup whose own block starts at or beyond Tn
// has an empty walk: it loads nothing and writes its zero rows of G (G is uninitialised memory: every row < T has one writer).
//
// CROSS-ATTENTION (vivit_attention_cross_jac_t_f32): the queries q [N, Tq, H d] and the keys and values kv [N, Tk, 2 Hkv d] (k | v,
// the packed layout without its query part) are two sequences with a length each, Lq[n] and Lk[n] (right padding, clamped to
// [0, Tq] and [0, Tk]); the results are Gq [V, N, Tq, H d] and Gkv [V, N, Tk, 2 Hkv d] = dK | dV.  There is NO causal flag and NO
// window: with Tq != Tk there is no agreed alignment of the diagonal.  Key j is live iff j < Lk[n], query i iff i < Lq[n] and
// Lk[n] > 0 (a query with no key to look at is dead, not a NaN); a live query sees every live key.  The same four kernels are
// compiled a second time from the geometry AttGeomX: the second sequence -- its base, row pitch, T, block count and lengths -- is
// a COMPILE-TIME variant (the kernels' template parameter Geo and the overloads on it below), so the self-attention instances are compiled from exactly the
// expressions they had and keep their registers (the key owner's scalar file is full).  The query-block owners walk
// the key blocks 0 .. ceil(Lk / 32) - 1, the key-block owner the query blocks 0 .. ceil(Lq / 32) - 1 of each head, in the order
// above: with Tq = Tk, equal lengths and the packed projection split in two, the tiles, the order and the bytes of the non-causal
// self-attention call.  Either result may be left out (a frozen memory needs no Gkv): its owner is not launched.
//
// SCORE MODIFIERS (vivit_attention_scoremod_jac_t_f32; self-attention only): a logit cap c > 0 and a table B [H, 2 T - 1] of biases
// per head and distance.  With z_ij = scale q_i k_j,
//   u = c tanh(z / c)  (no cap: u = z),   s_ij = u + B[h, j - i + T - 1]  (no table: s = u),   then the mask,  P = softmax_rows(s),
//   dS = P o (dP - D),   dZ = dS o (1 - t^2) with t = u / c  (no cap: dZ = dS),   dQ_h = scale dZ K_g,   dK_g = scale sum_h dZ_h^T Q_h,
// and dV as it was; the table is a constant for the input rule; its own factor: the diagonal owner (below).  The variant is COMPILE TIME again: the kernels' second template
// parameter Mod is AttPlain (the expressions that were there; every instance above) or AttScoreMod, whose instances exist for
// AttGeom alone.  att_logit forms s_ij from the product q_i k_j for lse and for both owners, the same operations in the same order and
// none of them contracted with a neighbour, so exp(s - lse) sees the very s that lse summed.  Neither owner keeps a second tile: the
// weight P o (1 - t^2) of (dP - D) is formed in the registers of P once P itself is in LDS (the key owner, for dV) or in its place
// (the query owner, which never uses P alone).  A table entry is read through the caches, for visible pairs only: both positions
// are then < Tn <= T, so j - i + T - 1 stays in [0, 2 T - 2].  Summation order, block ranges, dead positions and +0 rows are those
// above; the bytes of G[v, n] depend on the cap and the table besides.
//
// THE TABLE'S OWN FACTOR (vivit_attention_bias_factor_f32): a learned table is a parameter, and its per-sample factor is
//   Gb[v, n, h, r] = sum_{(i, j) visible, j - i = r} dS[v, n, h, i, j],   dS = P o (dP - D)
// -- the bias is added BEHIND the cap, so it is dS and not dZ that is summed: the diagonal sums of the dS tiles the two owners
// recompute and throw away.  Neither owner's instance is touched (the key owner's scalar file is full); a third owner is launched
// behind the same lse and row-dot launches:
//   attn_dbias_kernel       the DIAGONAL owner of one (n, h): block diagonal delta = jb - ib, -(KB - 1) .. KB - 1; it walks the query
//                           blocks ib in ascending order with jb = ib + delta over exactly the tiles the block ranges above call
//                           non-empty (both blocks < KBn, delta <= 0 when causal, |delta| <= WB), reloads Q, K, V, lse, dO and D per
//                           tile, forms s with att_logit and the mask with att_valid as attn_lse_kernel does, then dS for its VC factor
//                           rows, and adds the 63 diagonals rho = -31 .. 31 of each tile into one register per (vc, rho), i ascending;
//                           at the end partial[v, n, h, delta, rho] (pitch 64), zeros for a diagonal with no tile
//   attn_dbias_fold_kernel  distance r lies on the block diagonals floor(r / 32) at rho = r mod 32 and, for rho >= 1, the next one at
//                           rho - 32; column b of Gb[v, n, h] is ONE chain over the distances with index[r + T - 1] == b, r ascending,
//                           each distance the sum of its two block diagonals, delta ascending.  The index sends distances to columns (a table of maximum length L >= T:
//                           r + L - 1; T5's buckets: many distances to one column); a value outside [0, R) equals no column and is
//                           skipped.
// SUMMATION ORDER: blocks ascending, i ascending inside a block, then the fold's order; no atomics.  The bytes of Gb[v, n] depend on
// the shape parameters, the cap, the table, the index and the data of (v, n) only; a padded sample has the bytes of the sample cut
// to Tn and run alone with the index shifted by T - Tn (masked pairs and diagonals without a tile add zeros, which change no sum
// that starts at +0); dead positions are never loaded; columns no visible distance maps to are +0.  Workspace: 64 floats per
// (v, n, h, block diagonal) behind that of the input rule, O(T) per (v, n, h).
#include <math.h>

#include "common.h"

namespace vivit {

constexpr int ATT_B = 32;          // queries per query block = keys per key block
constexpr int ATT_LDP = 36;        // row pitch of the 32 x 32 tiles P and dS
constexpr int ATT_D_MAX = 128;
typedef float att_f32x4 __attribute__((ext_vector_type(4)));

// NT = column tiles of 16 that hold a head (d <= 16 NT).  VC = factor rows per workgroup.
template <int NT> struct AttCfg {
  static constexpr int DP = 16 * NT;
  static constexpr int LD = DP + 4;                      // row pitch of the [32][d] blocks
  static constexpr int VC = NT >= 4 ? 2 : 4;
  static constexpr int TPW = (2 * NT + 3) / 4;           // 16 x 16 tiles of a [32][DP] result per wave
  static constexpr int BLK = ATT_B * LD;
  static constexpr int TILE = ATT_B * ATT_LDP;
  // floats of LDS: the lse launch holds Q, K and the S tile; the owners hold three operand blocks, VC blocks of dO, P, VC tiles
  // dS, the row statistics lse[32] and D[VC][32]
  static constexpr int LSE_FLOATS = 2 * BLK + ATT_B * 33;
  static constexpr int OWN_FLOATS = (3 + VC) * BLK + (1 + VC) * TILE + ATT_B + VC * ATT_B;
};

// rows r0 .. r0 + 31 of a [T][stride] matrix, columns 0 .. d - 1 from `src` (already offset to the head) -> dst[32][LD]; rows
// beyond T (the sample's live length) and columns d .. DP - 1 are zero and never read.  vec: d % 4 == 0 and every row start is 16-byte aligned.
template <int NT>
__device__ __forceinline__ void att_load_block(float *__restrict__ dst, const float *__restrict__ src, int64_t stride, int r0, int T,
                                               int d, bool vec) {
  constexpr int DP = AttCfg<NT>::DP, LD = AttCfg<NT>::LD;
  const int tid = threadIdx.x;
  if (vec) {
    constexpr int DP4 = DP / 4;
    for (int idx = tid; idx < ATT_B * DP4; idx += 256) {
      const int r = idx / DP4, c = 4 * (idx - r * DP4);
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < T && c < d) q = *reinterpret_cast<const float4 *>(src + (int64_t)(r0 + r) * stride + c);
      *reinterpret_cast<float4 *>(dst + r * LD + c) = q;
    }
  } else {
    for (int idx = tid; idx < ATT_B * DP; idx += 256) {
      const int r = idx / DP, c = idx - r * DP;
      dst[r * LD + c] = (r0 + r < T && c < d) ? src[(int64_t)(r0 + r) * stride + c] : 0.f;
    }
  }
}

// C[i][j] = sum_c A[i][c] B[j][c] for one 16 x 16 tile; A, B: first row of the tile's rows in [..][LD] blocks; dk = d rounded up to 4.
// The lane holds C[4 (lane >> 4) + e][lane & 15], e < 4.
template <int NT>
__device__ __forceinline__ att_f32x4 att_tile_nt(const float *__restrict__ A, const float *__restrict__ B, int dk, int lane) {
  constexpr int LD = AttCfg<NT>::LD;
  const float *a = A + (lane & 15) * LD + (lane >> 4), *b = B + (lane & 15) * LD + (lane >> 4);
  att_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int c = 0;
  for (; c + 8 <= dk; c += 8) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[c], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c + 4], b[c + 4], acc1, 0, 0, 0);
  }
  if (c < dk) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[c], acc0, 0, 0, 0);
  return acc0 + acc1;
}

// acc[r][c] += sum_{k < 32} At[k][r] Bm[k][c]: At a [32][ATT_LDP] tile (k-major), Bm a [32][LD] block; tile (rt, ct) of the result
template <int NT>
__device__ __forceinline__ att_f32x4 att_acc_tn(const float *__restrict__ At, const float *__restrict__ Bm, int rt, int ct, int lane,
                                                att_f32x4 acc) {
  constexpr int LD = AttCfg<NT>::LD;
  const float *a = At + (lane >> 4) * ATT_LDP + 16 * rt + (lane & 15), *b = Bm + (lane >> 4) * LD + 16 * ct + (lane & 15);
#pragma unroll
  for (int k = 0; k < ATT_B; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k * ATT_LDP], b[k * LD], acc, 0, 0, 0);
  return acc;
}

// acc[r][c] += sum_{k < 32} A[r][k] Bm[k][c]: A a [32][ATT_LDP] tile (row-major), Bm a [32][LD] block
template <int NT>
__device__ __forceinline__ att_f32x4 att_acc_nn(const float *__restrict__ A, const float *__restrict__ Bm, int rt, int ct, int lane,
                                                att_f32x4 acc) {
  constexpr int LD = AttCfg<NT>::LD;
  const float *a = A + (16 * rt + (lane & 15)) * ATT_LDP + (lane >> 4), *b = Bm + (lane >> 4) * LD + 16 * ct + (lane & 15);
#pragma unroll
  for (int k = 0; k < ATT_B; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], b[k * LD], acc, 0, 0, 0);
  return acc;
}

struct AttGeom {
  int N, T, H, d, KB;        // KB = blocks of 32 along T
  int Hkv, R;                // key / value heads, query heads per group (H = R Hkv)
  int pitch, koff, voff;     // of a row of qkv and G: (H + 2 Hkv) d columns, k from column H d, v from column (H + Hkv) d
  int causal, vec;
  float scale;
  const int32_t *lengths;    // [N] on the device, or null: every sample has T positions
  int window;                // W >= 1, or 0: none (the host passes 0 for W >= T, so W + 30 stays an int)
};

// the live positions of sample n: an out-of-range length is clamped, so that it can never carry an access out of bounds
__device__ __forceinline__ int att_len(const AttGeom &g, int64_t n) {
  return g.lengths ? min(max(g.lengths[n], 0), g.T) : g.T;
}

// blocks a window reaches to either side of the diagonal (the head of the file); KBn where there is no window
__device__ __forceinline__ int att_reach(const AttGeom &g, int KBn) { return g.window > 0 ? (g.window + 30) >> 5 : KBn; }

struct AttLive { int q, k; };   // live queries and live keys of a sample (self-attention: the same number): rows beyond are never loaded

__device__ __forceinline__ bool att_valid(const AttGeom &g, AttLive L, int gi, int gj) {
  const int dist = gi - gj, Tn = L.q;
  return gi < Tn && gj < Tn && (!g.causal || dist >= 0) && (g.window <= 0 || (dist < g.window && -dist < g.window));
}

// cross-attention (the head of the file): the kernels' first pointer is q, their result Gq; the second sequence travels here
struct AttGeomX {
  int N, Tq, Tk, H, d, KBq, KBk;   // KBq, KBk = blocks of 32 along Tq and Tk
  int Hkv, R;
  int qpitch, kpitch, voff;        // of a row of q and Gq: H d columns; of kv and Gkv: 2 Hkv d columns, v from column Hkv d
  int vec;
  float scale;
  const float *kv;                 // [N, Tk, 2 Hkv d]
  float *Gkv;                      // [V, N, Tk, 2 Hkv d], or null (the key owner is then not launched)
  const int32_t *qlengths, *klengths;   // [N] on the device, or null
};

// WHAT THE KERNELS ASK OF A GEOMETRY, once per kind: self-attention answers every question about the queries and the keys from
// its one sequence (the same expressions the kernels held before there was a second kind), cross-attention from its two.
__device__ __forceinline__ AttLive att_live(const AttGeom &g, int64_t n) {
  const int Tn = att_len(g, n);
  return {Tn, Tn};
}
__device__ __forceinline__ AttLive att_live(const AttGeomX &g, int64_t n) {
  const int k = g.klengths ? min(max(g.klengths[n], 0), g.Tk) : g.Tk, q = g.qlengths ? min(max(g.qlengths[n], 0), g.Tq) : g.Tq;
  return {k > 0 ? q : 0, k};   // (no key to look at: the queries are dead)
}
__device__ __forceinline__ int att_Tq(const AttGeom &g) { return g.T; }
__device__ __forceinline__ int att_Tk(const AttGeom &g) { return g.T; }
__device__ __forceinline__ int att_KBq(const AttGeom &g) { return g.KB; }
__device__ __forceinline__ int att_KBk(const AttGeom &g) { return g.KB; }
__device__ __forceinline__ int64_t att_qpitch(const AttGeom &g) { return g.pitch; }
__device__ __forceinline__ int64_t att_kpitch(const AttGeom &g) { return g.pitch; }
__device__ __forceinline__ int att_k_to_v(const AttGeom &g) { return g.voff - g.koff; }
__device__ __forceinline__ int att_Tq(const AttGeomX &g) { return g.Tq; }
__device__ __forceinline__ int att_Tk(const AttGeomX &g) { return g.Tk; }
__device__ __forceinline__ int att_KBq(const AttGeomX &g) { return g.KBq; }
__device__ __forceinline__ int att_KBk(const AttGeomX &g) { return g.KBk; }
__device__ __forceinline__ int64_t att_qpitch(const AttGeomX &g) { return g.qpitch; }
__device__ __forceinline__ int64_t att_kpitch(const AttGeomX &g) { return g.kpitch; }
__device__ __forceinline__ int att_k_to_v(const AttGeomX &g) { return g.voff; }
// query rows of sample (or factor slice) r: `p` is qkv or G -- q or Gq -- as the kernel was given it
template <class P> __device__ __forceinline__ P att_q_rows(const AttGeom &g, P p, int64_t r) { return p + r * g.T * (int64_t)g.pitch; }
template <class P> __device__ __forceinline__ P att_q_rows(const AttGeomX &g, P p, int64_t r) { return p + r * g.Tq * (int64_t)g.qpitch; }
// key rows and value rows (head 0) of sample r, whose query rows start at `base`; the rows of dK of factor slice r, whose rows of dQ
// start at `gbase` (the rows of dV are att_k_to_v columns on)
__device__ __forceinline__ const float *att_k_rows(const AttGeom &g, const float *base, int64_t) { return base + g.koff; }
__device__ __forceinline__ const float *att_v_rows(const AttGeom &g, const float *base, int64_t) { return base + g.voff; }
__device__ __forceinline__ float *att_gk_rows(const AttGeom &g, float *gbase, int64_t) { return gbase + g.koff; }
__device__ __forceinline__ const float *att_k_rows(const AttGeomX &g, const float *, int64_t r) { return g.kv + r * g.Tk * (int64_t)g.kpitch; }
__device__ __forceinline__ const float *att_v_rows(const AttGeomX &g, const float *, int64_t r) {
  return g.kv + r * g.Tk * (int64_t)g.kpitch + g.voff;
}
__device__ __forceinline__ float *att_gk_rows(const AttGeomX &g, float *, int64_t r) { return g.Gkv + r * g.Tk * (int64_t)g.kpitch; }
// does query gi see key gj
__device__ __forceinline__ bool att_valid(const AttGeomX &, AttLive L, int gi, int gj) { return gi < L.q && gj < L.k; }
// the block ranges of the walks (BLOCK RANGES at the head of the file) are written once, in the kernels, from att_reach and
// att_causal: cross-attention has no window and no diagonal, every block is within reach (ib + reach stays an int: ib < 2^26)
__device__ __forceinline__ int att_reach(const AttGeomX &, int) { return 1 << 30; }
__device__ __forceinline__ bool att_causal(const AttGeom &g) { return g.causal; }
__device__ __forceinline__ bool att_causal(const AttGeomX &) { return false; }
// the queries q_lo .. q_hi that see key gj (empty for a dead key)
__device__ __forceinline__ void att_query_range(const AttGeom &g, AttLive L, int gj, int &q_lo, int &q_hi) {
  const int Tn = L.q, reach = g.window > 0 ? g.window - 1 : Tn;
  q_lo = gj < Tn ? (g.causal ? gj : gj - reach) : 0x7fffffff;
  q_hi = (int)min((int64_t)gj + reach, (int64_t)Tn - 1);
}
__device__ __forceinline__ void att_query_range(const AttGeomX &, AttLive L, int gj, int &q_lo, int &q_hi) {
  q_lo = gj < L.k ? 0 : 0x7fffffff, q_hi = L.q - 1;
}

// ---- the score function (SCORE MODIFIERS at the head of the file) -------------------------------------------------------------------
struct AttPlain {};
struct AttScoreMod {
  float cap;           // c > 0, or 0: none
  const float *bias;   // [H, 2 T - 1] on the device, or null: none
};

// the table row of head h, offset so that it is indexed by j - i in (-T, T)
__device__ __forceinline__ const float *att_bias_row(const AttPlain &, int, int) { return nullptr; }
__device__ __forceinline__ const float *att_bias_row(const AttScoreMod &m, int T, int h) {
  return m.bias ? m.bias + (int64_t)h * (2 * (int64_t)T - 1) + (T - 1) : nullptr;
}

// the logit s_ij of a VISIBLE pair from qk = q_i k_j (dji = j - i, `row` from att_bias_row); keep = 1 - t^2, the factor of dS in dZ
__device__ __forceinline__ float att_logit(const AttPlain &, float qk, float scale, const float *, int, float &) { return qk * scale; }
__device__ __forceinline__ float att_logit(const AttScoreMod &m, float qk, float scale, const float *row, int dji, float &keep) {
#pragma clang fp contract(off)   // (lse stores s, the owners subtract lse from it: no product here may fuse with what follows)
  float u = qk * scale;
  if (m.cap > 0.f) {
    const float t = tanhf(u / m.cap);
    u = m.cap * t;
    keep = 1.f - t * t;
  }
  return row ? u + row[dji] : u;
}
// the weight of (dP - D) in dZ
__device__ __forceinline__ float att_dz_weight(const AttPlain &, float p, float) { return p; }
__device__ __forceinline__ float att_dz_weight(const AttScoreMod &, float p, float keep) { return p * keep; }

// ---- row log-sum-exp --------------------------------------------------------------------------------------------------------------
template <int NT, class Geo, class Mod>
__global__ __launch_bounds__(256) void attn_lse_kernel(const float *__restrict__ qkv, float *__restrict__ lse, Geo g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  using C = AttCfg<NT>;
  float *sQ = att_smem, *sK = sQ + C::BLK, *sS = sK + C::BLK;   // sS [32][33]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t nh = blockIdx.x / att_KBq(g);
  const int ib = (int)(blockIdx.x - nh * att_KBq(g)), i0 = ib * ATT_B;
  const int64_t n = nh / g.H;
  const int h = (int)(nh - n * g.H), dk = (g.d + 3) & ~3;
  const AttLive L = att_live(g, n);
  if (i0 >= L.q) return;   // a dead query block: its lse is never read
  const float *base = att_q_rows(g, qkv, n), *kbase = att_k_rows(g, base, n) + (int64_t)(h / g.R) * g.d;
  att_load_block<NT>(sQ, base + (int64_t)h * g.d, att_qpitch(g), i0, L.q, g.d, g.vec);
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  const int row = tid >> 3, sub = tid & 7;
  float m = -INFINITY, l = 0.f;
  const float *brow = att_bias_row(mod, att_Tq(g), h);
  const int KBn = (L.k + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int jb_lo = max(ib - wb, 0), jb_hi = att_causal(g) ? ib : min(ib + wb, KBn - 1);
  for (int jb = jb_lo; jb <= jb_hi; ++jb) {
    const int j0 = jb * ATT_B;
    __syncthreads();   // the previous block's reads of sK and sS are done
    att_load_block<NT>(sK, kbase, att_kpitch(g), j0, L.k, g.d, g.vec);
    __syncthreads();
    const att_f32x4 s = att_tile_nt<NT>(sQ + 16 * ri * C::LD, sK + 16 * cj * C::LD, dk, lane);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * ri + 4 * kq + e, c = 16 * cj + j;
      float keep;
      sS[r * 33 + c] = att_valid(g, L, i0 + r, j0 + c) ? att_logit(mod, s[e], g.scale, brow, j0 - i0 + c - r, keep) : -INFINITY;
    }
    __syncthreads();
    // eight lanes per row, four columns each; every lane of a row keeps the same (m, l)
    float x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = sS[row * 33 + 4 * sub + q];
    float tm = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) tm = fmaxf(tm, __shfl_xor(tm, off, 64));
    const float mn = fmaxf(m, tm);
    const float mref = mn == -INFINITY ? 0.f : mn;   // (a row with nothing unmasked so far: every term below is exp(-inf) = 0)
    float ts = ((expf(x[0] - mref) + expf(x[1] - mref)) + expf(x[2] - mref)) + expf(x[3] - mref);
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) ts += __shfl_xor(ts, off, 64);
    l = l * expf(m - mref) + ts;
    m = mn;
  }
  if (sub == 0 && i0 + row < L.q) lse[nh * att_Tq(g) + i0 + row] = m + logf(l);
}

// ---- D[v, n, h, i] = sum_c M[v, n, i, h d + c] O[n, i, h d + c], i a live query ---------------------------------------------------
template <class Geo>
__global__ __launch_bounds__(256) void attn_rowdot_kernel(const float *__restrict__ M, const float *__restrict__ O, float *__restrict__ D,
                                                          int64_t total, Geo g) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t T = att_Tq(g), vnh = e / T;
  const int t = (int)(e - vnh * T);
  const int64_t vn = vnh / g.H;
  const int h = (int)(vnh - vn * g.H);
  const int64_t n = vn % g.N, E = (int64_t)g.H * g.d;
  if (t >= att_live(g, n).q) return;   // a dead row: D is never read there
  const float *m = M + (vn * T + t) * E + (int64_t)h * g.d, *o = O + (n * T + t) * E + (int64_t)h * g.d;
  float a = 0.f;
  for (int c = 0; c < g.d; ++c) a = fmaf(m[c], o[c], a);
  D[e] = a;
}

// what the two owners share: the dO blocks and D of the workgroup's factor rows for the query block at i0 (rows >= Tn, the live
// queries: zero)
template <int NT, class Geo>
__device__ __forceinline__ void att_load_factor(float *__restrict__ sdO, float *__restrict__ sD, const float *__restrict__ M,
                                                const float *__restrict__ Dws, const Geo &g, int Tn, int64_t v0, int nv, int64_t n,
                                                int h, int i0) {
  using C = AttCfg<NT>;
  const int64_t E = (int64_t)g.H * g.d;
#pragma unroll
  for (int vi = 0; vi < C::VC; ++vi)
    if (vi < nv) {
      const int64_t vn = (v0 + vi) * g.N + n;
      att_load_block<NT>(sdO + vi * C::BLK, M + vn * att_Tq(g) * E + (int64_t)h * g.d, E, i0, Tn, g.d, g.vec);
      if (threadIdx.x < ATT_B)
        sD[vi * ATT_B + threadIdx.x] = i0 + (int)threadIdx.x < Tn ? Dws[(vn * g.H + h) * att_Tq(g) + i0 + threadIdx.x] : 0.f;
    }
}

// one wave's 16 x 16 part of P = exp(S - lse) for the tile (query block at i0, key block at j0); zero where masked or beyond Tn
// (`visible(r, c)`: att_valid of the pair at row r and column c of the tile, in whatever form the owner keeps it).  `w`: the weight
// of (dP - D) in dZ, P itself without a cap; `brow`, `dj0 = j0 - i0`: the head's table row and the tile's distance for att_logit
template <int NT, class Mod, class Visible>
__device__ __forceinline__ att_f32x4 att_p_tile(const float *__restrict__ sQ, const float *__restrict__ sK, const float *__restrict__ sL,
                                                float scale, int dk, int lane, int ri, int cj, const Mod &mod,
                                                const float *__restrict__ brow, int dj0, att_f32x4 &w, Visible visible) {
  using C = AttCfg<NT>;
  const att_f32x4 s = att_tile_nt<NT>(sQ + 16 * ri * C::LD, sK + 16 * cj * C::LD, dk, lane);
  att_f32x4 p;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = 16 * ri + 4 * (lane >> 4) + e, c = 16 * cj + (lane & 15);
    float keep = 1.f;
    p[e] = visible(r, c) ? expf(att_logit(mod, s[e], scale, brow, dj0 + c - r, keep) - sL[r]) : 0.f;
    w[e] = att_dz_weight(mod, p[e], keep);
  }
  return p;
}

// ---- key-block owner: dK and dV ---------------------------------------------------------------------------------------------------
template <int NT, class Geo, class Mod>
__global__ __launch_bounds__(256) void attn_dkv_kernel(const float *__restrict__ M, const float *__restrict__ qkv,
                                                       const float *__restrict__ lse, const float *__restrict__ Dws, float *__restrict__ G,
                                                       int64_t V, Geo g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  using C = AttCfg<NT>;
  float *sK = att_smem, *sV = sK + C::BLK, *sQ = sV + C::BLK, *sdO = sQ + C::BLK;
  float *sP = sdO + C::VC * C::BLK, *sdS = sP + C::TILE, *sL = sdS + C::VC * C::TILE, *sD = sL + ATT_B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ng = blockIdx.x / att_KBk(g);
  const int jb = (int)(blockIdx.x - ng * att_KBk(g)), j0 = jb * ATT_B;
  const int64_t n = ng / g.Hkv;
  const int kv = (int)(ng - n * g.Hkv), dk = (g.d + 3) & ~3;
  const int64_t qpitch = att_qpitch(g), kpitch = att_kpitch(g);
  const int64_t v0 = (int64_t)blockIdx.y * C::VC;
  const int nv = V - v0 < C::VC ? (int)(V - v0) : C::VC;
  const float *base = att_q_rows(g, qkv, n);
  const AttLive L = att_live(g, n);
  // the query blocks that see this key block (the head of the file); a dead key block (j0 >= L.k) has none, loads nothing and
  // stores its zeros
  const int KBn = (L.q + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int ib_lo = att_causal(g) ? jb : max(jb - wb, 0), ib_hi = min(jb + wb, KBn - 1);
  const int per_head = j0 < L.k ? ib_hi - ib_lo + 1 : 0;
  if (per_head > 0) {
    att_load_block<NT>(sK, att_k_rows(g, base, n) + (int64_t)kv * g.d, kpitch, j0, L.k, g.d, g.vec);
    att_load_block<NT>(sV, att_v_rows(g, base, n) + (int64_t)kv * g.d, kpitch, j0, L.k, g.d, g.vec);
  }
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  // att_valid for the lane's key gj, which is the same in every tile of the walk, as the range q_lo .. q_hi of the queries that see
  // it (empty for a dead key): two registers of the lane instead of Tn, the window and the causal flag in the scalar file, which this
  // kernel fills
  const int gj = j0 + 16 * cj + j;
  int q_lo, q_hi;
  att_query_range(g, L, gj, q_lo, q_hi);
  att_f32x4 accK[C::VC][C::TPW], accV[C::VC][C::TPW];
#pragma unroll
  for (int vi = 0; vi < C::VC; ++vi)
#pragma unroll
    for (int u = 0; u < C::TPW; ++u) accK[vi][u] = accV[vi][u] = (att_f32x4){0.f, 0.f, 0.f, 0.f};
  // the group's query heads in ascending order, the query blocks of each in ascending order: one chain of sums per output element
  for (int step = 0; step < g.R * per_head; ++step) {
    const int hr = step / per_head, ib = ib_lo + step - hr * per_head;
    const int h = kv * g.R + hr, i0 = ib * ATT_B;
    const int64_t nh = n * g.H + h;
    __syncthreads();   // the previous query block's tiles and operands have been read
    att_load_block<NT>(sQ, base + (int64_t)h * g.d, qpitch, i0, L.q, g.d, g.vec);
    if (tid < ATT_B) sL[tid] = i0 + tid < L.q ? lse[nh * att_Tq(g) + i0 + tid] : 0.f;
    att_load_factor<NT>(sdO, sD, M, Dws, g, L.q, v0, nv, n, h, i0);
    __syncthreads();
    att_f32x4 w;
    const att_f32x4 p = att_p_tile<NT>(sQ, sK, sL, g.scale, dk, lane, ri, cj, mod, att_bias_row(mod, att_Tq(g), h), j0 - i0, w,
                                       [&](int r, int) { return i0 + r >= q_lo && i0 + r <= q_hi; });
#pragma unroll
    for (int e = 0; e < 4; ++e) sP[(16 * ri + 4 * kq + e) * ATT_LDP + 16 * cj + j] = p[e];
#pragma unroll
    for (int vi = 0; vi < C::VC; ++vi)
      if (vi < nv) {
        const att_f32x4 dp = att_tile_nt<NT>(sdO + vi * C::BLK + 16 * ri * C::LD, sV + 16 * cj * C::LD, dk, lane);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 16 * ri + 4 * kq + e;
          sdS[vi * C::TILE + r * ATT_LDP + 16 * cj + j] = w[e] * (dp[e] - sD[vi * ATT_B + r]);
        }
      }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < C::TPW; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
      if (t < 2 * NT && 16 * ct < g.d) {
#pragma unroll
        for (int vi = 0; vi < C::VC; ++vi)
          if (vi < nv) {
            accV[vi][u] = att_acc_tn<NT>(sP, sdO + vi * C::BLK, rt, ct, lane, accV[vi][u]);
            accK[vi][u] = att_acc_tn<NT>(sdS + vi * C::TILE, sQ, rt, ct, lane, accK[vi][u]);
          }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < C::TPW; ++u) {
    const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = 16 * ct + j;
    if (t < 2 * NT && c < g.d) {
#pragma unroll
      for (int vi = 0; vi < C::VC; ++vi)
        if (vi < nv) {
          float *gk = att_gk_rows(g, att_q_rows(g, G, (v0 + vi) * g.N + n), (v0 + vi) * g.N + n) + (int64_t)kv * g.d + c;
          const int kv_to_v = att_k_to_v(g);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = j0 + 16 * rt + 4 * kq + e;
            if (r < att_Tk(g)) {   // (a dead key's row: +0 whatever the sign of the scale)
              gk[(int64_t)r * kpitch] = r < L.k ? g.scale * accK[vi][u][e] : 0.f;
              gk[(int64_t)r * kpitch + kv_to_v] = r < L.k ? accV[vi][u][e] : 0.f;
            }
          }
        }
    }
  }
}

// ---- query-block owner: dQ --------------------------------------------------------------------------------------------------------
template <int NT, class Geo, class Mod>
__global__ __launch_bounds__(256) void attn_dq_kernel(const float *__restrict__ M, const float *__restrict__ qkv,
                                                      const float *__restrict__ lse, const float *__restrict__ Dws, float *__restrict__ G,
                                                      int64_t V, Geo g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  using C = AttCfg<NT>;
  float *sK = att_smem, *sV = sK + C::BLK, *sQ = sV + C::BLK, *sdO = sQ + C::BLK;
  float *sdS = sdO + C::VC * C::BLK + C::TILE, *sL = sdS + C::VC * C::TILE, *sD = sL + ATT_B;   // (the P tile's room is unused here)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t nh = blockIdx.x / att_KBq(g);
  const int ib = (int)(blockIdx.x - nh * att_KBq(g)), i0 = ib * ATT_B;
  const int64_t n = nh / g.H;
  const int h = (int)(nh - n * g.H), dk = (g.d + 3) & ~3;
  const int64_t qpitch = att_qpitch(g), kpitch = att_kpitch(g);
  const int64_t v0 = (int64_t)blockIdx.y * C::VC;
  const int nv = V - v0 < C::VC ? (int)(V - v0) : C::VC;
  const float *base = att_q_rows(g, qkv, n), *kbase = att_k_rows(g, base, n) + (int64_t)(h / g.R) * g.d;
  const AttLive L = att_live(g, n);
  // the key blocks this query block sees (the head of the file); a dead query block (i0 >= L.q) has none, loads nothing and stores
  // its zeros
  const int KBn = (L.k + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int jb_lo = max(ib - wb, 0), jb_hi = i0 < L.q ? (att_causal(g) ? ib : min(ib + wb, KBn - 1)) : -1;
  if (jb_lo <= jb_hi) {
    att_load_block<NT>(sQ, base + (int64_t)h * g.d, qpitch, i0, L.q, g.d, g.vec);
    if (tid < ATT_B) sL[tid] = i0 + tid < L.q ? lse[nh * att_Tq(g) + i0 + tid] : 0.f;
    att_load_factor<NT>(sdO, sD, M, Dws, g, L.q, v0, nv, n, h, i0);
  }
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  const float *brow = att_bias_row(mod, att_Tq(g), h);
  att_f32x4 accQ[C::VC][C::TPW];
#pragma unroll
  for (int vi = 0; vi < C::VC; ++vi)
#pragma unroll
    for (int u = 0; u < C::TPW; ++u) accQ[vi][u] = (att_f32x4){0.f, 0.f, 0.f, 0.f};
  for (int jb = jb_lo; jb <= jb_hi; ++jb) {
    const int j0 = jb * ATT_B;
    __syncthreads();   // the previous key block's tiles and operands have been read
    att_load_block<NT>(sK, kbase, kpitch, j0, L.k, g.d, g.vec);
    att_load_block<NT>(sV, kbase + att_k_to_v(g), kpitch, j0, L.k, g.d, g.vec);
    __syncthreads();
    att_f32x4 w;   // (P alone is not used here)
    att_p_tile<NT>(sQ, sK, sL, g.scale, dk, lane, ri, cj, mod, brow, j0 - i0, w, [&](int r, int c) { return att_valid(g, L, i0 + r, j0 + c); });
#pragma unroll
    for (int vi = 0; vi < C::VC; ++vi)
      if (vi < nv) {
        const att_f32x4 dp = att_tile_nt<NT>(sdO + vi * C::BLK + 16 * ri * C::LD, sV + 16 * cj * C::LD, dk, lane);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 16 * ri + 4 * kq + e;
          sdS[vi * C::TILE + r * ATT_LDP + 16 * cj + j] = w[e] * (dp[e] - sD[vi * ATT_B + r]);
        }
      }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < C::TPW; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
      if (t < 2 * NT && 16 * ct < g.d) {
#pragma unroll
        for (int vi = 0; vi < C::VC; ++vi)
          if (vi < nv) accQ[vi][u] = att_acc_nn<NT>(sdS + vi * C::TILE, sK, rt, ct, lane, accQ[vi][u]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < C::TPW; ++u) {
    const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = 16 * ct + j;
    if (t < 2 * NT && c < g.d) {
#pragma unroll
      for (int vi = 0; vi < C::VC; ++vi)
        if (vi < nv) {
          float *gq = att_q_rows(g, G, (v0 + vi) * g.N + n) + (int64_t)h * g.d + c;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = i0 + 16 * rt + 4 * kq + e;
            if (r < att_Tq(g)) gq[(int64_t)r * qpitch] = r < L.q ? g.scale * accQ[vi][u][e] : 0.f;   // (a dead query's row: +0)
          }
        }
    }
  }
}

// ---- diagonal owner: the factor of the bias table (THE TABLE'S OWN FACTOR at the head of the file) ---------------------------------
// One workgroup owns the block diagonal delta = jb - ib of one (n, h) for VC factor rows: it walks the query blocks ib in ascending
// order with jb = ib + delta and, per tile, recomputes dS = P o (dP - D) of its VC rows as the query owner does (without the cap's
// derivative: the table is added behind the cap).  Thread (vc, rho), rho = -31 .. 31, then adds the diagonal j - i = rho of tile vc,
// i ascending, to ONE register that lives across the walk.  LDS banks of that read (ds_read_b32: bank = word mod 32 within a half
// wave): at step i the thread reads word vc TILE + 36 i + c of row i, c = i + rho its column (clamped to the row where the diagonal
// does not cross it) -- a diagonal steps by 37 words, but that is a stride in time, not across lanes: at one step the lanes of a
// half wave read ONE row each of at most two tiles, lanes with the same column read the same word (a broadcast), and where a half
// straddles two factor rows (63 threads each) the columns of the first tile's lanes all lie above those of the second's, so with
// TILE = 1152 = 0 mod 32 different words never share a bank: no conflict.
template <int NT, class Geo, class Mod>
__global__ __launch_bounds__(256) void attn_dbias_kernel(const float *__restrict__ M, const float *__restrict__ qkv,
                                                         const float *__restrict__ lse, const float *__restrict__ Dws,
                                                         float *__restrict__ partial, int64_t V, Geo g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  using C = AttCfg<NT>;
  float *sK = att_smem, *sV = sK + C::BLK, *sQ = sV + C::BLK, *sdO = sQ + C::BLK;
  float *sdS = sdO + C::VC * C::BLK + C::TILE, *sL = sdS + C::VC * C::TILE, *sD = sL + ATT_B;   // (the P tile's room is unused here)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ND = 2 * g.KB - 1;   // block diagonals -(KB - 1) .. KB - 1
  const int64_t nh = blockIdx.x / ND;
  const int delta = (int)(blockIdx.x - nh * ND) - (g.KB - 1);
  const int64_t n = nh / g.H;
  const int h = (int)(nh - n * g.H), dk = (g.d + 3) & ~3;
  const int64_t v0 = (int64_t)blockIdx.y * C::VC;
  const int nv = V - v0 < C::VC ? (int)(V - v0) : C::VC;
  const float *base = att_q_rows(g, qkv, n), *kbase = att_k_rows(g, base, n) + (int64_t)(h / g.R) * g.d;
  const AttLive L = att_live(g, n);
  // the tiles of this diagonal that the owners' block ranges call non-empty (the head of the file): both blocks live, delta <= 0
  // when causal, |delta| within the window's reach; a diagonal with none loads nothing and stores its zeros
  const int KBn = (L.q + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const bool reached = delta >= -wb && delta <= (att_causal(g) ? 0 : wb);
  const int ib_lo = max(-delta, 0), ib_hi = reached ? KBn - 1 - max(delta, 0) : -1;
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  const float *brow = att_bias_row(mod, att_Tq(g), h);
  const int vc = tid / 63, rho = tid - 63 * vc - 31;   // the thread's diagonal (vc < nv: it has one)
  float acc = 0.f;
  for (int ib = ib_lo; ib <= ib_hi; ++ib) {
    const int i0 = ib * ATT_B, j0 = (ib + delta) * ATT_B;
    __syncthreads();   // the previous tile's dS and operands have been read
    att_load_block<NT>(sQ, base + (int64_t)h * g.d, att_qpitch(g), i0, L.q, g.d, g.vec);
    if (tid < ATT_B) sL[tid] = i0 + tid < L.q ? lse[nh * att_Tq(g) + i0 + tid] : 0.f;
    att_load_factor<NT>(sdO, sD, M, Dws, g, L.q, v0, nv, n, h, i0);
    att_load_block<NT>(sK, kbase, att_kpitch(g), j0, L.k, g.d, g.vec);
    att_load_block<NT>(sV, kbase + att_k_to_v(g), att_kpitch(g), j0, L.k, g.d, g.vec);
    __syncthreads();
    att_f32x4 w;   // (the weight with the cap's derivative is not used here)
    const att_f32x4 p = att_p_tile<NT>(sQ, sK, sL, g.scale, dk, lane, ri, cj, mod, brow, j0 - i0, w,
                                       [&](int r, int c) { return att_valid(g, L, i0 + r, j0 + c); });
#pragma unroll
    for (int vi = 0; vi < C::VC; ++vi)
      if (vi < nv) {
        const att_f32x4 dp = att_tile_nt<NT>(sdO + vi * C::BLK + 16 * ri * C::LD, sV + 16 * cj * C::LD, dk, lane);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 16 * ri + 4 * kq + e;
          sdS[vi * C::TILE + r * ATT_LDP + 16 * cj + j] = p[e] * (dp[e] - sD[vi * ATT_B + r]);
        }
      }
    __syncthreads();
    if (vc < nv) {
      // (all 32 reads are issued before the chain of additions; a row the diagonal does not cross reads a clamped column and
      // adds +0, which changes no sum that started at +0)
      const float *t = sdS + vc * C::TILE;
      float x[ATT_B];
#pragma unroll
      for (int i = 0; i < ATT_B; ++i) x[i] = t[i * ATT_LDP + min(max(i + rho, 0), ATT_B - 1)];
#pragma unroll
      for (int i = 0; i < ATT_B; ++i) acc += (unsigned)(i + rho) < (unsigned)ATT_B ? x[i] : 0.f;
    }
  }
  if (vc < nv) partial[((((v0 + vc) * g.N + n) * g.H + h) * ND + (delta + g.KB - 1)) * 64 + rho + 31] = acc;
}

// the fold: Gb[vnh, b] = the sum over the distances r = -(T - 1) .. T - 1 with index[r + T - 1] == b, r ascending, of the (at most)
// two block diagonals that hold r -- delta = floor(r / 32) at rho = r - 32 delta plus delta + 1 at rho - 32, added to each other
// first -- one chain per element (a term meets at most T - 1 additions on its diagonal, one here and one per distance of the column).  A workgroup owns 256 columns b of one (v, n, h) and passes over the index in pieces of 256 that it keeps in
// LDS with the piece's partial sums (a diagonal that does not exist: +0, which changes no sum).  An index value outside [0, R) is
// equal to no column and is skipped, so no value can carry a store out of bounds; a column nothing maps to is written as +0.
__global__ __launch_bounds__(256) void attn_dbias_fold_kernel(const float *__restrict__ partial, const int32_t *__restrict__ index,
                                                              float *__restrict__ Gb, int64_t VNH, int T, int KB, int64_t R) {
  __shared__ int32_t sI[256];
  __shared__ float sA[256], sB[256];
  const int tid = threadIdx.x, ND = 2 * KB - 1;
  const int64_t RB = (R + 255) / 256, total = VNH * RB, width = 2 * (int64_t)T - 1;
  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    const int64_t vnh = item / RB, b = (item - vnh * RB) * 256 + tid;
    const float *p = partial + vnh * ND * 64;
    float acc = 0.f;
    for (int64_t k0 = 0; k0 < width; k0 += 256) {
      __syncthreads();   // the previous piece has been read
      const int64_t k = k0 + tid;
      int32_t col = -1;
      float a0 = 0.f, a1 = 0.f;
      if (k < width) {
        const int r = (int)(k - (T - 1)), delta = r >> 5, rho = r & 31;   // (floor and remainder, r < 0 included)
        col = index[k];
        if (delta >= -(KB - 1)) a0 = p[(int64_t)(delta + KB - 1) * 64 + rho + 31];
        if (rho >= 1 && delta + 1 <= KB - 1) a1 = p[(int64_t)(delta + KB) * 64 + rho - 1];
      }
      sI[tid] = col, sA[tid] = a0, sB[tid] = a1;
      __syncthreads();
      const int cnt = (int)min((int64_t)256, width - k0);
      if (b < R)
        for (int u = 0; u < cnt; ++u)
          if ((int64_t)sI[u] == b) acc += sA[u] + sB[u];
    }
    if (b < R) Gb[vnh * R + b] = acc;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct AttPlan {
  int status;            // VIVIT_OK, or why nothing is launched
  size_t lse_bytes, bytes;
  int64_t KB;
};

static AttPlan attention_plan(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d) {
  AttPlan p{VIVIT_OK, 0, 0, 0};
  if (V <= 0 || N <= 0 || T <= 0 || H <= 0 || Hkv <= 0 || d <= 0 || H % Hkv != 0) return p.status = VIVIT_E_BADARG, p;
  if (d > ATT_D_MAX) return p.status = VIVIT_E_UNSUPPORTED, p;
  // 32-bit quantities of the kernels: T + 32, the row pitch (H + 2 Hkv) d, the block indices N H KB (lse, dQ) and N Hkv KB (dK and
  // dV; Hkv <= H), the owner's R KB steps (R <= H), the row-dot grid; 64-bit: every element offset
  const int64_t lim = 0x7fffffffLL;
  const int64_t VC = d > 32 ? 2 : 4;
  p.KB = cdiv(T, ATT_B);
  if (T > lim - ATT_B || H + 2 * Hkv > lim / d || N > lim / H || N * H > lim / p.KB || N * Hkv > lim / p.KB || H > lim / p.KB ||
      cdiv(V, VC) > 65535)
    return p.status = VIVIT_E_UNSUPPORTED, p;
  const int64_t per_v = N * H * T;   // (< 2^62: three factors below 2^31 ... checked next with d and V)
  if (per_v > (int64_t)1 << 40 || V > ((int64_t)1 << 58) / (per_v * 3 * d) || cdiv(V * per_v, 256) > lim) return p.status = VIVIT_E_UNSUPPORTED, p;
  p.lse_bytes = align_up((size_t)per_v * 4, 256);
  p.bytes = p.lse_bytes + (size_t)(V * per_v) * 4;
  return p;
}

// the cross-attention entry's plan: that of the query sequence (the workspace is counted in queries) and the limits of the keys'
static AttPlan attention_cross_plan(int64_t V, int64_t N, int64_t Tq, int64_t Tk, int64_t H, int64_t Hkv, int64_t d, int64_t &KBk) {
  if (Tk <= 0) return AttPlan{VIVIT_E_BADARG, 0, 0, 0};
  AttPlan p = attention_plan(V, N, Tq, H, Hkv, d);
  if (p.status != VIVIT_OK) return p;
  // 32-bit: Tk + 32, the block index N Hkv KBk of the key owner (its R KBq steps, the pitches H d and 2 Hkv d < (H + 2 Hkv) d and
  // the blocks N H KBq of the query owners are the plan's); 64-bit: every element offset of kv and Gkv
  const int64_t lim = 0x7fffffffLL;
  KBk = cdiv(Tk, ATT_B);
  const int64_t per_k = N * Hkv * Tk;   // (N Hkv < 2^31 by the plan)
  if (Tk > lim - ATT_B || N * Hkv > lim / KBk || per_k > (int64_t)1 << 40 || V > ((int64_t)1 << 58) / (per_k * 2 * d))
    return AttPlan{VIVIT_E_UNSUPPORTED, 0, 0, 0};
  return p;
}

// the four launches; `G`: the result of the query owner (null: not launched), `Gkv`: that of the key owner (null: not launched; for
// self-attention the same packed tensor as G)
template <int NT, class Geo, class Mod>
static int attention_launch(const float *M, const float *qkv, const float *out, float *G, float *Gkv, float *lse, float *Dws,
                            int64_t V, const Geo &g, const Mod &mod, int T, int KBq, int KBk, hipStream_t s) {
  using C = AttCfg<NT>;
  static unsigned long long attr_done = 0;
  constexpr int lse_lds = C::LSE_FLOATS * 4, own_lds = C::OWN_FLOATS * 4;
  if (own_lds > 64 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
    if (!ensure_dynamic_lds(reinterpret_cast<const void *>(attn_dkv_kernel<NT, Geo, Mod>), own_lds, attr_done) ||
        !ensure_dynamic_lds(reinterpret_cast<const void *>(attn_dq_kernel<NT, Geo, Mod>), own_lds, attr_done))
      return VIVIT_E_LAUNCH;
    attr_done |= 1ull << (dev & 63);
  }
  const int64_t NH = (int64_t)g.N * g.H, total = V * NH * T;
  const unsigned blocks = (unsigned)(NH * KBq), kv_blocks = (unsigned)((int64_t)g.N * g.Hkv * KBk);
  attn_lse_kernel<NT, Geo, Mod><<<blocks, 256, lse_lds, s>>>(qkv, lse, g, mod);
  attn_rowdot_kernel<Geo><<<(unsigned)cdiv(total, 256), 256, 0, s>>>(M, out, Dws, total, g);
  const unsigned chunks = (unsigned)cdiv(V, C::VC);
  if (Gkv) attn_dkv_kernel<NT, Geo, Mod><<<dim3(kv_blocks, chunks), 256, own_lds, s>>>(M, qkv, lse, Dws, G, V, g, mod);
  if (G) attn_dq_kernel<NT, Geo, Mod><<<dim3(blocks, chunks), 256, own_lds, s>>>(M, qkv, lse, Dws, G, V, g, mod);
  return launch_status();
}

template <class Geo, class Mod>
static int attention_launch_d(const float *M, const float *qkv, const float *out, float *G, float *Gkv, float *lse, float *Dws,
                              int64_t V, const Geo &g, const Mod &mod, int T, int KBq, int KBk, hipStream_t s) {
  if (g.d <= 16) return attention_launch<1>(M, qkv, out, G, Gkv, lse, Dws, V, g, mod, T, KBq, KBk, s);
  if (g.d <= 32) return attention_launch<2>(M, qkv, out, G, Gkv, lse, Dws, V, g, mod, T, KBq, KBk, s);
  if (g.d <= 64) return attention_launch<4>(M, qkv, out, G, Gkv, lse, Dws, V, g, mod, T, KBq, KBk, s);
  return attention_launch<8>(M, qkv, out, G, Gkv, lse, Dws, V, g, mod, T, KBq, KBk, s);
}

static inline bool att_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the geometry of a self-attention call that the plan has accepted
static AttGeom attention_self_geom(const float *M, const float *qkv, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d, int64_t KB,
                                   float scale, int causal, const int32_t *lengths, int64_t window) {
  AttGeom g;
  g.N = (int)N, g.T = (int)T, g.H = (int)H, g.d = (int)d, g.KB = (int)KB;
  g.Hkv = (int)Hkv, g.R = (int)(H / Hkv);
  g.pitch = (int)((H + 2 * Hkv) * d), g.koff = (int)(H * d), g.voff = (int)((H + Hkv) * d);
  g.causal = causal != 0;
  g.vec = (d & 3) == 0 && att_aligned16(M) && att_aligned16(qkv);
  g.scale = scale;
  g.lengths = lengths;
  g.window = window >= T ? 0 : (int)window;   // (a window of T or more cuts nothing; this also covers every value beyond an int)
  return g;
}

// the self-attention entries: every refusal, then the four launches with the score function `mod`
template <class Mod>
static int attention_self(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T, int64_t H,
                          int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths, int64_t window, const Mod &mod,
                          void *workspace, size_t workspace_bytes, void *stream) {
  if (!M || !qkv || !out || !G || window < 0) return VIVIT_E_BADARG;
  const AttPlan p = attention_plan(V, N, T, H, Hkv, d);
  if (p.status != VIVIT_OK) return p.status;
  if (!workspace || workspace_bytes < p.bytes) return VIVIT_E_WORKSPACE;
  const AttGeom g = attention_self_geom(M, qkv, N, T, H, Hkv, d, p.KB, scale, causal, lengths, window);
  float *lse = static_cast<float *>(workspace);
  float *Dws = reinterpret_cast<float *>(static_cast<char *>(workspace) + p.lse_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return attention_launch_d(M, qkv, out, G, G, lse, Dws, V, g, mod, g.T, g.KB, g.KB, s);
}

// ---- the table's own factor ---------------------------------------------------------------------------------------------------------
// the plan of the scoremod entry and, behind its workspace, the partial sums [V, N, H, 2 KB - 1, 64] of the diagonal owner
static AttPlan attention_bias_plan(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d, size_t &partial_off) {
  AttPlan p = attention_plan(V, N, T, H, Hkv, d);
  if (p.status != VIVIT_OK) return p;
  // 32-bit: the diagonal owner's block index N H (2 KB - 1) (N H KB is the plan's); 64-bit: every element offset (V <= 4 * 65535 by
  // the plan's chunk limit, so V N H (2 KB - 1) 256 < 2^58)
  if (N * H > 0x7fffffffLL / (2 * p.KB - 1)) return p.status = VIVIT_E_UNSUPPORTED, p;
  partial_off = p.bytes;
  p.bytes += (size_t)(V * N * H) * (size_t)(2 * p.KB - 1) * 64 * 4;
  return p;
}

template <int NT>
static int attention_bias_launch(const float *M, const float *qkv, const float *out, float *Gb, float *lse, float *Dws, float *partial,
                                 int64_t V, const AttGeom &g, const AttScoreMod &mod, const int32_t *index, int64_t R, hipStream_t s) {
  using C = AttCfg<NT>;
  static unsigned long long attr_done = 0;
  constexpr int lse_lds = C::LSE_FLOATS * 4, own_lds = C::OWN_FLOATS * 4;
  if (own_lds > 64 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
    if (!ensure_dynamic_lds(reinterpret_cast<const void *>(attn_dbias_kernel<NT, AttGeom, AttScoreMod>), own_lds, attr_done))
      return VIVIT_E_LAUNCH;
    attr_done |= 1ull << (dev & 63);
  }
  const int64_t NH = (int64_t)g.N * g.H, total = V * NH * g.T, ND = 2 * (int64_t)g.KB - 1;
  attn_lse_kernel<NT, AttGeom, AttScoreMod><<<(unsigned)(NH * g.KB), 256, lse_lds, s>>>(qkv, lse, g, mod);
  attn_rowdot_kernel<AttGeom><<<(unsigned)cdiv(total, 256), 256, 0, s>>>(M, out, Dws, total, g);
  attn_dbias_kernel<NT, AttGeom, AttScoreMod><<<dim3((unsigned)(NH * ND), (unsigned)cdiv(V, C::VC)), 256, own_lds, s>>>(M, qkv, lse, Dws, partial,
                                                                                                                    V, g, mod);
  const int64_t items = V * NH * cdiv(R, 256);
  attn_dbias_fold_kernel<<<(unsigned)(items < 0x7fffffffLL ? items : 0x7fffffffLL), 256, 0, s>>>(partial, index, Gb, V * NH, g.T, g.KB, R);
  return launch_status();
}

} // namespace vivit

using namespace vivit;

extern "C" {

size_t vivit_attention_masked_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d) {
  const AttPlan p = attention_plan(V, N, T, H, Hkv, d);
  return p.status == VIVIT_OK ? p.bytes : 0;
}

// lengths [N] int32 on the device or null; window >= 1 or 0 (none): the one entry that launches, the others below call it
int vivit_attention_masked_jac_t_f32(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T,
                                     int64_t H, int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths,
                                     int64_t window, void *workspace, size_t workspace_bytes, void *stream) {
  return attention_self(M, qkv, out, G, V, N, T, H, Hkv, d, scale, causal, lengths, window, AttPlain{}, workspace, workspace_bytes, stream);
}

// the score modifiers (the head of the file): softcap > 0 or 0 (none), bias [H, 2 T - 1] on the device or null (none); with neither
// the masked entry, its plain instances and its bytes
size_t vivit_attention_scoremod_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d) {
  return vivit_attention_masked_jac_t_f32_workspace_bytes(V, N, T, H, Hkv, d);
}

int vivit_attention_scoremod_jac_t_f32(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T,
                                       int64_t H, int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths,
                                       int64_t window, float softcap, const float *bias, void *workspace, size_t workspace_bytes,
                                       void *stream) {
  if (!(softcap >= 0.f) || isinf(softcap)) return VIVIT_E_BADARG;   // (negative, NaN, inf)
  if (softcap == 0.f && !bias)
    return vivit_attention_masked_jac_t_f32(M, qkv, out, G, V, N, T, H, Hkv, d, scale, causal, lengths, window, workspace, workspace_bytes,
                                            stream);
  return attention_self(M, qkv, out, G, V, N, T, H, Hkv, d, scale, causal, lengths, window, AttScoreMod{softcap, bias}, workspace,
                        workspace_bytes, stream);
}

// the factor of the bias table (the head of the file): bias [H, 2 T - 1] and index [2 T - 1] on the device, neither null; Gb [V, N, H, R]
size_t vivit_attention_bias_factor_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d) {
  size_t off = 0;
  const AttPlan p = attention_bias_plan(V, N, T, H, Hkv, d, off);
  return p.status == VIVIT_OK ? p.bytes : 0;
}

int vivit_attention_bias_factor_f32(const float *M, const float *qkv, const float *out, float *Gb, int64_t V, int64_t N, int64_t T,
                                    int64_t H, int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths, int64_t window,
                                    float softcap, const float *bias, const int32_t *index, int64_t R, void *workspace,
                                    size_t workspace_bytes, void *stream) {
  if (!(softcap >= 0.f) || isinf(softcap)) return VIVIT_E_BADARG;   // (negative, NaN, inf)
  if (!M || !qkv || !out || !Gb || !bias || !index || R < 1 || window < 0) return VIVIT_E_BADARG;
  size_t off = 0;
  const AttPlan p = attention_bias_plan(V, N, T, H, Hkv, d, off);
  if (p.status != VIVIT_OK) return p.status;
  if (!workspace || workspace_bytes < p.bytes) return VIVIT_E_WORKSPACE;
  const AttGeom g = attention_self_geom(M, qkv, N, T, H, Hkv, d, p.KB, scale, causal, lengths, window);
  const AttScoreMod mod{softcap, bias};
  char *ws = static_cast<char *>(workspace);
  float *lse = reinterpret_cast<float *>(ws), *Dws = reinterpret_cast<float *>(ws + p.lse_bytes), *partial = reinterpret_cast<float *>(ws + off);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d <= 16) return attention_bias_launch<1>(M, qkv, out, Gb, lse, Dws, partial, V, g, mod, index, R, s);
  if (d <= 32) return attention_bias_launch<2>(M, qkv, out, Gb, lse, Dws, partial, V, g, mod, index, R, s);
  if (d <= 64) return attention_bias_launch<4>(M, qkv, out, Gb, lse, Dws, partial, V, g, mod, index, R, s);
  return attention_bias_launch<8>(M, qkv, out, Gb, lse, Dws, partial, V, g, mod, index, R, s);
}

// cross-attention (the head of the file): q_lengths, k_lengths [N] int32 on the device or null; Gq or Gkv may be null, not both
size_t vivit_attention_cross_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t Tq, int64_t Tk, int64_t H, int64_t Hkv,
                                                       int64_t d) {
  int64_t KBk = 0;
  const AttPlan p = attention_cross_plan(V, N, Tq, Tk, H, Hkv, d, KBk);
  return p.status == VIVIT_OK ? p.bytes : 0;
}

int vivit_attention_cross_jac_t_f32(const float *M, const float *q, const float *kv, const float *out, float *Gq, float *Gkv, int64_t V,
                                    int64_t N, int64_t Tq, int64_t Tk, int64_t H, int64_t Hkv, int64_t d, float scale,
                                    const int32_t *q_lengths, const int32_t *k_lengths, void *workspace, size_t workspace_bytes,
                                    void *stream) {
  if (!M || !q || !kv || !out || (!Gq && !Gkv)) return VIVIT_E_BADARG;
  int64_t KBk = 0;
  const AttPlan p = attention_cross_plan(V, N, Tq, Tk, H, Hkv, d, KBk);
  if (p.status != VIVIT_OK) return p.status;
  if (!workspace || workspace_bytes < p.bytes) return VIVIT_E_WORKSPACE;
  AttGeomX g;
  g.N = (int)N, g.Tq = (int)Tq, g.Tk = (int)Tk, g.H = (int)H, g.d = (int)d, g.KBq = (int)p.KB, g.KBk = (int)KBk;
  g.Hkv = (int)Hkv, g.R = (int)(H / Hkv);
  g.qpitch = (int)(H * d), g.kpitch = (int)(2 * Hkv * d), g.voff = (int)(Hkv * d);
  g.vec = (d & 3) == 0 && att_aligned16(M) && att_aligned16(q) && att_aligned16(kv);
  g.scale = scale;
  g.kv = kv, g.Gkv = Gkv;
  g.qlengths = q_lengths, g.klengths = k_lengths;
  float *lse = static_cast<float *>(workspace);
  float *Dws = reinterpret_cast<float *>(static_cast<char *>(workspace) + p.lse_bytes);
  return attention_launch_d(M, q, out, Gq, Gkv, lse, Dws, V, g, AttPlain{}, g.Tq, g.KBq, g.KBk, static_cast<hipStream_t>(stream));
}

// grouped-query attention without lengths or a window
size_t vivit_attention_gqa_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d) {
  return vivit_attention_masked_jac_t_f32_workspace_bytes(V, N, T, H, Hkv, d);
}

int vivit_attention_gqa_jac_t_f32(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T,
                                  int64_t H, int64_t Hkv, int64_t d, float scale, int causal, void *workspace, size_t workspace_bytes,
                                  void *stream) {
  return vivit_attention_masked_jac_t_f32(M, qkv, out, G, V, N, T, H, Hkv, d, scale, causal, nullptr, 0, workspace, workspace_bytes,
                                          stream);
}

// multi-head attention: every query head has its own key and value head
size_t vivit_attention_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t d) {
  return vivit_attention_masked_jac_t_f32_workspace_bytes(V, N, T, H, H, d);
}

int vivit_attention_jac_t_f32(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T, int64_t H,
                              int64_t d, float scale, int causal, void *workspace, size_t workspace_bytes, void *stream) {
  return vivit_attention_masked_jac_t_f32(M, qkv, out, G, V, N, T, H, H, d, scale, causal, nullptr, 0, workspace, workspace_bytes,
                                          stream);
}

} // extern "C"
