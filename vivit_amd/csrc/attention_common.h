// What the attention translation units share (attention.hip: head dimensions up to 128; attention_wide.hip: 129 to 256;
// attention_forward.hip: the forward pass, up to 128; attention_backward.hip: its gradient from the saved lse, up to 128;
// attention_wide_forward.hip and attention_wide_backward.hip: the same two for 129 to 256, through attention_wide_common.h): the tile
// configuration, the LDS block loader and the MFMA tile products, the two geometries with their mask and block-range helpers, the
// score function, the row log-sum-exp and row-dot kernels, and the host plan.  The contract they serve stands at the head of
// attention.hip.
#pragma once
#include <math.h>

#include "common.h"

namespace vivit {

constexpr int ATT_B = 32;          // queries per query block = keys per key block
constexpr int ATT_LDP = 36;        // row pitch of the 32 x 32 tiles P and dS
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

// blocks a window reaches to either side of the diagonal (the head of attention.hip); KBn where there is no window
__device__ __forceinline__ int att_reach(const AttGeom &g, int KBn) { return g.window > 0 ? (g.window + 30) >> 5 : KBn; }

struct AttLive { int q, k; };   // live queries and live keys of a sample (self-attention: the same number): rows beyond are never loaded

__device__ __forceinline__ bool att_valid(const AttGeom &g, AttLive L, int gi, int gj) {
  const int dist = gi - gj, Tn = L.q;
  return gi < Tn && gj < Tn && (!g.causal || dist >= 0) && (g.window <= 0 || (dist < g.window && -dist < g.window));
}

// cross-attention (the head of attention.hip): the kernels' first pointer is q, their result Gq; the second sequence travels here
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
// the block ranges of the walks (BLOCK RANGES at the head of attention.hip) are written once, in the kernels, from att_reach and
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

// ---- the score function (SCORE MODIFIERS at the head of attention.hip) -------------------------------------------------------------------
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

// one wave's 16 x 16 part of P = exp(S - lse) for the tile (query block at i0, key block at j0), from its part `s` of the products
// q_i k_j; zero where masked or beyond Tn (`visible(r, c)`: att_valid of the pair at row r and column c of the tile, in whatever
// form the owner keeps it).  `w`: the weight of (dP - D) in dZ, P itself without a cap; `brow`, `dj0 = j0 - i0`: the head's table
// row and the tile's distance for att_logit; sL: lse of the block's 32 queries
template <class Mod, class Visible>
__device__ __forceinline__ att_f32x4 att_p_of(const att_f32x4 &s, const float *__restrict__ sL, float scale, int lane, int ri, int cj,
                                              const Mod &mod, const float *__restrict__ brow, int dj0, att_f32x4 &w, Visible visible) {
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
// the same with the product: sQ, sK the [32][LD] blocks of the queries and the keys (the owners of attention.hip)
template <int NT, class Mod, class Visible>
__device__ __forceinline__ att_f32x4 att_p_tile(const float *__restrict__ sQ, const float *__restrict__ sK, const float *__restrict__ sL,
                                                float scale, int dk, int lane, int ri, int cj, const Mod &mod,
                                                const float *__restrict__ brow, int dj0, att_f32x4 &w, Visible visible) {
  using C = AttCfg<NT>;
  const att_f32x4 s = att_tile_nt<NT>(sQ + 16 * ri * C::LD, sK + 16 * cj * C::LD, dk, lane);
  return att_p_of(s, sL, scale, lane, ri, cj, mod, brow, dj0, w, visible);
}

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
// Acc: the type of the chain, rounded to float once at the end (float: the chain of the narrow units; double: attention_wide.hip)
template <class Geo, class Acc = float>
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
  Acc a = 0;
  for (int c = 0; c < g.d; ++c) a = fma((Acc)m[c], (Acc)o[c], a);
  D[e] = (float)a;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct AttPlan {
  int status;            // VIVIT_OK, or why nothing is launched
  size_t lse_bytes, bytes;
  int64_t KB;
};

// (d_max: the widest head of the calling unit's kernels)
static AttPlan attention_plan(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d, int64_t d_max) {
  AttPlan p{VIVIT_OK, 0, 0, 0};
  if (V <= 0 || N <= 0 || T <= 0 || H <= 0 || Hkv <= 0 || d <= 0 || H % Hkv != 0) return p.status = VIVIT_E_BADARG, p;
  if (d > d_max) return p.status = VIVIT_E_UNSUPPORTED, p;
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

constexpr int ATT_D_MAX = 128;   // the head dimensions of attention.hip and attention_forward.hip (129 to 256: attention_wide.hip)

// the cross-attention entries' plan: that of the query sequence (the workspace is counted in queries) and the limits of the keys'
static AttPlan attention_cross_plan(int64_t V, int64_t N, int64_t Tq, int64_t Tk, int64_t H, int64_t Hkv, int64_t d, int64_t &KBk) {
  if (Tk <= 0) return AttPlan{VIVIT_E_BADARG, 0, 0, 0};
  AttPlan p = attention_plan(V, N, Tq, H, Hkv, d, ATT_D_MAX);
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

// the geometry of a cross-attention call that the plan has accepted (M: the factor, or q again where there is none)
static AttGeomX attention_cross_geom(const float *M, const float *q, const float *kv, float *Gkv, int64_t N, int64_t Tq, int64_t Tk,
                                     int64_t H, int64_t Hkv, int64_t d, int64_t KBq, int64_t KBk, float scale,
                                     const int32_t *q_lengths, const int32_t *k_lengths) {
  AttGeomX g;
  g.N = (int)N, g.Tq = (int)Tq, g.Tk = (int)Tk, g.H = (int)H, g.d = (int)d, g.KBq = (int)KBq, g.KBk = (int)KBk;
  g.Hkv = (int)Hkv, g.R = (int)(H / Hkv);
  g.qpitch = (int)(H * d), g.kpitch = (int)(2 * Hkv * d), g.voff = (int)(Hkv * d);
  g.vec = (d & 3) == 0 && att_aligned16(M) && att_aligned16(q) && att_aligned16(kv);
  g.scale = scale;
  g.kv = kv, g.Gkv = Gkv;
  g.qlengths = q_lengths, g.klengths = k_lengths;
  return g;
}

} // namespace vivit
