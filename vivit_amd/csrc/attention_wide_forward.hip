// Scaled dot-product self-attention, the FORWARD pass for head dimensions 129 .. 256 (vivit_attention_wide_forward_f32): the
// function, the contract and the online softmax of attention_forward.hip (its head; nothing is restated here) with the work split
// of attention_wide.hip -- the resident operand at full width, the visiting ones in column halves of 128.  One launch:
//   attn_wide_fwd_kernel   the QUERY-block owner of one (n, h, block of 32 queries), the grid, the block range jb_lo .. jb_hi and the
//                          dead-block exit of attn_fwd_kernel.  Q of its queries stays in LDS at full width (pitch 260); two HALF
//                          SLOTS of pitch 132 take, per key block, first the two halves of K and then the two halves of V:
//                            1. K half 0 and half 1 into the slots (rows beyond the live keys and the columns >= d of half 1: zeros,
//                               never read from memory),
//                            2. the wave's 16 x 16 S tile in registers, its two chains carried across the halves
//                               (att_wide_tile_nt): every logit has the bits of att_tile_nt<16>, the very s the wide rule's lse
//                               launch sums and attention_wide_backward.hip recomputes; the logit of every visible pair and -inf
//                               for the others into the LDS tile sP [32][36],
//                            3. V half 0 and half 1 into the same slots (K has been read: one barrier serves the tile and the
//                               slots), and under those loads the online softmax of attn_fwd_kernel unchanged: eight lanes per
//                               row, (m, l) in their registers, p back into sP, alpha into sR,
//                            4. O = alpha O + P V_c per half c: the output block [32][256] is 32 tiles of 16 x 16, eight per wave
//                               ([half][tile]), in MFMA accumulators across the whole walk (att_acc_nn on a half slot).
//                          After the walk O / l for the columns < d of the live rows, and lse = m + log l.
// Four barriers per key block.  LDS: 33 280 (Q) + 2 x 16 896 (the slots) + 4 608 (the tile) + 128 (the row factors) = 71 808 bytes:
// two workgroups share a CU's 160 KB, so one's loads run under the other's products, the reasoning of attention_forward.hip.  K and
// V at full width instead (no halves, one barrier fewer) come to 104 KB and one workgroup per CU; that variant was not built and not
// measured.
// SUMMATION ORDER of an output element: key blocks ascending, inside a block k ascending in steps of four; the halves split columns
// of O, never a sum.  l: as attn_fwd_kernel.  No atomics, no workspace; the bytes of out[n] and lse[n] depend on the shape
// parameters, the cap, the table, the length of n and the data of sample n only, and out[n, :Tn] has the bytes of the sample cut to
// Tn and run alone.  DEAD POSITIONS: no operand row of one is loaded; rows of dead queries are +0 in out and in lse.
#include "attention_wide_common.h"

namespace vivit {

constexpr int ATT_WIDE_FWD_FLOATS = AttWF::BLK + 2 * AttWH::BLK + AttWF::TILE + ATT_B;   // Q; the half slots; the tile S -> P; alpha, then l
static_assert(ATT_WIDE_FWD_FLOATS * 4 == 71808 && 2 * ATT_WIDE_FWD_FLOATS * 4 <= 160 * 1024, "two workgroups share a CU's LDS");
static_assert(AttWH::DP == ATT_WIDE_HALF && AttWH::TPW == 4, "a half is eight column tiles: four 16 x 16 tiles per wave");

template <class Mod>
__global__ __launch_bounds__(256) void attn_wide_fwd_kernel(const float *__restrict__ qkv, float *__restrict__ out, float *__restrict__ lse,
                                                            AttGeom g, Mod mod) {
  extern __shared__ __attribute__((aligned(16))) float att_smem[];
  constexpr int FL = AttWF::LD, HL = AttWH::LD, HBLK = AttWH::BLK;
  float *sQ = att_smem, *sH = sQ + AttWF::BLK, *sP = sH + 2 * HBLK, *sR = sP + AttWF::TILE;   // sH: the two half slots
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t nh = blockIdx.x / g.KB;
  const int ib = (int)(blockIdx.x - nh * g.KB), i0 = ib * ATT_B;
  const int64_t n = nh / g.H;
  const int h = (int)(nh - n * g.H), dk = (g.d + 3) & ~3, T = g.T;
  const int64_t E = (int64_t)g.H * g.d, pitch = g.pitch;
  const AttLive L = att_live(g, n);
  float *orow = out + (n * T + i0) * E + (int64_t)h * g.d;   // row 0 of the block, column 0 of the head
  float *lrow = lse ? lse + nh * T + i0 : nullptr;
  if (i0 >= L.q) {   // a block with no live query: nothing is loaded, its rows are +0
    for (int idx = tid; idx < ATT_B * g.d; idx += 256) {
      const int r = idx / g.d, c = idx - r * g.d;
      if (i0 + r < T) orow[(int64_t)r * E + c] = 0.f;
    }
    if (lrow && tid < ATT_B && i0 + tid < T) lrow[tid] = 0.f;
    return;
  }
  const float *base = att_q_rows(g, qkv, n), *kbase = base + g.koff + (int64_t)(h / g.R) * g.d, *vbase = kbase + att_k_to_v(g);
  att_load_block<16>(sQ, base + (int64_t)h * g.d, pitch, i0, L.q, g.d, g.vec);
  const int ri = wave >> 1, cj = wave & 1, j = lane & 15, kq = lane >> 4;
  const int row = tid >> 3, sub = tid & 7;
  float m = -INFINITY, l = 0.f;
  const att_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  att_f32x4 acc[2][4];   // [half][tile of the wave]
#pragma unroll
  for (int hp = 0; hp < 2; ++hp)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[hp][u] = zero;
  const float *brow = att_bias_row(mod, T, h);
  const int KBn = (L.k + ATT_B - 1) / ATT_B, wb = att_reach(g, KBn);
  const int jb_lo = max(ib - wb, 0), jb_hi = att_causal(g) ? ib : min(ib + wb, KBn - 1);
  for (int jb = jb_lo; jb <= jb_hi; ++jb) {
    const int j0 = jb * ATT_B;
    __syncthreads();   // the previous key block's reads of the slots (V), sP and sR are done
#pragma unroll
    for (int half = 0; half < 2; ++half) att_wide_load_half(sH + half * HBLK, kbase, pitch, j0, L.k, g.d, g.vec, half);
    __syncthreads();
    att_f32x4 s0 = zero, s1 = zero;
    att_wide_tile_nt<FL, HL>(sQ + 16 * ri * FL, sH + 16 * cj * HL, ATT_WIDE_HALF, lane, s0, s1);
    att_wide_tile_nt<FL, HL>(sQ + 16 * ri * FL + ATT_WIDE_HALF, sH + HBLK + 16 * cj * HL, dk - ATT_WIDE_HALF, lane, s0, s1);
    const att_f32x4 s = s0 + s1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 16 * ri + 4 * kq + e, c = 16 * cj + j;
      float keep;
      sP[r * ATT_LDP + c] = att_valid(g, L, i0 + r, j0 + c) ? att_logit(mod, s[e], g.scale, brow, j0 - i0 + c - r, keep) : -INFINITY;
    }
    __syncthreads();   // the tile is written, K has been read
#pragma unroll
    for (int half = 0; half < 2; ++half) att_wide_load_half(sH + half * HBLK, vbase, pitch, j0, L.k, g.d, g.vec, half);
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
    for (int hp = 0; hp < 2; ++hp)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = wave + 4 * u, rt = t & 1, ct = t >> 1;
        if (ATT_WIDE_HALF * hp + 16 * ct < g.d) {
          const att_f32x4 a = *reinterpret_cast<const att_f32x4 *>(sR + 16 * rt + 4 * kq);
          acc[hp][u] = att_acc_nn<8>(sP, sH + hp * HBLK, rt, ct, lane, acc[hp][u] * a);
        }
      }
  }
  __syncthreads();   // the last key block's reads of sR are done
  if (sub == 0) {
    sR[row] = l;
    if (lrow && i0 + row < T) lrow[row] = i0 + row < L.q ? m + logf(l) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int hp = 0; hp < 2; ++hp)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = wave + 4 * u, rt = t & 1, ct = t >> 1, c = ATT_WIDE_HALF * hp + 16 * ct + j;
      if (c < g.d) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 16 * rt + 4 * kq + e;
          if (i0 + r < T) orow[(int64_t)r * E + c] = i0 + r < L.q ? acc[hp][u][e] / sR[r] : 0.f;   // (a dead query's row: +0)
        }
      }
    }
}

template <class Mod>
static int attention_wide_forward_launch(const float *qkv, float *out, float *lse, const AttGeom &g, const Mod &mod, hipStream_t s) {
  static unsigned long long attr_done = 0;
  constexpr int lds = ATT_WIDE_FWD_FLOATS * 4;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
  if (!ensure_dynamic_lds(reinterpret_cast<const void *>(attn_wide_fwd_kernel<Mod>), lds, attr_done)) return VIVIT_E_LAUNCH;
  attr_done |= 1ull << (dev & 63);
  attn_wide_fwd_kernel<Mod><<<(unsigned)((int64_t)g.N * g.H * g.KB), 256, lds, s>>>(qkv, out, lse, g, mod);
  return launch_status();
}

} // namespace vivit

using namespace vivit;

extern "C" {

// the arguments and the refusals of vivit_attention_forward_f32, in its order, for 128 < d <= 256
int vivit_attention_wide_forward_f32(const float *qkv, float *out, float *lse, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d,
                                     float scale, int causal, const int32_t *lengths, int64_t window, float softcap, const float *bias,
                                     void *stream) {
  if (!(softcap >= 0.f) || isinf(softcap)) return VIVIT_E_BADARG;   // (negative, NaN, inf)
  if (!qkv || !out || window < 0) return VIVIT_E_BADARG;
  const AttPlan p = attention_wide_plan(1, N, T, H, Hkv, d);
  if (p.status != VIVIT_OK) return p.status;
  const AttGeom g = attention_self_geom(qkv, qkv, N, T, H, Hkv, d, p.KB, scale, causal, lengths, window);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (softcap == 0.f && !bias) return attention_wide_forward_launch(qkv, out, lse, g, AttPlain{}, s);
  return attention_wide_forward_launch(qkv, out, lse, g, AttScoreMod{softcap, bias}, s);
}

} // extern "C"
