// The general fp32 GEMM / SYRK tile of the library (route Tile128: every shape and layout; batched mode; the lower-triangle
// update of the band reduction).
//
//   C[M,N] = alpha * op(A) op(B)^T + beta * C,   exact fp32 (v_mfma_f32_32x32x2_f32 is a
//   k-ordered fmaf chain), accumulators flushed into a second accumulator every 2048 k so that
//   long contractions (P up to ~4e5 for the Gram build) keep pairwise-like rounding error.
//
// Tile: 128x128x16 per 256-thread workgroup; 4 waves in a 2x2 grid, each wave owns a 64x64
// block = 2x2 MFMA 32x32 tiles (64 accumulator VGPRs + 64 for the second level).  Operands are
// register-staged into double-buffered LDS (one barrier per K tile).  fp32 MFMA runs at the
// vector rate (64 flop/clk/SIMD), so one wave spends 2048 cycles of matrix work per K tile and
// the 4 global float4 loads + 8 ds_read_b128 per wave per K tile hide completely behind it.
//
// blockIdx -> tile mapping is XCD-aware: the grid is cut into 16x16-tile super-blocks; inside a
// super-block the 8 workgroups that share an XCD (blockIdx % 8, round-robin dispatch) own one
// compact 8x4-tile sub-block, so the A/B row panels they stream are shared through that XCD's
// L2 (speed only, never correctness).
//
// SYRK mode (the Gram build, K1): B == A, only super-blocks/tiles with tile_i >= tile_j are
// computed (n(n+1)p flops instead of 2n^2p) and off-diagonal tiles are stored twice, the mirror
// image transposed through LDS so that both stores are coalesced.
#include "gemm_plan.h"

namespace vivit {

constexpr int FLUSH_TILES = 2048 / BK;         // second-level accumulation period

// Global -> registers for one ROWS x 16 operand tile (ROWS / 64 float4 per thread).  MODE:
//   0  tile completely in range, operand 16-byte aligned: unconditional float4
//   1  aligned operand, ragged rows (and, for LAY_M, row count % 4 == 0): float4 from a clamped
//      row + zero select -- still one vector load per thread and no branch
//   2  anything else: clamped scalar loads
// Full K tiles only for modes 0/1 (a ragged last K tile is loaded with mode 2).
template <int LAY, int MODE, int ROWS>
__device__ __forceinline__ void tile_load(gcptr P, int64_t ld, int64_t row0, int64_t nrows, int64_t k0,
                                          int64_t kend, int tid, float4 (&st)[ROWS / 64]) {
#pragma unroll
  for (int q = 0; q < ROWS / 64; ++q) {
    const int f = tid + 256 * q;
    if (LAY == LAY_K) {
      const int64_t row = row0 + (f >> 2), k = k0 + 4 * (f & 3);
      if constexpr (MODE == 0) {
        st[q] = ldg4(P + row * ld + k);
      } else if constexpr (MODE == 1) {
        const bool ok = row < nrows;
        const float4 v = ldg4(P + (ok ? row : nrows - 1) * ld + k);
        st[q] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        st[q] = make_float4(ld1_sel(P, row, nrows, k, kend, ld), ld1_sel(P, row, nrows, k + 1, kend, ld),
                            ld1_sel(P, row, nrows, k + 2, kend, ld), ld1_sel(P, row, nrows, k + 3, kend, ld));
      }
    } else {
      const int64_t row = row0 + 4 * (f & (ROWS / 4 - 1)), k = k0 + f / (ROWS / 4);
      if constexpr (MODE == 0) {
        st[q] = ldg4(P + k * ld + row);
      } else if constexpr (MODE == 1) {
        const bool ok = row < nrows;  // nrows % 4 == 0: the whole float4 is in or out
        const float4 v = ldg4(P + k * ld + (ok ? row : 0));
        st[q] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        st[q] = make_float4(ld1_sel(P, k, kend, row, nrows, ld), ld1_sel(P, k, kend, row + 1, nrows, ld),
                            ld1_sel(P, k, kend, row + 2, nrows, ld), ld1_sel(P, k, kend, row + 3, nrows, ld));
      }
    }
  }
}

// Registers -> LDS.
template <int LAY, int ROWS>
__device__ __forceinline__ void tile_store(float *__restrict__ s, int tid, const float4 (&st)[ROWS / 64]) {
#pragma unroll
  for (int q = 0; q < ROWS / 64; ++q) {
    const int f = tid + 256 * q;
    if (LAY == LAY_K) {
      *reinterpret_cast<float4 *>(s + (f >> 2) * SK + 4 * (f & 3)) = st[q];
    } else {
      *reinterpret_cast<float4 *>(s + (f / (ROWS / 4)) * (ROWS + 4) + 4 * (f & (ROWS / 4 - 1))) = st[q];
    }
  }
}

// MFMA operand fragments for the 8 k-pairs of one K tile.  MFMA u = 4q + t (q in 0..1,
// t in 0..3) consumes k = 8q + 4h + t from lane half h = lane >> 5; both layouts use that same
// assignment so any A layout pairs with any B layout.
//   frag[q][t] for rows r0 + (lane & 31).
template <int LAY, int ROWS>
__device__ __forceinline__ void frag_load(const float *__restrict__ s, int r, int h, float (&fr)[2][4]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (LAY == LAY_K) {
      const float4 v = *reinterpret_cast<const float4 *>(s + r * SK + 4 * (2 * q + h));
      fr[q][0] = v.x; fr[q][1] = v.y; fr[q][2] = v.z; fr[q][3] = v.w;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) fr[q][t] = s[(8 * q + 4 * h + t) * (ROWS + 4) + r];
    }
  }
}

// WM = waves along M: 2 -> 128 x 128 tile (2 x 2 waves), 1 -> 64 x 256 tile (1 x 4 waves) for outputs
// with at most 64 rows (the panel products of the band reduction), where the square tile would
// spend half of its MFMAs on padding.
template <int ALAY, int BLAY, int WM = 2>
__global__ __launch_bounds__(256, 2) void gemm_kernel(GemmArgs p) {
  constexpr int WN = 4 / WM, BM = 64 * WM, BN = 64 * WN;
  constexpr int TA = tile_floats(BM), TB = tile_floats(BN);
  static_assert(WM == 1 || WM == 2, "wave grid");
  __shared__ __attribute__((aligned(16))) float smem[2 * TA + 2 * TB];
  if (p.desc) {  // batched mode: this problem's pointers and sizes come from device memory
    const GemmDesc ds = p.desc[blockIdx.z];
    p.A = ds.A; p.B = ds.B; p.C = ds.C;
    p.M = ds.M; p.N = ds.N; p.K = ds.K; p.lda = ds.lda; p.ldb = ds.ldb; p.ldc = ds.ldc;
    p.tiles_m = (int)((ds.M + BM - 1) / BM);
    p.tiles_n = (int)((ds.N + BN - 1) / BN);
    p.kchunk = ((ds.K + BK - 1) / BK) * BK;
    p.a_vec = ((reinterpret_cast<uintptr_t>(ds.A) & 15) == 0 && (ds.lda & 3) == 0) ? 1 : 0;
    p.b_vec = ((reinterpret_cast<uintptr_t>(ds.B) & 15) == 0 && (ds.ldb & 3) == 0) ? 1 : 0;
  }
  int ti, tj;
  if (!map_tile(p.syrk, p.sbw, p.tiles_m, p.tiles_n, ti, tj)) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int r = lane & 31, h = lane >> 5;

  const int64_t row0 = (int64_t)ti * BM, col0 = (int64_t)tj * BN;
  const int64_t kbeg = (int64_t)blockIdx.y * p.kchunk;
  const int64_t kend = (kbeg + p.kchunk < p.K) ? kbeg + p.kchunk : p.K;
  const int nt = (int)((kend - kbeg + BK - 1) / BK);

#define SA(b) (smem + (b) * TA)
#define SB_(b) (smem + 2 * TA + (b) * TB)

  f32x16 acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; tot[i][j][e] = 0.f; }
  // C prefetch (accumulating GEMMs on interior tiles): the second-level accumulator starts as (beta/alpha) C,
  // read while the K loop runs, instead of reading C after it with nothing left to hide the latency
  // (the rank-128 updates of the band reduction and the back-transformation have K = 128: 8 K tiles).
  const bool prefetch_c = p.ksplit <= 1 && p.beta != 0.f && p.alpha != 0.f && row0 + BM <= p.M && col0 + BN <= p.N;
  if (prefetch_c) {
    const float ba = p.beta / p.alpha;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        gcptr cbase = (gcptr)p.C + (row0 + wm * 64 + i * 32 + 4 * h) * p.ldc + col0 + wn * 64 + j * 32 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[i][j][e] = ba * cbase[(int64_t)((e & 3) + 8 * (e >> 2)) * p.ldc];
      }
  }

  // One K tile of MFMA work from LDS buffer `cur`.
  auto compute = [&](int cur) {
    float fa[2][2][4], fb[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) frag_load<ALAY, BM>(SA(cur), wm * 64 + i * 32 + r, h, fa[i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) frag_load<BLAY, BN>(SB_(cur), wn * 64 + j * 32 + r, h, fb[j]);
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][q][tt], fb[j][q][tt], acc[i][j], 0, 0, 0);
  };
  auto flush = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        tot[i][j] += acc[i][j];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
      }
  };

  // Register-staged double buffering: the loads of tile t+1 are issued BEFORE the MFMAs of tile t
  // and written to the other LDS buffer after them; one barrier per K tile.
  auto mainloop = [&](auto mode_tag) {
    constexpr int MODE = decltype(mode_tag)::value;
    constexpr bool FAST = MODE < 2;
    // modes 0/1 cover the full K tiles; a ragged last K tile goes through the scalar loader.
    const int nt_fast = FAST ? (int)((kend - kbeg) / BK) : 0;
    if constexpr (WM == 1) {
      // 64-row outputs stream their big operand once from HBM (the panel products of the band reduction):
      // two register sets keep the global loads TWO K tiles ahead (2 x 20 KB per workgroup in flight; with
      // one tile ahead the kernel was latency-bound at 1.4 TB/s)
      const int nt_fast = FAST ? (int)((kend - kbeg) / BK) : 0;
      float4 sA[2][BM / 64], sB[2][BN / 64];
      auto load2 = [&](int t, auto par) __attribute__((always_inline)) {
        constexpr int P = decltype(par)::value;
        const int64_t k0 = kbeg + (int64_t)t * BK;
        if (FAST && t < nt_fast) {
          tile_load<ALAY, MODE, BM>((gcptr)p.A, p.lda, row0, p.M, k0, kend, tid, sA[P]);
          tile_load<BLAY, MODE, BN>((gcptr)p.B, p.ldb, col0, p.N, k0, kend, tid, sB[P]);
        } else {
          tile_load<ALAY, 2, BM>((gcptr)p.A, p.lda, row0, p.M, k0, kend, tid, sA[P]);
          tile_load<BLAY, 2, BN>((gcptr)p.B, p.ldb, col0, p.N, k0, kend, tid, sB[P]);
        }
      };
      using P0 = std::integral_constant<int, 0>;
      using P1 = std::integral_constant<int, 1>;
      if (nt > 0) {
        load2(0, P0{});
        tile_store<ALAY, BM>(SA(0), tid, sA[0]);
        tile_store<BLAY, BN>(SB_(0), tid, sB[0]);
        if (nt > 1) load2(1, P1{});
      }
      __syncthreads();
      int since_flush = 0;
      // tile t: LDS buffer t & 1; register set t & 1 is free (tile t is in LDS) and receives tile t + 2;
      // tile t + 1 waits in set (t + 1) & 1 and is written to LDS after the MFMAs
      auto step = [&](int t, auto par) __attribute__((always_inline)) {
        constexpr int P = decltype(par)::value;
        if (t + 2 < nt) load2(t + 2, par);
        compute(P);
        if (++since_flush == FLUSH_TILES) { since_flush = 0; flush(); }
        if (t + 1 < nt) {
          tile_store<ALAY, BM>(SA(P ^ 1), tid, sA[P ^ 1]);
          tile_store<BLAY, BN>(SB_(P ^ 1), tid, sB[P ^ 1]);
        }
        __syncthreads();
      };
      int t = 0;
      for (; t + 1 < nt; t += 2) {
        step(t, P0{});
        step(t + 1, P1{});
      }
      if (t < nt) step(t, P0{});
      return;
    }
    float4 stA[BM / 64], stB[BN / 64];
    auto load = [&](int t) {
      const int64_t k0 = kbeg + (int64_t)t * BK;
      if (FAST && t < nt_fast) {
        tile_load<ALAY, MODE, BM>((gcptr)p.A, p.lda, row0, p.M, k0, kend, tid, stA);
        tile_load<BLAY, MODE, BN>((gcptr)p.B, p.ldb, col0, p.N, k0, kend, tid, stB);
      } else {
        tile_load<ALAY, 2, BM>((gcptr)p.A, p.lda, row0, p.M, k0, kend, tid, stA);
        tile_load<BLAY, 2, BN>((gcptr)p.B, p.ldb, col0, p.N, k0, kend, tid, stB);
      }
    };
    if (nt > 0) {
      load(0);
      tile_store<ALAY, BM>(SA(0), tid, stA);
      tile_store<BLAY, BN>(SB_(0), tid, stB);
    }
    __syncthreads();
    int since_flush = 0;
    for (int t = 0; t < nt; ++t) {
      const int cur = t & 1;
      if (t + 1 < nt) load(t + 1);
      compute(cur);
      if (++since_flush == FLUSH_TILES) { since_flush = 0; flush(); }
      if (t + 1 < nt) {
        tile_store<ALAY, BM>(SA(cur ^ 1), tid, stA);
        tile_store<BLAY, BN>(SB_(cur ^ 1), tid, stB);
      }
      __syncthreads();
    }
  };
  // a LAY_M operand needs its row count to be a multiple of 4 for the clamped vector mode
  const bool vec_ok = p.a_vec && p.b_vec && (ALAY == LAY_K || (p.M & 3) == 0) && (BLAY == LAY_K || (p.N & 3) == 0);
  const bool full = row0 + BM <= p.M && col0 + BN <= p.N;
  if (vec_ok && full) mainloop(std::integral_constant<int, 0>{});
  else if (vec_ok) mainloop(std::integral_constant<int, 1>{});
  else mainloop(std::integral_constant<int, 2>{});
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) tot[i][j] += acc[i][j];

  // ---- epilogue.  C/D map of the 32x32 MFMA: col = lane & 31, row = (e&3) + 8*(e>>2) + 4*h.
  const bool partial = p.ksplit > 1;
  gptr Cout = (gptr)(partial ? p.slab + (int64_t)blockIdx.y * p.M * p.N : p.C);
  const int64_t ldc = partial ? p.N : p.ldc;
  const float alpha = partial ? 1.f : p.alpha;
  const float beta = partial ? 0.f : p.beta;

  const bool full_tile = row0 + BM <= p.M && col0 + BN <= p.N;
  if (full_tile) {
    // unguarded epilogue: all loads (beta != 0) are issued before the first use
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        gptr cbase = Cout + (row0 + wm * 64 + i * 32 + 4 * h) * ldc + col0 + wn * 64 + j * 32 + r;
        float old[16];
        const bool rd = beta != 0.f && !prefetch_c;
        if (rd) {
#pragma unroll
          for (int e = 0; e < 16; ++e) old[e] = cbase[(int64_t)((e & 3) + 8 * (e >> 2)) * ldc];
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float v = alpha * tot[i][j][e];
          if (rd) v += beta * old[e];
          cbase[(int64_t)((e & 3) + 8 * (e >> 2)) * ldc] = v;
          tot[i][j][e] = v;  // final value: the mirrored store below reuses it
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t col = col0 + wn * 64 + j * 32 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int64_t row = row0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
          float v = alpha * tot[i][j][e];
          if (row < p.M && col < p.N) {
            gptr c = Cout + row * ldc + col;
            if (beta != 0.f) v += beta * *c;
            *c = v;
          }
          tot[i][j][e] = v;
        }
      }
  }

  if (WM == 2 && p.syrk == 1 && !partial && ti != tj) {
    // Mirror image: C[col][row] = same value, transposed through LDS (32x33 floats per wave)
    // so that the second store is also 128-B coalesced.
    // (each wave transposes through its own LDS patch: wave-local ordering suffices, no workgroup barrier
    // per block; all waves left the K loop through its final barrier)
    float *ts = smem + wave * (32 * 33);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
        for (int e = 0; e < 16; ++e) ts[r * 33 + (e & 3) + 8 * (e >> 2) + 4 * h] = tot[i][j][e];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int64_t mrow0 = col0 + wn * 64 + j * 32;  // rows of the mirrored block
        const int64_t mcol = row0 + wm * 64 + i * 32 + r;
#pragma unroll
        for (int rr = 0; rr < 32; rr += 2) {
          const int64_t mrow = mrow0 + rr + h;
          if (mrow < p.N && mcol < p.M) {
            // C is symmetric on entry (SYRK accumulate / symmetric rank-2k update), so the mirror
            // image equals the value just stored in the lower tile: no second read of C
            gptr c = (gptr)p.C + mrow * p.ldc + mcol;
            *c = ts[(rr + h) * 33 + r];
          }
        }
      }
  }
}

// ---- Tile128: gemm_kernel, every shape
// wave grid of the tile: 1 x 4 waves (64 x 256) when the output has at most 64 rows and is wide
static int pick_wm(int64_t M, int64_t N, bool syrk) { return (!syrk && M <= 64 && N > 128) ? 1 : 2; }

bool plan_tile128(const GemmShape &sh, GemmPlan &pl) {
  const int64_t M = sh.M, N = sh.N, K = sh.K;
  const bool syrk = sh.syrk;
  pl = GemmPlan{};
  pl.route = GemmRoute::Tile128;
  const int wm = pick_wm(M, N, syrk);
  const int64_t tm = cdiv(M, 64 * wm), tn = cdiv(N, 256 / wm);
  const int64_t tiles = syrk ? tm * (tm + 1) / 2 : tm * tn;
  pl.ksplit = 1;
  pl.kchunk = cdiv(K, BK) * BK;
  if (pl.kchunk < BK) pl.kchunk = BK;
  const int64_t ktiles = cdiv(K, BK);
  // Fill at least ~2 workgroups per CU when the output has few tiles and K is deep; keep every
  // split at least 32 K tiles long and the slab modest.
  if (tiles < 256 && ktiles >= 64) {
    // one resident round (2 workgroups per CU x 256 CUs) for compute-bound shapes; a one-tile-wide
    // output streams its big operand once and is bandwidth-bound: more, shorter splits keep enough
    // bytes in flight
    int64_t want = (tm == 1 || tn == 1) ? 2048 / tiles : 512 / tiles;
    int64_t maxs = (tm == 1 || tn == 1) ? ktiles / 8 : ktiles / 32;
    int64_t s = want < maxs ? want : maxs;
    // a single-tile output (the 64 x 64 Gram blocks of the band reduction's panels: both operands stream 64 rows
    // x m) has nothing but split-K to spread over the chip (with the slot rotation of map_tile: before it every
    // split's only valid workgroup sat on XCD 0 and more splits bought nothing); at most 64 splits for any output
    if (s > 64) s = 64;
    while (s > 1 && (size_t)s * (size_t)M * (size_t)N * 4 > ((size_t)1 << 30)) --s;
    if (s > 1) {
      pl.kchunk = cdiv(ktiles, s) * BK;
      pl.ksplit = (int)cdiv(K, pl.kchunk);
    }
  }
  pl.slab_bytes = pl.ksplit > 1 ? (size_t)pl.ksplit * (size_t)M * (size_t)N * sizeof(float) : 0;
  pl.bytes = pl.slab_bytes;
  return true;
}

int launch_tile128(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, size_t workspace_bytes,
                          hipStream_t stream) {
  p.ksplit = pl.ksplit;
  p.kchunk = pl.kchunk;
  p.slab = nullptr;
  if (p.ksplit > 1) {
    if (!workspace || workspace_bytes < pl.bytes) return VIVIT_E_WORKSPACE;
    p.slab = ws_at<float>(workspace, pl.slab_off);
  }
  const int wm = pick_wm(p.M, p.N, sh.syrk);
  p.tiles_m = (int)cdiv(p.M, 64 * wm);
  p.tiles_n = (int)cdiv(p.N, 256 / wm);
  p.syrk = sh.syrk ? 1 : 0;
  p.a_vec = operand_vec(p.A, p.lda);
  p.b_vec = operand_vec(p.B, p.ldb);
  p.desc = nullptr;
  const int64_t nsb = tile_grid(p.tiles_m, p.tiles_n, sh.syrk, &p.sbw);
  if (nsb < 0) return VIVIT_E_UNSUPPORTED;
  dim3 grid((unsigned)(nsb * 256), (unsigned)p.ksplit, 1);
  dim3 block(256, 1, 1);
  const bool prof = sh.syrk && p.A == p.B && prof_enabled() && sh.pub;  // only the caller's Gram SYRK is profiled as such
  if (prof) prof_begin(0, (double)p.M * (double)(p.M + 1) * (double)p.K, stream);
  with_layouts(alay, blay, [&](auto LA, auto LB) {
    if (wm == 1)
      gemm_kernel<LA, LB, 1><<<grid, block, 0, stream>>>(p);
    else
      gemm_kernel<LA, LB><<<grid, block, 0, stream>>>(p);
  });
  if (prof) prof_end(0, stream);
  int st = launch_status();
  if (st != VIVIT_OK) return st;
  if (p.ksplit > 1) {
    launch_gemm_reduce(p.slab, p.C, p.M, p.N, p.ldc, p.ksplit, p.alpha, p.beta, p.syrk, stream);
    st = launch_status();
  }
  return st;
}

int gemm_lower_launch(const float *A, const float *B, float *C, int64_t n, int64_t K, int64_t lda, int64_t ldb,
                      int64_t ldc, float alpha, float beta, hipStream_t stream) {
  if (n <= 0) return VIVIT_OK;
  if (!A || !B || !C || K <= 0 || lda < n || ldb < n || ldc < n) return VIVIT_E_BADARG;
  GemmArgs p;
  p.A = A; p.B = B; p.C = C;
  p.M = n; p.N = n; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.alpha = alpha; p.beta = beta;
  p.ksplit = 1;
  p.kchunk = cdiv(K, BK) * BK;
  p.slab = nullptr;
  p.tiles_m = p.tiles_n = (int)cdiv(n, BM);
  p.syrk = 2;
  p.a_vec = operand_vec(A, lda);
  p.b_vec = operand_vec(B, ldb);
  p.desc = nullptr;
  p.sbw = SB;
  const int64_t sbm = cdiv(p.tiles_m, SB);
  const int64_t nsb = sbm * (sbm + 1) / 2;
  gemm_kernel<LAY_M, LAY_M><<<dim3((unsigned)(nsb * 256), 1, 1), 256, 0, stream>>>(p);
  return launch_status();
}

int gemm_batched_launch(int alay, int blay, const GemmDesc *desc, int batch, int64_t maxM, int64_t maxN, float alpha,
                        float beta, hipStream_t stream) {
  if (batch <= 0 || maxM <= 0 || maxN <= 0) return VIVIT_OK;
  if (!desc) return VIVIT_E_BADARG;
  GemmArgs p;
  p.A = nullptr; p.B = nullptr; p.C = nullptr;
  p.M = maxM; p.N = maxN; p.K = 0; p.lda = p.ldb = p.ldc = 0;
  p.alpha = alpha; p.beta = beta;
  p.ksplit = 1;
  p.kchunk = BK;
  p.slab = nullptr;
  p.tiles_m = (int)cdiv(maxM, BM);
  p.tiles_n = (int)cdiv(maxN, BN);
  p.syrk = 0;
  p.a_vec = p.b_vec = 0;
  p.desc = desc;
  const int64_t nsb = tile_grid(p.tiles_m, p.tiles_n, false, &p.sbw);
  if (nsb < 0 || batch > 65535) return VIVIT_E_UNSUPPORTED;
  dim3 grid((unsigned)(nsb * 256), 1, (unsigned)batch);
  with_layouts(alay, blay, [&](auto LA, auto LB) { gemm_kernel<LA, LB><<<grid, 256, 0, stream>>>(p); });
  return launch_status();
}

} // namespace vivit
