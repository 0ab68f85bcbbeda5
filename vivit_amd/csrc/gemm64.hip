// Streaming variant for outputs with at most 64 rows (the panel product P^T = V^T A22 of the band
// reduction: 64 x m x m, its big operand read exactly once from HBM, 32 flop/byte).  Such a product is
// HBM-bound and needs ~100 KB in flight per CU; the register-staged tile has 20-40.  Same global -> LDS
// DMA and swizzled tiles as gemm256_kernel, 64 x 256 tile (four waves of 64 x 64), SEVEN LDS stages of
// 20 KB: six K tiles (120 KB) are in flight while one is being multiplied.  Accumulators are 64 registers,
// nothing spills, so the waits are plain asm `s_waitcnt vmcnt(20)` (all but the four newest tiles landed).
#include "gemm_plan.h"

namespace vivit {

constexpr int G64_NST = 7;
constexpr int G64_TA = 64 * BK, G64_TB = 256 * BK, G64_STG = G64_TA + G64_TB;  // floats
constexpr int GEMM64_LDS_BYTES = G64_NST * G64_STG * 4;                        // 140 KB

template <int ALAY, int BLAY>
__global__ __launch_bounds__(256, 1) void gemm64_dma_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem3[];
  // stand-in for a public gemm64_bx_kernel launch (same grid and slab): runs only when that launch flagged an operand
  if (p.gate && (*p.gate & p.gate_mask) == 0) return;
  const int tj = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t col0 = (int64_t)tj * 256;
  const int64_t kbeg = (int64_t)blockIdx.y * p.kchunk;
  const int64_t kend = (kbeg + p.kchunk < p.K) ? kbeg + p.kchunk : p.K;
  const int nt = (int)((kend - kbeg) / BK);  // K and kchunk are multiples of 16 (host)

  f32x16 acc[2][2];
  auto clear_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  };
  clear_acc();

  const bool partial = p.ksplit > 1 || p.gate;
  gptr Cout = (gptr)(partial ? p.slab + (int64_t)blockIdx.y * p.M * p.N : p.C);
  const int64_t ldc = partial ? p.N : p.ldc;
  const float alpha = partial ? 1.f : p.alpha;
  const float beta0 = partial ? 0.f : p.beta;
  auto flush_to_c = [&](bool first) __attribute__((always_inline)) {
    const float beta = first ? beta0 : 1.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t col = col0 + wave * 64 + j * 32 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int64_t row = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
          if (row < p.M && col < p.N) {
            gptr c = Cout + row * ldc + col;
            float v = alpha * acc[i][j][e];
            if (beta != 0.f) v += beta * *c;
            *c = v;
          }
        }
      }
  };

  float fa[2][2][4], fb[2][2][4];  // [half parity][tile][k pair]
  auto frags = [&](int st, int q, int par) __attribute__((always_inline)) {
    const float *sa = smem3 + st * G64_STG, *sb = sa + G64_TA;
#pragma unroll
    for (int i = 0; i < 2; ++i) frag_half<ALAY, 64>(sa, i * 32 + r, q, h, fa[par][i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) frag_half<BLAY, 256>(sb, wave * 64 + j * 32 + r, q, h, fb[par][j]);
  };
  auto mfma_half = [&](int par) __attribute__((always_inline)) {
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[par][i][tt], fb[par][j][tt], acc[i][j], 0, 0, 0);
  };

  // DMA sources: wave w moves block w of the A tile and blocks w, w+4, w+8, w+12 of the B tile
  gcptr srcA = dma_src<ALAY, 64>(p.A, p.lda, 0, p.M, wave, lane) + (ALAY == LAY_K ? kbeg : kbeg * p.lda);
  gcptr srcB[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    srcB[u] = dma_src<BLAY, 256>(p.B, p.ldb, col0, p.N, wave + 4 * u, lane) + (BLAY == LAY_K ? kbeg : kbeg * p.ldb);
  const int64_t stepA = (ALAY == LAY_K) ? BK : (int64_t)BK * p.lda, stepB = (BLAY == LAY_K) ? BK : (int64_t)BK * p.ldb;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)smem3 +
                                                       (unsigned)(wave * 256 * 4));
  auto issue = [&](int st) __attribute__((always_inline)) {
    const unsigned base = lds0 + (unsigned)(st * G64_STG * 4);
    dma16(srcA, base);
    srcA += stepA;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dma16(srcB[u], base + (unsigned)((G64_TA + 4 * u * 256) * 4));
      srcB[u] += stepB;
    }
  };

  bool first_flush = true;
  constexpr int FL = 8192 / BK;
  for (int c0 = 0; c0 < nt; c0 += FL) {
    const int c1 = c0 + FL < nt ? c0 + FL : nt;
    if (c0 > 0) clear_acc();
    __syncthreads();
    // tiles c0 .. c0+NST-2 requested up front; tile t lives in stage (t - c0) % NST
    int issued = c0;
    for (; issued < c1 && issued < c0 + G64_NST - 1; ++issued) issue((issued - c0) % G64_NST);
    // first tile landed (everything but the younger requests)
    if (issued - c0 >= 2) {
      // wait for tile c0 only if enough tiles are in flight to express it with a constant; else wait for all
      if (issued - c0 == G64_NST - 1) __asm__ volatile("s_waitcnt vmcnt(25)" ::: "memory");  // (NST-2) * 5
      else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    frags(0, 0, 0);
    for (int t = c0; t < c1; ++t) {
      const int st = (t - c0) % G64_NST, st1 = (t + 1 - c0) % G64_NST;
      // own part of tile t+1 landed: at most tiles t+2 .. t+NST-2 (NST-3 of them) may still be in flight
      if (issued - (t + 2) >= G64_NST - 3) __asm__ volatile("s_waitcnt vmcnt(20)" ::: "memory");
      else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (issued < c1) {  // request tile t+NST-1 into the stage tile t-1 has left
        issue((issued - c0) % G64_NST);
        ++issued;
      }
      frags(st, 1, 1);
      mfma_half(0);
      __builtin_amdgcn_sched_barrier(0);
      if (t + 1 < c1) {
        __syncthreads();  // every wave's part of tile t+1 is in LDS; tile t-1's stage is free for the next request
        frags(st1, 0, 0);
      }
      mfma_half(1);
      __builtin_amdgcn_sched_barrier(0);
    }
    flush_to_c(first_flush);
    first_flush = false;
  }
}

// ---- The same 64-row streaming product on the bf16 pipe (round 4).
// The fp32 kernel above is bound by its own MFMAs (32 of 64 cycles per K tile and wave: 2.1 ms for 64 x 40960 x 40960
// where the DMA stream alone takes 1.1 ms, scripts/probe/panel_product.py on timing-only builds, since removed).  Here every product is
// six v_mfma_f32_32x32x16_bf16 on exact three-way bf16 splits (24 MFMAs of 32 cycles per K tile and wave):
//   * the small operand A (64 x K, read by every workgroup) is split ONCE by g64_split_a_kernel into the fragment
//     order of the MFMA -- per K tile [row tile 2][piece 3][lane 64][8 bf16] = 6 KB -- and streamed by DMA like B;
//   * the big operand B (K x N or N x K, fp32, read exactly once from HBM) is split in registers by the wave that
//     multiplies it: 16 values per lane and K tile (~100 VALU instructions), issued between the MFMAs of the PREVIOUS
//     tile (pieces are double-buffered in registers; one wave per SIMD owns the SIMD's 512 registers).
// Splitting both operands in registers was measured too: ~200 VALU instructions per tile do not fit the MFMA gaps
// (1.88 ms).  Element j of a lane's eight values of a K tile is k = 8 (j >> 2) + 4 h + (j & 3) for both operands (the order
// frag_half delivers B in), which is all a 16-deep MFMA needs.  One DMA stream runs over the whole K range of the
// workgroup; accumulation chains are closed in registers every 2048 k (the MFMA's truncating accumulator: see
// bx_chain_tiles) and C or the split-K slab is written once.
constexpr int G64X_NST = 7;
constexpr int G64X_TA = 6 * 1024 / 4;                 // floats: the A pieces of one K tile (6 KB)
constexpr int G64X_STG = G64X_TA + G64_TB;            // 22 KB per stage
constexpr int GEMM64X_LDS_BYTES = G64X_NST * G64X_STG * 4;  // 154 KB
constexpr int G64X_CHAIN = 2048 / BK;

// this lane's K index inside a K tile for element j of its MFMA fragment
__device__ __forceinline__ int g64x_k(int h, int j) { return 8 * (j >> 2) + 4 * h + (j & 3); }

// Range gate of the PUBLIC 64-row product (STRICT instances; the band reduction's own product keeps the plain ones): the
// two bits of bx_split_kernel, gathered per lane as the largest 2|a| bit pattern (bit 0: >= 2 x 0x7F7F8000, NaN above it)
// and the smallest 2|a| - 1 (bit 1: below 2 x 0x0D800000 - 1, i.e. 0 < |a| < 2^-100; an exact zero wraps to the top) --
// three VALU instructions per value, no compare per value -- and ORed into one flag per launch.  A flagged product is
// recomputed by gemm64_dma_kernel (fp32 MFMA) behind the bf16-pipe launch; see launch_gemm64.
struct G64Range {
  unsigned mx = 0u, mn = 0xffffffffu;
};
__device__ __forceinline__ void g64_range_add(G64Range &g, float a) {
  const unsigned u = __float_as_uint(a) << 1;
  g.mx = max(g.mx, u);
  g.mn = min(g.mn, u - 1u);
}
__device__ __forceinline__ void g64_range_flag(const G64Range &g, int *flag) {
  const bool big = g.mx >= (0x7F7F8000u << 1), tiny = g.mn < (0x0D800000u << 1) - 1u;
  const unsigned long long m0 = __builtin_amdgcn_ballot_w64(big), m1 = __builtin_amdgcn_ballot_w64(tiny);
  if ((m0 | m1) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, (m0 ? BX_GATE_RANGE : 0) | (m1 ? BX_GATE_TINY : 0));  // rare
}

template <int ALAY, bool STRICT = false>
__global__ __launch_bounds__(128) void g64_split_a_kernel(const float *__restrict__ A, int64_t lda, int64_t M, uint4 *__restrict__ out,
                                                          int *__restrict__ flag) {
  const int64_t kt = blockIdx.x;
  const int i = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5;
  const int64_t row = 32 * i + (l & 31);
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t k = kt * BK + g64x_k(h, j);
    f[j] = row < M ? (ALAY == LAY_K ? A[row * lda + k] : A[k * lda + row]) : 0.f;
  }
  if constexpr (STRICT) {
    G64Range g;
#pragma unroll
    for (int j = 0; j < 8; ++j) g64_range_add(g, f[j]);
    g64_range_flag(g, flag);
  }
  unsigned hh[4], mm[4], ll[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) bx_split2(f[2 * u], f[2 * u + 1], hh[u], mm[u], ll[u]);
  uint4 *o = out + (kt * 6 + i * 3) * 64 + l;
  o[0] = make_uint4(hh[0], hh[1], hh[2], hh[3]);
  o[64] = make_uint4(mm[0], mm[1], mm[2], mm[3]);
  o[128] = make_uint4(ll[0], ll[1], ll[2], ll[3]);
}

// STRICT (public products): also gathers the range bits of every B value it splits (G64Range) into *flag, and always writes
// the split-K slab (one slice when ksplit is 1), so that the gated fp32 kernel behind it can still replace the whole result.
template <int BLAY, bool STRICT = false>
__global__ __launch_bounds__(256, 1) void gemm64_bx_kernel(GemmArgs p, const uint4 *__restrict__ apieces, int *__restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) float smem3[];
  const int tj = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t col0 = (int64_t)tj * 256;
  const int64_t kbeg = (int64_t)blockIdx.y * p.kchunk;
  const int64_t kend = (kbeg + p.kchunk < p.K) ? kbeg + p.kchunk : p.K;
  const int nt = (int)((kend - kbeg) / BK);  // K and kchunk are multiples of 16 (host)

  f32x16 acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f, tot[i][j][e] = 0.f;

  // DMA sources: wave w moves bytes [1536 w, 1536 w + 1536) of the A pieces (one full and one half-wave request) and
  // blocks w, w+4, w+8, w+12 of the B tile
  gcptr srcB[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    srcB[u] = dma_src<BLAY, 256>(p.B, p.ldb, col0, p.N, wave + 4 * u, lane) + (BLAY == LAY_K ? kbeg : kbeg * p.ldb);
  const int64_t stepB = (BLAY == LAY_K) ? BK : (int64_t)BK * p.ldb;
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)smem3;
  const unsigned ldsA = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(wave * 1536)),
                 ldsB = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(G64X_TA * 4 + wave * 1024));
  // Round 6: the requests take a wave-uniform base in scalar registers + ONE 32-bit offset per lane and stream instead of a
  // 64-bit pointer per lane (global_load_lds_dwordx4 v, s[..]): in the 256-tile kernel's K loop that is what a request's cost
  // to the SIMD hangs on (~25 cycles against ~3, gemm256_bx_kernel).  A lane's offset from the first row of the tile is
  // below 256 rows x ldb x 4 bytes; it does not change along K.  Same-box A/B against the per-lane pointers
  // of rounds 4-5 on N(0,1) data (profiles/r06_g64_ab.log): m = 40 960: 1820-1886 against 1884-1898 us; m = 20 480: 470-484
  // against 509-515 us.
  gcptr baseA = (gcptr)(reinterpret_cast<const char *>(apieces) + (kbeg / BK) * 6144) + __builtin_amdgcn_readfirstlane(wave * (1536 / 4));
  gcptr baseB = (gcptr)p.B + (BLAY == LAY_K ? (col0 < p.N ? col0 : 0) * p.ldb + kbeg : kbeg * p.ldb + (col0 < p.N ? col0 : 0));
  const unsigned voffA = (unsigned)lane * 16u;
  unsigned voffB[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) voffB[u] = (unsigned)((const char *)srcB[u] - (const char *)baseB);
  auto dma16s = [](gcptr base, unsigned voff, unsigned lds_byte_addr) __attribute__((always_inline)) {
    __asm__ volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_byte_addr), "v"(voff), "s"(base) : "memory");
  };
  auto issue = [&](int st) __attribute__((always_inline)) {   // 6 requests per wave
    const unsigned so = (unsigned)(st * G64X_STG * 4);
    dma16s(baseA, voffA, ldsA + so);
    if (lane < 32) dma16s(baseA + 256, voffA, ldsA + so + 1024);   // (+256 floats = 1 KB; counted by vmcnt whatever the exec mask)
    baseA += 6144 / 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) dma16s(baseB, voffB[u], ldsB + so + (unsigned)(4 * u * 1024));
    baseB += stepB;
  };

  struct P3 { bf16x8 h, m, l; };
  P3 pa[2][2], pb[2][2];   // [tile parity][row / column tile]
  float raw[2][8];         // the next K tile's B fragments as read from LDS (columns 0-31, 32-63 of the wave's 64)
  auto read_next = [&](int st, int par) __attribute__((always_inline)) {
    const float *sa = smem3 + st * G64X_STG, *sb = sa + G64X_TA;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bf16x8 *q = reinterpret_cast<const bf16x8 *>(sa) + (i * 3) * 64 + lane;
      pa[par][i].h = q[0];
      pa[par][i].m = q[64];
      pa[par][i].l = q[128];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      frag_half<BLAY, 256>(sb, wave * 64 + j * 32 + r, 0, h, *reinterpret_cast<float(*)[4]>(&raw[j][0]));
      frag_half<BLAY, 256>(sb, wave * 64 + j * 32 + r, 1, h, *reinterpret_cast<float(*)[4]>(&raw[j][4]));
    }
  };
  // (STRICT: every split_raw call sees real B values of this workgroup -- the one after its last tile reads the stage of tile
  // nt - 7, and every split has more than 40 K tiles (plan_gemm64) -- so no uninitialised LDS reaches the flag)
  G64Range rng;
  auto split_raw = [&](int par) __attribute__((always_inline)) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    if constexpr (STRICT) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int u = 0; u < 8; ++u) g64_range_add(rng, raw[j][u]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned hh[4], mm[4], ll[4];
      // (13 instructions per pair as hipcc compiles it; a 9-instruction form -- packed subtractions in inline asm, the
      // packed conversion hidden from the optimiser -- ran 7 % SLOWER on the same box: hazard s_nops around the asm)
#pragma unroll
      for (int u = 0; u < 4; ++u) bx_split2(raw[j][2 * u], raw[j][2 * u + 1], hh[u], mm[u], ll[u]);
      pb[par][j].h = __builtin_bit_cast(bf16x8, (u32x4){hh[0], hh[1], hh[2], hh[3]});
      pb[par][j].m = __builtin_bit_cast(bf16x8, (u32x4){mm[0], mm[1], mm[2], mm[3]});
      pb[par][j].l = __builtin_bit_cast(bf16x8, (u32x4){ll[0], ll[1], ll[2], ll[3]});
    }
  };
  auto mfma_bx = [&](int par) __attribute__((always_inline)) {
    // six partial products per output tile, smallest first; the four tiles' chains interleaved
#define G64_BX4(PA, PB)                                                                                                 \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[i][j] =             \
      __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[par][i].PA, pb[par][j].PB, acc[i][j], 0, 0, 0);
    G64_BX4(l, h) G64_BX4(h, l) G64_BX4(m, m) G64_BX4(m, h) G64_BX4(h, m) G64_BX4(h, h)
#undef G64_BX4
  };

  int issued = 0, ist = 0;   // tiles requested so far; the stage the next request goes to
  for (; issued < nt && issued < G64X_NST - 1; ++issued, ++ist) issue(ist);
  if (issued == G64X_NST - 1) __asm__ volatile("s_waitcnt vmcnt(30)" ::: "memory");  // (NST-2) * 6: tile 0 landed
  else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  read_next(0, 0);
  split_raw(0);
  int t = 0, st1 = 1;
  // tile t: its pieces are in registers (parity par); tile t+1 is read from LDS and split while tile t's 24 MFMAs run
  auto step = [&](int par) __attribute__((always_inline)) {
    if (issued < nt) {
      // own part of tile t+1 landed: tiles t+2 .. t+NST-2 (NST-3 of them) may still be in flight
      __asm__ volatile("s_waitcnt vmcnt(24)" ::: "memory");
      issue(ist);  // tile t+NST-1 into the stage tile t-1 has left (its LDS reads ended before the previous barrier)
      ++issued;
      ist = ist + 1 == G64X_NST ? 0 : ist + 1;
    } else {
      __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();           // every wave's part of tile t+1 is in LDS
    read_next(st1, par ^ 1);   // (after the last tile: a stale stage, the values are not used)
    __builtin_amdgcn_sched_barrier(0);
    mfma_bx(par);
    split_raw(par ^ 1);
    // (an empty use, so that the split stays in this block: the compiler sinks it into the next step's otherwise)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __asm__ volatile("" : "+v"(pb[par ^ 1][j].h), "+v"(pb[par ^ 1][j].m), "+v"(pb[par ^ 1][j].l));
    // the split's ~100 VALU instructions between the MFMAs: 4 MFMAs first (the LDS reads are on their way), then 5 : 1
    // (STRICT: ~150 with the range bits, 7 : 1)
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
#pragma unroll
    for (int u = 0; u < 20; ++u) {
      __builtin_amdgcn_sched_group_barrier(0x002, STRICT ? 7 : 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    ++t;
    st1 = st1 + 1 == G64X_NST ? 0 : st1 + 1;
  };
  static_assert(G64X_CHAIN % 2 == 0, "chains hold whole pairs of tiles (the register parity of the pieces)");
  while (t < nt) {
    const int len = nt - t < G64X_CHAIN ? nt - t : G64X_CHAIN;   // this chain; only the last one can be odd
    for (int c = 0; c < len / 2; ++c) {
      step(0);
      step(1);
    }
    if (len & 1) step(0);
#pragma unroll
    for (int i = 0; i < 2; ++i)   // close the chain in registers
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          tot[i][j][e] += acc[i][j][e];
          acc[i][j][e] = 0.f;
        }
  }

  if constexpr (STRICT) g64_range_flag(rng, flag);
  const bool partial = STRICT || p.ksplit > 1;
  gptr Cout = (gptr)(partial ? p.slab + (int64_t)blockIdx.y * p.M * p.N : p.C);
  const int64_t ldc = partial ? p.N : p.ldc;
  const float alpha = partial ? 1.f : p.alpha, beta = partial ? 0.f : p.beta;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t col = col0 + wave * 64 + j * 32 + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t row = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (row < p.M && col < p.N) {
          gptr c = Cout + row * ldc + col;
          float v = alpha * tot[i][j][e];
          if (beta != 0.f) v += beta * *c;
          *c = v;
        }
      }
    }
}

// hipFuncAttributeMaxDynamicSharedMemorySize of the 64-row streaming kernels, once per device
static bool gemm64_attrs() {
  static unsigned long long attr_done = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (attr_done & (1ull << (dev & 63))) return true;
  const struct { const void *fn; int bytes; } kernels[] = {
      {reinterpret_cast<const void *>(gemm64_dma_kernel<LAY_K, LAY_K>), GEMM64_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm64_dma_kernel<LAY_K, LAY_M>), GEMM64_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm64_dma_kernel<LAY_M, LAY_K>), GEMM64_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm64_dma_kernel<LAY_M, LAY_M>), GEMM64_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm64_bx_kernel<LAY_K>), GEMM64X_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm64_bx_kernel<LAY_M>), GEMM64X_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm64_bx_kernel<LAY_K, true>), GEMM64X_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm64_bx_kernel<LAY_M, true>), GEMM64X_LDS_BYTES}};
  for (const auto &k : kernels)
    if (!ensure_dynamic_lds(k.fn, k.bytes, attr_done)) return false;
  attr_done |= 1ull << (dev & 63);
  return true;
}

// ---- Gemm64: the 64-row streaming kernels, split-K so that ~2 workgroups per CU exist (one resident at a time: 140 KB LDS)
// Workspace: the slab, behind it the bf16 pieces of the 64-row operand (gemm64_bx_kernel: 6 KB per K tile), behind them
// the range flag of a public product.
bool plan_gemm64(const GemmShape &sh, GemmPlan &pl) {
  const int64_t M = sh.M, N = sh.N, K = sh.K;
  if (sh.syrk || !(M <= 64 && N >= 2048 && K >= 2048 && (K % BK) == 0)) return false;
  pl = GemmPlan{};
  pl.route = GemmRoute::Gemm64;
  const int64_t tiles = cdiv(N, 256), ktiles = K / BK;
  // one workgroup per CU: pick the split count (>= 2 rounds of work, every split >= 64 K tiles) whose last
  // round of 256 workgroups is fullest
  int64_t s = 1;
  double best = 0.0;
  for (int64_t c = 1; c <= 24; ++c) {
    if (c > 1 && ktiles / c < 64) break;
    const int64_t wgs = tiles * c;
    const double fill = (double)wgs / (double)(256 * cdiv(wgs, 256));
    const double score = wgs >= 512 ? fill : fill * 0.5 * (double)wgs / 512.0;  // too few workgroups: latency-bound
    if (score > best + 1e-9) { best = score; s = c; }
  }
  pl.kchunk = cdiv(ktiles, s) * BK;
  pl.ksplit = (int)cdiv(K, pl.kchunk);
  // a public product on the bf16 pipe always goes through the slab (its gated fp32 stand-in may replace the partial sums)
  const bool strict = gemm64_bx_enabled() && sh.pub;
  pl.slab_bytes = (pl.ksplit > 1 || strict) ? (size_t)pl.ksplit * (size_t)M * (size_t)N * sizeof(float) : 0;
  pl.bytes = pl.slab_bytes;
  if (!gemm64_bx_enabled()) return true;
  pl.a_off = align_up(pl.slab_bytes, 256);
  const size_t pieces_end = pl.a_off + (size_t)ktiles * 6144;
  pl.flags_off = align_up(pieces_end, 256);
  pl.bytes = strict ? pl.flags_off + 256 : pieces_end;
  return true;
}

// gemm64_bx_kernel addresses B as a scalar base + a 32-bit byte offset per lane: up to 255 rows of ldb floats (K-contiguous B)
// or 15 k rows (k-major B), + 1 KB inside a row.  Wider leading dimensions would wrap it (silently: the request reads another row
// of the same operand), so they take gemm64_dma_kernel, whose lane addresses are 64-bit.
static bool gemm64_bx_reach(int blay, int64_t ldb) {
  return (int64_t)(blay == LAY_K ? 255 : 15) * ldb * 4 + 1024 < ((int64_t)1 << 32);
}

int launch_gemm64(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, size_t workspace_bytes,
                         hipStream_t stream) {
  p.ksplit = pl.ksplit;
  p.kchunk = pl.kchunk;
  // Which kernel runs depends on SHAPE (leading dimensions included) and ENVIRONMENT only (results are bit-identical from call
  // to call, include/vivit_hip.h): a workspace smaller than the query's answer is refused -- it is never a silent switch to the
  // fp32 kernel, whose summation order (and speed) differs.
  const bool bx = gemm64_bx_enabled() && gemm64_bx_reach(blay, p.ldb);
  // Public products on the bf16 pipe (INPUT RANGE CONTRACT): both split kernels OR the range bits of their operand into a flag,
  // the bf16-pipe product writes the slab, gemm64_dma_kernel on the same grid returns at once unless the flag is set and
  // otherwise rewrites the whole slab in fp32, and the reduce applies alpha and beta once.  No host synchronisation.
  const bool strict = bx && sh.pub;
  p.slab = nullptr;
  if (p.ksplit > 1 || strict) {
    if (!workspace || workspace_bytes < pl.slab_bytes) return VIVIT_E_WORKSPACE;
    p.slab = ws_at<float>(workspace, pl.slab_off);
  }
  uint4 *apieces = nullptr;
  int *flag = nullptr;
  if (bx) {   // the pieces of A behind the slab, the range flag behind them
    if (!workspace || workspace_bytes < pl.bytes) return VIVIT_E_WORKSPACE;
    apieces = ws_at<uint4>(workspace, pl.a_off);
    if (strict) flag = ws_at<int>(workspace, pl.flags_off);
  }
  if (!gemm64_attrs()) return VIVIT_E_LAUNCH;
  if (flag && hipMemsetAsync(flag, 0, sizeof(int), stream) != hipSuccess) return VIVIT_E_LAUNCH;
  p.tiles_m = 1;
  p.tiles_n = (int)cdiv(p.N, 256);
  p.syrk = 0;
  p.desc = nullptr;
  dim3 grid((unsigned)p.tiles_n, (unsigned)p.ksplit, 1);
  auto launch_dma = [&](const GemmArgs &q) {
    with_layouts(alay, blay, [&](auto LA, auto LB) { gemm64_dma_kernel<LA, LB><<<grid, 256, GEMM64_LDS_BYTES, stream>>>(q); });
  };
  const unsigned kt = (unsigned)(p.K / BK);
  if (strict) {
    with_layout(alay, [&](auto L) { g64_split_a_kernel<L, true><<<kt, 128, 0, stream>>>(p.A, p.lda, p.M, apieces, flag); });
    with_layout(blay, [&](auto L) { gemm64_bx_kernel<L, true><<<grid, 256, GEMM64X_LDS_BYTES, stream>>>(p, apieces, flag); });
    int st = launch_status();
    if (st != VIVIT_OK) return st;
    GemmArgs f = p;
    f.gate = flag;
    f.gate_mask = tls_bx_gate_mask;
    launch_dma(f);
  } else if (bx) {   // products on the bf16 pipe: split the 64-row operand once, then stream
    with_layout(alay, [&](auto L) { g64_split_a_kernel<L><<<kt, 128, 0, stream>>>(p.A, p.lda, p.M, apieces, nullptr); });
    with_layout(blay, [&](auto L) { gemm64_bx_kernel<L><<<grid, 256, GEMM64X_LDS_BYTES, stream>>>(p, apieces, nullptr); });
  } else {
    launch_dma(p);
  }
  int st = launch_status();
  if (st != VIVIT_OK) return st;
  if (p.slab) {
    launch_gemm_reduce(p.slab, p.C, p.M, p.N, p.ldc, p.ksplit, p.alpha, p.beta, 0, stream);
    st = launch_status();
  }
  return st;
}

} // namespace vivit
