// fp32 GEMM / SYRK on the bf16 matrix pipe ("bf16 x 6"): the fp32 MFMA (v_mfma_f32_32x32x2_f32) retires 64 flop per
// SIMD-cycle, v_mfma_f32_32x32x16_bf16 1024.  Every fp32 operand is split EXACTLY into three bf16 pieces,
//   a = a_hi + a_mid + a_lo    (a_hi = bf16(a), a_mid = bf16(a - a_hi), a_lo = bf16(a - a_hi - a_mid); 3 x 8 = 24
//                               significand bits, the two subtractions are exact in fp32),
// and a product a b is the sum of the partial products whose weight is at least 2^-16 of it,
//   hi hi + hi mid + mid hi + hi lo + lo hi + mid mid          (each EXACT in the MFMA: 8 x 8 -> 16 bits, fp32 accumulate);
// the three dropped ones (mid lo, lo mid, lo lo) are below 2^-24 |a b|, i.e. below the rounding error the fp32 MFMA
// commits on the product itself.  Six bf16 MFMAs replace eight fp32 MFMAs per 16 k: 2.67x the matrix-pipe rate for the
// same accumulation arithmetic (fp32 accumulators, the same two-level flush into C, tile map and epilogues of
// gemm256_kernel).  Operands are K-contiguous (LAY_K) on both sides: the Gram SYRK and the NT products.
// (The six-product kernel issues them as THREE v_mfma_f32_16x16x32_bf16 per 16 x 16 tile -- lo hi + hi lo, mid mid + mid hi,
// hi mid + hi hi, each instruction summing two partial products over the same 16 k --: same pipe rate, same exactness argument,
// a higher clock under the power limit; see gemm256_bx_kernel.)
//
// Two kernels: bx_split_kernel writes the three pieces of a column chunk of an operand as bf16 matrices (HBM-bound:
// 4 B read + 6 B written per element, 1-2 % of the product's time); gemm256_bx_kernel is then a pure bf16 GEMM on the
// data path of gemm256_kernel: global -> LDS DMA, three stages, requested two K tiles ahead, no VALU work per
// element at all.  (A first version split inside the GEMM, global -> registers -> 3 bf16 -> LDS: hipcc would not
// overlap the ~300 VALU operations per K tile with the 96 MFMAs of a one-wave-per-SIMD kernel, and kept the
// prefetched values in scratch: 207 TFLOP/s-equivalent at best against 149 for the fp32 MFMA kernel.)
// LDS: per stage and operand 3 pieces x 8 blocks of 1 KB; block b = rows 32 b .. 32 b + 31 as [k half][32 rows][8 bf16]:
// ONE DMA instruction fills a block (lane -> (row lane % 32, half lane / 32), 16 B each), ONE conflict-free
// ds_read_b128 per lane reads an MFMA operand (row r, the 8 k of half h).  A and B use the same assignment of k to
// (half, slot), which is all the MFMA needs (the sum over k is order independent).
#include "gemm_plan.h"

namespace vivit {

typedef const unsigned short __attribute__((address_space(1))) *gcptr16;
constexpr int BX_PIECE = 8 * 1024;               // bytes of one piece of one operand tile (256 rows x 16 k bf16)
constexpr int BX_OPER = 3 * BX_PIECE;            // 24 KB
constexpr int BX_STAGE = 2 * BX_OPER;            // A and B: 48 KB
// three stages = 144 KB: one workgroup per CU (two would need 288 KB; a CU has 160 KB)
constexpr int GEMM256BX_LDS_BYTES = 3 * BX_STAGE;

// Pieces of the column chunk [k0, k0 + kc) of A (rows x ., row stride lda) in the BLOCKED layout the GEMM's DMA wants:
//   P[pc][k tile kt (16 k)][row block rb (32 rows)] = 1 KB = [k half][32 rows][8 bf16]
// so that one global_load_lds instruction of the GEMM reads 1 KB of consecutive bytes (a row-major piece matrix made
// every lane fetch 16 bytes from a different cache line: 4x the L2 traffic, the product ran at 105 TFLOP/s-equivalent).
// One workgroup converts 32 rows x 64 k: coalesced 32-byte reads per lane, transposition through LDS, 1 KB bursts out.
// Rows beyond `rows` are written as zeros.  kc % 16 == 0; grid.x = row blocks, grid.y = groups of 4 k tiles.
//
// Range gate: the three-way split is exact for finite values whose smallest piece is a NORMAL bf16 number.  A value that
// is non-finite or rounds to +-inf as bf16 (|a| >= 0x7F7F8000 = 3.3962e38) sets bit 0 of *flag, a non-zero value below
// 2^-100 (its `lo` piece could fall below 2^-126) sets bit 1; the bf16-pipe product of a flagged chunk returns at once
// and the fp32 MFMA kernel, launched behind it on the same columns, computes the chunk instead (BX_GATE below).
template <int LAY>
__global__ __launch_bounds__(256) void bx_split_kernel(const float *__restrict__ A, int64_t rows, int64_t lda, int64_t k0,
                                                       int64_t kc, unsigned short *__restrict__ P, int64_t piece_stride,
                                                       int64_t nrb, int *__restrict__ flag) {
  __shared__ __attribute__((aligned(16))) unsigned char sp[3][4][1024];
  __shared__ float tr[LAY == LAY_M ? 64 * 33 : 1];
  const int tid = threadIdx.x;
  const int64_t rb = blockIdx.x;
  const int64_t kt0 = (int64_t)blockIdx.y * 4;
  const int64_t nkt = kc >> 4;
  const int rl = tid >> 3, seg = tid & 7;           // row in the block, 8-float segment of the 64 k
  float v[8];
  if (LAY == LAY_K) {
    const int64_t row = rb * 32 + rl;
    const int64_t k = kt0 * 16 + seg * 8;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (row < rows && k < kc) {
      const float4 *src = reinterpret_cast<const float4 *>(A + row * lda + k0 + k);
      v0 = src[0];
      v1 = src[1];
    }
    v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
  } else {
    // k-major source X[k][row]: coalesced reads along the rows (8 rows per thread), transposition through LDS
    const int kk = tid >> 2, rs = tid & 3;
    const int64_t k = kt0 * 16 + kk, row = rb * 32 + rs * 8;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (k < kc && row + 8 <= rows) {
      const float4 *src = reinterpret_cast<const float4 *>(A + (k0 + k) * lda + row);
      v0 = src[0];
      v1 = src[1];
    } else if (k < kc) {
      float e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = row + j < rows ? A[(k0 + k) * lda + row + j] : 0.f;
      v0 = make_float4(e[0], e[1], e[2], e[3]);
      v1 = make_float4(e[4], e[5], e[6], e[7]);
    }
    float *d = tr + kk * 33 + rs * 8;
    d[0] = v0.x; d[1] = v0.y; d[2] = v0.z; d[3] = v0.w; d[4] = v1.x; d[5] = v1.y; d[6] = v1.z; d[7] = v1.w;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tr[(seg * 8 + j) * 33 + rl];
  }
  {
    int bad = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = fabsf(v[j]);
      bad |= !(x < __uint_as_float(0x7F7F8000u)) ? BX_GATE_RANGE : 0;           // inf, NaN, rounds to inf as bf16
      bad |= (x < __uint_as_float(0x0D800000u) && x != 0.f) ? BX_GATE_TINY : 0;  // 0 < |a| < 2^-100
    }
    const unsigned long long m0 = __builtin_amdgcn_ballot_w64((bad & BX_GATE_RANGE) != 0);
    const unsigned long long m1 = __builtin_amdgcn_ballot_w64((bad & BX_GATE_TINY) != 0);
    if ((m0 | m1) != 0 && (tid & 63) == 0) atomicOr(flag, (m0 ? BX_GATE_RANGE : 0) | (m1 ? BX_GATE_TINY : 0));  // rare
  }
  {
    unsigned h[4], m[4], l[4];
    bx_split2(v[0], v[1], h[0], m[0], l[0]);
    bx_split2(v[2], v[3], h[1], m[1], l[1]);
    bx_split2(v[4], v[5], h[2], m[2], l[2]);
    bx_split2(v[6], v[7], h[3], m[3], l[3]);
    const int kt = seg >> 1, half = seg & 1;
    const int o = half * 512 + rl * 16;
    *reinterpret_cast<uint4 *>(&sp[0][kt][o]) = make_uint4(h[0], h[1], h[2], h[3]);
    *reinterpret_cast<uint4 *>(&sp[1][kt][o]) = make_uint4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<uint4 *>(&sp[2][kt][o]) = make_uint4(l[0], l[1], l[2], l[3]);
  }
  __syncthreads();
  // 12 KB out: thread t moves 16 bytes of (piece, k tile) = (j / 4, j % 4) for j = t / 64 + 4 i
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = (tid >> 6) + 4 * i, pc = j >> 2, kt = j & 3;
    if (kt0 + kt < nkt) {
      unsigned char *dst = reinterpret_cast<unsigned char *>(P + pc * piece_stride) + ((kt0 + kt) * nrb + rb) * 1024 + (tid & 63) * 16;
      *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(&sp[pc][kt][(tid & 63) * 16]);
    }
  }
}

// The partial products of a split product are accumulated in a fixed order of (A piece, B piece); element (r, c) and
// element (c, r) of a DIAGONAL tile of a SYRK see that order with the roles swapped and may differ in the last bit
// (off-diagonal tiles are mirrored exactly).  The lower triangle of every diagonal 256 x 256 tile is copied up.
__global__ __launch_bounds__(256) void bx_sym_diag_kernel(float *__restrict__ C, int64_t n, int64_t ldc) {
  const int64_t base = (int64_t)blockIdx.x * B2;
  for (int idx = threadIdx.x; idx < B2 * B2; idx += 256) {
    const int64_t rr = base + idx / B2, cc = base + idx % B2;
    if (rr < n && cc < n && cc > rr) C[rr * ldc + cc] = C[cc * ldc + rr];
  }
}

struct GemmBxArgs {
  const unsigned short *A, *B;   // piece 0 of each operand (blocked layout of bx_split_kernel); pieces 1, 2 at + strideA / strideB elements
  int64_t strideA, strideB;
  int64_t nrbA, nrbB;            // 32-row blocks per k tile of each operand
  float *C;
  int64_t M, N, K, ldc;          // K = contraction length of THIS launch (multiple of 16)
  float alpha, beta;
  int tiles_m, tiles_n, syrk, sbw;
  // split-K over blockIdx.y for small outputs with a deep contraction (kt_split > 0): split z takes k tiles
  // [z kt_split, (z + 1) kt_split) and writes its partial tile (alpha = 1, beta = 0) to slab[z][M][N]
  float *slab;
  int kt_split;
  const int *gate;               // range flag of this chunk (bx_split_kernel); the kernel returns when *gate & gate_mask
  int gate_mask;
  // K tiles accumulated in one MFMA chain before the sum is added into C with a VALU add (see bx_flush_tiles);
  // flush_diag: the same for the diagonal tiles of a SYRK (sums of squares: every product has the same sign)
  int flush_tiles, flush_diag;
};

#if defined(BX_STAMP)
// Diagnostic build only (scripts/probe/bx_clock.py; never in the product library): every workgroup stamps s_memtime (core
// clock) and s_memrealtime (100 MHz) around its K loop into a buffer of its own -- the in-kernel clock the chip holds
// under this kernel's load is d(memtime) / d(memrealtime) x 100 MHz (MI355X_MICROARCH.md, "DVFS give-back" item 6).
__device__ unsigned long long *g_bx_stamp = nullptr;
__device__ unsigned int g_bx_stamp_cap = 0;
#endif

#include "bx_kloop_asm.inc"

// ASM (default since round 6): the steady part of the K loop runs as ONE hand-scheduled inline-asm block (bx_kloop_asm.inc,
// generated by scripts/gen_bx_kloop.py: fixed register map, every memory instruction placed between the MFMAs by hand);
// prologue, the last tiles of a pass, the chain flushes and the epilogues stay the C++ below, which is also the reference
// implementation (ASM = false, VIVIT_BX_ASM=0).  Same instructions in the same order per accumulator: bit-identical
// results (tests/test_bx_asm_gpu.py).
//
// MFMA shape (second half of round 6).  The six-product kernel computes on v_mfma_f32_16x16x32_bf16, two partial products fused
// along the instruction's K = 32 (see "S16" at the fragment loads): the same flops as six v_mfma_f32_32x32x16_bf16 per 32 x 32
// block, in twice as many instructions of half the length.  It needs MORE core cycles per K tile (3072 of them are MFMA cycles
// either way; in-kernel stamps, profiles/r06_bx16_timeline*.log: 3440-3470 against 3250-3280, 40 fragment reads instead of 27)
// -- and runs faster, because the kernel is power-limited and the chip holds a higher clock on this shape (2.0-2.1 against 1.8 GHz
// on half-zero data, 1.8 against 1.7 on N(0,1); MI355X_MICROARCH.md, DVFS give-back item 7): the headline-shaped SYRK takes
// 875 / 780 ms (N(0,1) / half zeros) against 921 / 819 ms on the same box (profiles/r06_syrk_ab_s16.log; the 32 x 32 x 16 form
// with its own asm block was a build option until it was removed after these measurements).
//
// What the blocks do differently from the compiler's schedule, in core cycles per K tile (32 x 32 x 16 form, where they were
// measured one by one; profiles/r06_bx_attribution*.log; the C++ loop: 3525):
//   * the twelve global -> LDS requests take a scalar base + ONE 32-bit lane offset instead of twelve 64-bit per-lane
//     pointers (global_load_lds_dwordx4 v, s[..]): the requests cost ~30 cycles per tile instead of ~290 -- it is the address
//     registers of a request, not its issue slot, that hold up the SIMD (eight waves, two per SIMD, did not hide it: same 3500);
//   * never more than two ds_read_b128 per 32-cycle MFMA gap (a third one by every wave saturates the LDS array for that gap: ~100)
//     -- one per 16-cycle gap in the 16 x 16 x 32 form;
//   * one request per gap over the second half of the tile, never beside fragment reads (all in the last row: + 190; one per gap
//     right behind the barrier, 16 x 16 x 32 form: + 370);
//   * an accumulator comes back every 8th instruction at the earliest (16 x 16 x 32 form: every 2nd costs ~ 25);
//   * three tiles per trip with the stage registers renamed instead of rotated (- 45); M0 written one gap ahead of its request
//     instead of s_nop in front of it (- 30).
//   32 x 32 x 16 form: 3283 (no barrier: 3235; no requests: 3253; neither: 3226).  16 x 16 x 32 form: 3440 (no barrier: 3400; no
//   requests: 3380; neither: 3350).  Fewer cycles come back as time only in part (DVFS give-back): - 7 % cycles were - 3.8 % time.
template <int NPROD, bool ASM = false>
__global__ __launch_bounds__(256, 1) void gemm256_bx_kernel(GemmBxArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_bx[];
  constexpr bool S16 = NPROD == 6;   // the MFMA shape (accumulator layout below)
#if defined(BX_STAMP) && BX_STAMP == 2   // timeline build (scripts/probe/bx_timeline.py): 8 words per workgroup
  const unsigned long long stamp_entry = __builtin_amdgcn_s_memrealtime();
#endif
  if (p.gate && (*p.gate & p.gate_mask) != 0) return;  // the fp32 MFMA kernel takes this chunk
  int ti, tj, zsplit;
  {
    const int nt_all = (int)(p.K / BK);
    if (!map_tile_z(p.syrk, p.sbw, p.tiles_m, p.tiles_n, p.kt_split > 0 ? (nt_all + p.kt_split - 1) / p.kt_split : 1, ti, tj, zsplit)) return;
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  // Accumulator layout.  The six-product kernel computes on v_mfma_f32_16x16x32_bf16 (S16): the 32 x 32 block acc[i][j] is four
  // 16 x 16 tiles (tr, tc) in registers 4 (2 tr + tc) .. + 3, lane l holding rows 4 (l / 16) .. + 3 of column l % 16 of each.
  // (With the B fragment as the instruction's first operand a lane would hold row l % 16 and the four CONSECUTIVE columns
  // 4 (l / 16) .. + 3 instead -- bit-identical sums, one 16-byte access per tile in the flush and a mirrored store that is
  // coalesced as it stands; measured SLOWER on the same box, profiles/r06_syrk_ab_transposed.log: headline-shaped SYRK 875 / 783
  // against 866 / 772 ms, rank-1024 update of 20480^2 4.18 against 3.94 ms.)
  // The other kernels on v_mfma_f32_32x32x16_bf16 (register e = rows (e & 3) + 8 (e >> 2) + 4 (l / 32) of column l % 32).
  const int r16 = lane & 15, kb = lane >> 4;
  // element e of a block: (row, column) = (lrow + erc(e), lcol + ecc(e)), a lane part and a part that is a constant per register
  const int lrow = S16 ? 4 * kb : 4 * h, lcol = S16 ? r16 : r;
  auto erc = [](int e) __attribute__((always_inline)) -> int { return S16 ? 16 * (e >> 3) + (e & 3) : (e & 3) + 8 * (e >> 2); };
  auto ecc = [](int e) __attribute__((always_inline)) -> int { return S16 ? 16 * ((e >> 2) & 1) : 0; };
  auto erow = [&](int e) __attribute__((always_inline)) -> int { return lrow + erc(e); };
  auto ecol = [&](int e) __attribute__((always_inline)) -> int { return lcol + ecc(e); };
  const int64_t row0 = (int64_t)ti * B2, col0 = (int64_t)tj * B2;
  int nt = (int)(p.K / BK);
  int64_t kt0 = 0;
  if (p.kt_split > 0) {
    kt0 = (int64_t)zsplit * p.kt_split;
    nt = nt - (int)kt0 < p.kt_split ? nt - (int)kt0 : p.kt_split;
  }

  // (S16: see the accumulator layout above -- the 32 x 32 block is four separate 4-register accumulators)
  constexpr int NQ = S16 ? 4 : 1, QW = 16 / NQ;
  typedef typename std::conditional<S16, f32x4, f32x16>::type AccV;
  AccV acc[4][4][NQ];
  auto aget = [&](int i, int j, int e) __attribute__((always_inline)) -> float { return acc[i][j][e / QW][e % QW]; };
  auto aset = [&](int i, int j, int e, float v) __attribute__((always_inline)) { acc[i][j][e / QW][e % QW] = v; };
  auto clear_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) aset(i, j, e, 0.f);
  };
  clear_acc();

  gptr Cout = p.kt_split > 0 ? (gptr)p.slab + (int64_t)zsplit * p.M * p.N : (gptr)p.C;
  const int64_t ldc = p.kt_split > 0 ? p.N : p.ldc;
  const float alpha_ = p.kt_split > 0 ? 1.f : p.alpha, beta_ = p.kt_split > 0 ? 0.f : p.beta;
  const bool full_tile = row0 + B2 <= p.M && col0 + B2 <= p.N;
  // C <- C' + alpha * acc with C' = beta * C on the first flush and C afterwards; acc <- final value.  The loads go to
  // the L2 (sc1): earlier chains of this tile were added into C by L2 atomics (flush_mid), which the L1 does not see.
  auto ld_l2 = [](gptr q) __attribute__((always_inline)) -> float {
    return __hip_atomic_load((const float *)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto flush_to_c = [&](bool first) __attribute__((always_inline)) {
    const float beta = first ? beta_ : 1.f;
    int opaque = 0;
    __asm__ volatile("" : "+v"(opaque));  // keeps the 256 output addresses out of LICM's reach (see gemm256_kernel)
    // One row of four 32 x 32 blocks at a time: 64 loads in flight, then as many stores (block by block - 16 loads, wait, 16
    // stores - the read-modify-write cost ~40 us per 256 x 256 tile: half of a K = 512 update's time; two rows in flight together
    // took the same time, four spilled: + 4 %)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __asm__ volatile("" ::: "memory");
      const int64_t rbase = row0 + wm * 128 + i * 32 + lrow + opaque;
      if (full_tile) {
        float old[4][16];
        if (beta != 0.f) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            gptr cbase = Cout + rbase * ldc + (col0 + wn * 128 + j * 32 + lcol);
#pragma unroll
            for (int e = 0; e < 16; ++e) old[j][e] = ld_l2(cbase + (int64_t)erc(e) * ldc + ecc(e));
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          gptr cbase = Cout + rbase * ldc + (col0 + wn * 128 + j * 32 + lcol);
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            float v = alpha_ * aget(i, j, e);
            if (beta != 0.f) v += beta * old[j][e];
            cbase[(int64_t)erc(e) * ldc + ecc(e)] = v;
            aset(i, j, e, v);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int64_t row = rbase + erc(e), col = col0 + wn * 128 + j * 32 + ecol(e);
            float v = alpha_ * aget(i, j, e);
            if (row < p.M && col < p.N) {
              gptr c = Cout + row * ldc + col;
              if (beta != 0.f) v += beta * ld_l2(c);
              *c = v;
            }
            aset(i, j, e, v);
          }
        }
      }
    }
  };

  // The flush INSIDE the K loop (end of an accumulation chain): C += alpha * acc with no-return fp32 atomics executed in
  // the L2 (global_atomic_add_f32: a correctly rounded fp32 add, exactly the VALU add of the other flushes), or a plain
  // store when this is the tile's first flush and beta = 0 (the host passes only beta = 0 or 1 and scales C beforehand
  // otherwise).  This workgroup is the only writer of its tile and a wave's memory operations on one address stay in
  // order, so the result is the same deterministic sum -- but nothing is loaded and nothing is waited for: the
  // read-modify-write happens where the data lives while the next chain's MFMAs run, and the global -> LDS pipeline is
  // not restarted (that alone cost 34 us per chain).  (Out of line -- accumulators copied to a private array, a noinline
  // function issuing the atomics -- the flush cost 140 us: 512 KB of scratch traffic per workgroup.)
  auto flush_mid = [&](bool store) __attribute__((always_inline)) {
    int opaque = 0;
    __asm__ volatile("" : "+v"(opaque));
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t rb = row0 + wm * 128 + i * 32 + lrow + opaque, cb0 = col0 + wn * 128 + j * 32 + lcol;
        gptr cb = Cout + rb * ldc + cb0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int dr = erc(e), dc = ecc(e);
          if (full_tile || (rb + dr < p.M && cb0 + dc < p.N)) {
            if (store) cb[(int64_t)dr * ldc + dc] = alpha_ * aget(i, j, e);
            else __builtin_amdgcn_global_atomic_fadd_f32(cb + (int64_t)dr * ldc + dc, alpha_ * aget(i, j, e));
          }
        }
      }
  };

  // ---- DMA sources: wave w fills blocks w and w + 4 of every piece of both operands (12 instructions per K tile),
  // each instruction 1 KB of consecutive global bytes (blocked piece layout).  Row blocks beyond the matrix read the
  // last block (their outputs are never stored).  The pointers advance by one k tile per request.
  gcptr16 srcA[2], srcB[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int blk = wave + 4 * u;
    int64_t ba = row0 / 32 + blk, bb = col0 / 32 + blk;   // 32-row block of the operand (clamped: never stored rows)
    ba = ba < p.nrbA ? ba : p.nrbA - 1;
    bb = bb < p.nrbB ? bb : p.nrbB - 1;
    srcA[u] = (gcptr16)p.A + (kt0 * p.nrbA + ba) * 512 + 8 * lane;          // 1 KB block = 512 bf16; lane -> its 16 bytes
    srcB[u] = (gcptr16)p.B + (kt0 * p.nrbB + bb) * 512 + 8 * lane;
  }
  const int64_t stepA = p.nrbA * 512, stepB = p.nrbB * 512;  // one k tile further
  // (In the C++ loop -- the reference implementation, ASM = false, and the tiles around the asm block -- the addresses stay per-lane
  // 64-bit registers, advanced by one v_lshl_add_u64 per request.  The asm block takes the scalar form -- block address in an SGPR
  // pair advanced by s_add_u32 / s_addc_u32, one shared 32-bit lane offset, `global_load_lds_dwordx4 v, s[..]` -- which in this
  // C++ loop measured 1.5-4 % SLOWER on the SYRK shape (225.1 / 248.8 against 227-234 / 252.5 TFLOP/s, round 5,
  // scripts/probe/syrk_ab.sh).)
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem_bx +
                                                       (unsigned)(wave * 1024));
  auto dma16b = [&](gcptr16 src, unsigned lds_byte_addr) __attribute__((always_inline)) {
    __asm__ volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_byte_addr), "v"(src) : "memory");
  };
  // part q of the 12 requests of one K tile: q = 0..3 -> (block u = q / 2, operand q % 2), three pieces each
  auto issue_part = [&](int st, int q) __attribute__((always_inline)) {
    const int u = q >> 1;
    if ((q & 1) == 0) {
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
        dma16b(srcA[u] + pc * p.strideA, lds0 + (unsigned)(st * BX_STAGE + pc * BX_PIECE + 4 * u * 1024));
      srcA[u] += stepA;
    } else {
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
        dma16b(srcB[u] + pc * p.strideB, lds0 + (unsigned)(st * BX_STAGE + BX_OPER + pc * BX_PIECE + 4 * u * 1024));
      srcB[u] += stepB;
    }
  };
  auto issue = [&](int st) __attribute__((always_inline)) {  // the next not yet requested K tile into stage st
#pragma unroll
    for (int q = 0; q < 4; ++q) issue_part(st, q);
  };
  // ---- one K tile of 16: 16 output tiles x NPROD bf16 MFMAs per wave; the smallest partial products go in first.
  // The B pieces of the wave's four column tiles stay in registers for the tile (48), the A pieces stream per row tile.
  // S16: one v_mfma_f32_16x16x32_bf16 adds TWO partial products -- its K = 32 is the tile's 16 k twice, first with one pair of
  // pieces and then with another.  Lane l supplies row (column) l % 16 and k block l / 16 of the instruction's 32: blocks 0, 1 are
  // the two 8-k halves of the first piece, blocks 2, 3 those of the second, so a fragment is still ONE ds_read_b128 with the piece
  // picked per lane.  Three instructions per 16 x 16 tile and K tile, smallest terms first:
  //   [a2 | a0] x [b0 | b2]  ->  lo hi + hi lo        [a1 | a1] x [b1 | b0]  ->  mid mid + mid hi        [a0 | a0] x [b1 | b0]  ->  hi mid + hi hi
  // i.e. three A fragments per 16 rows and two B fragments per 16 columns (the B fragments of the wave's 128 columns stay in
  // registers for the tile: 64).  40 fragment reads per wave and K tile against 28 for the 32 x 32 x 16 shape, 192 instructions of
  // 8 passes against 96 of 16 -- same flops, but the chip holds a ~12 % higher clock on this shape (profiles/r06_bx_mfma16_timing.log).
  const unsigned fofsA = S16 ? (unsigned)((wm * 4) * 1024 + (kb & 1) * 512 + r16 * 16) : (unsigned)((wm * 4) * 1024 + h * 512 + r * 16);
  const unsigned fofsB = S16 ? (unsigned)((wn * 4) * 1024 + (kb & 1) * 512 + r16 * 16) : (unsigned)((wn * 4) * 1024 + h * 512 + r * 16);
  constexpr int NCA = 3, NCB = S16 ? 2 : 3, NSUB = S16 ? 2 : 1;   // fragments per 32-row block: NCA (NCB) combinations x NSUB halves
  // byte offset of combination c of A (d of B) inside a stage: the piece this lane reads
  unsigned cofsA[NCA], cofsB[NCB];
  if (S16) {
    cofsA[0] = (unsigned)((kb >> 1 ? 0 : 2) * BX_PIECE) + fofsA;   // [a2 | a0]
    cofsA[1] = (unsigned)(1 * BX_PIECE) + fofsA;                   // [a1 | a1]
    cofsA[2] = fofsA;                                              // [a0 | a0]
    cofsB[0] = (unsigned)(BX_OPER + (kb >> 1 ? 2 : 0) * BX_PIECE) + fofsB;   // [b0 | b2]
    cofsB[1] = (unsigned)(BX_OPER + (kb >> 1 ? 0 : 1) * BX_PIECE) + fofsB;   // [b1 | b0]
  } else {
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
      cofsA[pc] = (unsigned)(pc * BX_PIECE) + fofsA;
      if (pc < NCB) cofsB[pc] = (unsigned)(BX_OPER + pc * BX_PIECE) + fofsB;
    }
  }
  struct FragB {
    bf16x8 v[NCB][4 * NSUB];
  };
  struct FragA {
    bf16x8 v[NCA][NSUB];
  };
  auto load_b_col = [&](int st, int j, FragB &f) __attribute__((always_inline)) {   // the fragments of 32-column block j
    const unsigned char *sS = smem_bx + st * BX_STAGE;
#pragma unroll
    for (int d = 0; d < NCB; ++d)
#pragma unroll
      for (int tc = 0; tc < NSUB; ++tc) f.v[d][NSUB * j + tc] = *reinterpret_cast<const bf16x8 *>(sS + cofsB[d] + j * 1024 + tc * 256);
  };
  auto load_b = [&](int st) __attribute__((always_inline)) -> FragB {
    FragB f;
#pragma unroll
    for (int j = 0; j < 4; ++j) load_b_col(st, j, f);
    return f;
  };
  auto load_a = [&](int st, int i) __attribute__((always_inline)) -> FragA {   // the fragments of 32-row block i
    const unsigned char *sS = smem_bx + st * BX_STAGE;
    FragA f;
#pragma unroll
    for (int c = 0; c < NCA; ++c)
#pragma unroll
      for (int tr = 0; tr < NSUB; ++tr) f.v[c][tr] = *reinterpret_cast<const bf16x8 *>(sS + cofsA[c] + i * 1024 + tr * 256);
    return f;
  };
  auto mfma_row = [&](auto iconst, const FragA &fa, const FragB &fb, auto &&between) __attribute__((always_inline)) {
    constexpr int i = decltype(iconst)::value;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      between(j);
      if constexpr (S16) {
#pragma unroll
        for (int m = 0; m < 3; ++m)   // (the four tiles in turn: consecutive instructions never share an accumulator)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[i][j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa.v[m][t >> 1], fb.v[m == 0 ? 0 : 1][2 * j + (t & 1)], acc[i][j][t], 0, 0, 0);
      } else {
        f32x16 c = acc[i][j][0];
        if (NPROD >= 9) {
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v[2][0], fb.v[2][j], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v[2][0], fb.v[1][j], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v[1][0], fb.v[2][j], c, 0, 0, 0);
        }
        if (NPROD >= 6) {
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v[2][0], fb.v[0][j], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v[0][0], fb.v[2][j], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v[1][0], fb.v[1][j], c, 0, 0, 0);
        }
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v[1][0], fb.v[0][j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v[0][0], fb.v[1][j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v[0][0], fb.v[0][j], c, 0, 0, 0);
        acc[i][j][0] = c;
      }
    }
  };
  using J0 = std::integral_constant<int, 0>;
  using J1 = std::integral_constant<int, 1>;
  using J2 = std::integral_constant<int, 2>;
  using J3 = std::integral_constant<int, 3>;
  // Pipeline (tile t lives in stage t % 3).  The fragment reads of a row tile are issued BEFORE the MFMAs of the
  // previous one, and the first fragments of tile t + 1 during the second half of tile t, so the matrix pipe never
  // waits for LDS.  In the middle of tile t every wave waits for its own share of tile t + 1 (requested one tile ago);
  // the barrier there publishes tile t + 1 and certifies that every wave is completely past tile t - 1, whose stage then
  // receives the requests for tile t + 2.
  // One pipelined pass over all K tiles.  Every `flush_tiles` tiles (rounded to the two-tile trip) an MFMA chain ends:
  // its sum goes into C (flush_mid) and the accumulators restart from zero -- see bx_flush_tiles for why chains are short.
#if defined(BX_STAMP)
  const unsigned long long stamp_c0 = __builtin_amdgcn_s_memtime(), stamp_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  bool first_flush = true;
  const int flush_tiles = (((p.syrk != 0 && ti == tj) ? p.flush_diag : p.flush_tiles) + 1) & ~1;
  const bool mirrored = p.syrk == 1 && ti != tj;   // the mirror store wants the final values in the accumulators
  {
    const int t1 = nt;
    // (tile 1 is requested behind tile 0 BEFORE the wait for tile 0: its latency runs beside tile 0's instead of behind the barrier)
    issue(0);
    if (1 < t1) {
      issue(1);
      __asm__ volatile("s_waitcnt vmcnt(12)" ::: "memory");   // all but the 12 requests of tile 1: tile 0 has landed
    } else {
      __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __asm__ volatile("s_barrier" ::: "memory");
#if defined(BX_STAMP) && BX_STAMP == 2
    const unsigned long long stamp_loop0 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0 && g_bx_stamp && p.syrk == 2 && blockIdx.x < g_bx_stamp_cap) g_bx_stamp[8 * blockIdx.x + 3] = stamp_loop0;
#endif
    // two named fragment sets in ping-pong (tile t uses one and fills the other for tile t + 1)
    FragB fbX = load_b(0), fbY;
    FragA faX = load_a(0, 0), faY;
    int st = 0, t = 0, next_flush = flush_tiles;
    auto tile = [&](const FragB &fb, const FragA &fa, FragB &fbn, FragA &fan) __attribute__((always_inline)) {
      const int st1 = st == 2 ? 0 : st + 1, st2 = st == 0 ? 2 : st - 1;   // stages of tiles t + 1 and t + 2 (= t - 1)
      const int stn = t + 1 < t1 ? st1 : st;                              // (last tile: harmless re-read of its own stage)
      auto nothing = [](int) {};
      FragA fa1 = load_a(st, 1);
      mfma_row(J0{}, fa, fb, nothing);
      FragA fa2 = load_a(st, 2);
      mfma_row(J1{}, fa1, fb, nothing);
      __builtin_amdgcn_sched_barrier(0);
      // own share of tile t + 1 has landed.  The wait is the compiler-VISIBLE builtin on purpose: hipcc cannot see the asm DMA
      // requests, but it does track its own memory operations (accumulator rows it keeps in scratch around a flush, spill
      // reloads in front of the loop); with those pending in its model it put s_waitcnt vmcnt(12/8/4/0) in front of the first
      // MFMAs of every second tile -- where the hardware counter also holds the DMA requests just issued (+ 40 us per 128 K
      // tiles).  Seeing this vmcnt(0) it knows nothing of its own is pending afterwards.
      __asm__ volatile("" ::: "memory");
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      __asm__ volatile("s_barrier" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      FragA fa3 = load_a(st, 3);
      // The 12 requests of tile t + 2 go out three at a time in ROW 3, behind the fragment reads of each column tile -- away
      // from the barrier: a burst right behind it stalls the wave at issue while the matrix pipe runs dry (round 2), and three
      // per column tile of row 2 (rounds 2-4), still within ~800 cycles of the release, cost 3 % of the kernel.  Same-box A/B
      // at n = 40 960, P = 131 072 (scripts/probe/syrk_ab.sh, profiles/r05_syrk_ab*.log), N(0,1) / half-zero data: row 2
      // (rounds 2-4) 225.1 / 246.3 TFLOP/s; two per column tile of row 2 + one per column tile of row 3 231.0 / 254.0; row 3
      // (this) 233.4 / 256.4 (238.3 / 263.6 against 231.8 / 257.2 on a faster box); row 3, one behind every second MFMA
      // 233.2 / 251.0; rows 2 + 3, one behind every fourth MFMA 232.3 / 250.6; row 3 with the wait + barrier moved between rows 2
      // and 3 234.1 / 259.4 against 238.3 / 263.6 on that box.  The requests then have rows 0 and 1 of the next tile (48 MFMAs,
      // ~0.9 us) + what is left of row 3 to land before the mid-tile wait.
      const bool req = t + 2 < t1;
      mfma_row(J2{}, fa2, fb, nothing);
      // first fragments of tile t + 1: the B pieces of column tile j behind the MFMAs of column tile j - 1 of row 3
      {
        mfma_row(J3{}, fa3, fb, [&](int j) __attribute__((always_inline)) {
          load_b_col(stn, j, fbn);
          __builtin_amdgcn_sched_barrier(0);
          if (req) issue_part(st2, j);
          __builtin_amdgcn_sched_barrier(0);
        });
      }
      fan = load_a(stn, 0);
      st = st1;
      ++t;
    };
    while (true) {
      const int tc = next_flush < t1 ? next_flush : t1;
      if constexpr (ASM && NPROD == 6) {
        // every tile of the asm block requests tile t + 2: it runs up to the last two tiles of the pass (the chain ends of this
        // loop stay where they are)
        // (a whole number of the block's trips AND of this loop's two-tile trips)
        int na = (tc < t1 - 2 ? tc : t1 - 2) - t;
        na -= na % (2 * BX_KLOOP_ASM_UNROLL);
        if (na > 0) {
          const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem_bx;
          const int64_t strideA_b = 2 * p.strideA, strideB_b = 2 * p.strideB, stepA_b = 2 * stepA, stepB_b = 2 * stepB;
          __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the fragment sets of the C++ loop are not carried into the block)
          // the block names its accumulators: acc[i][j][q] is pinned to a[16 (4 i + j) + 4 q .. + 3]
          __asm__ volatile(BX_KLOOP_ASM_TEXT
                           : BX_KLOOP_ASM_ACC(acc)
                           : "v"(lds_base + cofsA[0]), "v"(lds_base + cofsA[1]), "v"(lds_base + cofsA[2]), "v"(lds_base + cofsB[0]),
                             "v"(lds_base + cofsB[1]), "v"(srcA[0]), "v"(srcA[1]), "v"(srcB[0]), "v"(srcB[1]), "s"(strideA_b), "s"(strideB_b),
                             "s"(stepA_b), "s"(stepB_b), "s"(lds0), "s"(st), "s"(na), "s"(0)
                           : BX_KLOOP_ASM_CLOBBERS);
          // the block leaves the request pointers na tiles further and the stage of the new tile t: redo both here (cheap,
          // and the operands above stay plain inputs -- 16 read-write accumulator operands already count twice)
          srcA[0] += (int64_t)na * stepA; srcA[1] += (int64_t)na * stepA;
          srcB[0] += (int64_t)na * stepB; srcB[1] += (int64_t)na * stepB;
          st = (st + na) % 3;
          t += na;
          fbX = load_b(st);
          faX = load_a(st, 0);
        }
      }
      while (t + 2 <= tc) {  // two tiles per trip, no exit in between (the sets swap roles and are back in place)
        tile(fbX, faX, fbY, faY);
        tile(fbY, faY, fbX, faX);
      }
      if (t + 2 > t1) break;  // at most one tile left: it joins this chain
      // end of a chain; its memory operations drain behind the next tile's MFMAs.  (As a register read-modify-write like the last
      // flush: the same within 2 % on split-K Gram matrices and on a five-chain product, profiles/r06_splitk_compact.log.)
      flush_mid(first_flush && beta_ == 0.f);
      first_flush = false;
      clear_acc();
      next_flush += flush_tiles;
      // the fragments of tile t are read again (nothing but the accumulators is carried across the flush)
      __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      fbX = load_b(st);
      faX = load_a(st, 0);
    }
    if (t < t1) tile(fbX, faX, fbY, faY);
  }
#if defined(BX_STAMP)
#if BX_STAMP == 2   // (the launches that add a chunk into the lower tiles without mirroring: all but the last of a Gram SYRK)
  if (tid == 0 && g_bx_stamp && p.syrk == 2 && blockIdx.x < g_bx_stamp_cap) {
    int hwid, xcc;
    __asm__ volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    __asm__ volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    unsigned long long *w = g_bx_stamp + 8 * blockIdx.x;
    w[0] = __builtin_amdgcn_s_memtime() - stamp_c0;
    w[1] = __builtin_amdgcn_s_memrealtime() - stamp_r0;
    w[2] = stamp_entry;
    w[4] = __builtin_amdgcn_s_memrealtime();   // end of the K loop
    w[6] = ((unsigned long long)(unsigned)xcc << 32) | (unsigned)hwid;
  }
#else
  if (tid == 0 && g_bx_stamp && blockIdx.y == 0 && blockIdx.x < g_bx_stamp_cap) {
    g_bx_stamp[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - stamp_c0;
    g_bx_stamp[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - stamp_r0;
  }
#endif
#endif
  // The last flush: the register read-modify-write, which leaves the final values in the accumulators for the mirror store below.
  // Two alternatives measured slower on the same box (headline-shaped SYRK on N(0,1) / half-zero data; rank-1024 update of 20480^2):
  //   * an LDS-DMA flush that fetched the old values of C into the dead operand stages: 893 / 801 ms, 4.47 ms (mirrored tiles only:
  //     916 / 807 ms, 5.04 ms) against 867 / 773 ms, 3.97 ms.  Inside it hipcc reloaded spilled lane constants from scratch and
  //     waited for them with vmcnt(0), which also waited for every old-value request in flight (profiles/r06_syrk_ab_flush.log);
  //   * no-return L2 atomics where nothing needs the final values: 865 / 759 against 843 / 744 ms, 4.62 against 3.84 ms -- the 1024
  //     atomic instructions of a tile take 43 us to issue against 18 us for the read-modify-write (profiles/r06_syrk_ab_atomic.log).
  flush_to_c(first_flush);

  if (mirrored) {
    __syncthreads();
    float *ts = reinterpret_cast<float *>(smem_bx) + wave * (32 * 33);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
        for (int e = 0; e < 16; ++e) ts[ecol(e) * 33 + erow(e)] = aget(i, j, e);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int64_t mrow0 = col0 + wn * 128 + j * 32;
        const int64_t mcol = row0 + wm * 128 + i * 32 + r;
#pragma unroll
        for (int rr = 0; rr < 32; rr += 2) {
          const int64_t mrow = mrow0 + rr + h;
          if (mrow < p.N && mcol < p.M) {
            gptr c = (gptr)p.C + mrow * p.ldc + mcol;
            *c = ts[(rr + h) * 33 + r];
          }
        }
      }
  }
#if defined(BX_STAMP) && BX_STAMP == 2
  if (tid == 0 && g_bx_stamp && p.syrk == 2 && blockIdx.x < g_bx_stamp_cap) g_bx_stamp[8 * blockIdx.x + 7] = __builtin_amdgcn_s_memrealtime();   // flush issued
  __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's flush is in memory
  __syncthreads();
  if (tid == 0 && g_bx_stamp && p.syrk == 2 && blockIdx.x < g_bx_stamp_cap) g_bx_stamp[8 * blockIdx.x + 5] = __builtin_amdgcn_s_memrealtime();
#endif
}

// hipFuncAttributeMaxDynamicSharedMemorySize of gemm256_bx_kernel, once per device
static bool tile256_bx_attrs() {
  static unsigned long long attr_done = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (attr_done & (1ull << (dev & 63))) return true;
  const struct { const void *fn; int bytes; } kernels[] = {
      {reinterpret_cast<const void *>(gemm256_bx_kernel<3>), GEMM256BX_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm256_bx_kernel<6>), GEMM256BX_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm256_bx_kernel<9>), GEMM256BX_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm256_bx_kernel<6, true>), GEMM256BX_LDS_BYTES}};
  for (const auto &k : kernels)
    if (!ensure_dynamic_lds(k.fn, k.bytes, attr_done)) return false;
  attr_done |= 1ull << (dev & 63);
  return true;
}

// ---- the bf16 pipe of the 256 tile (Tile256Bx, BxSplitK)
// Length of one MFMA accumulation chain of the bf16-pipe kernel, in K tiles.  v_mfma_f32_32x32x16_bf16 is NOT a chain
// of correctly rounded fmas: it adds the accumulator and two 8-product group sums after aligning them to the largest
// exponent with about one guard bit, and what is shifted out is TRUNCATED (scripts/probe/mfma_round.hip: c = 1 plus
// sixteen products of 3/64 ulp returns 1; one product of 0.51 ulp rounds up correctly).  Once the accumulator is more
// than ~2^6 times a group sum (chains beyond ~512 k) the low bits of every group sum are cut off towards zero: noise of
// twice the fp32 chain's rounding for sums of random signs, and a BIAS for sums of equal signs -- the diagonal of a Gram
// matrix, entries of correlated rows.  Measured on n = 5120, K = 401 408 (independent N(0,1) rows), chain length ->
// off-diagonal error per term of the random walk / mean relative error of the diagonal:
//     8192 -> 3.2e-6 / -2.5e-6     4096 -> 2.3e-6 / -2.0e-6     2048 -> 1.7e-6 / -1.3e-6     1024 -> 1.2e-6 / -5.5e-7
//      512 -> 9.8e-7 / -6e-8       fp32 MFMA kernel (chains of 8192, correctly rounded): 1.6e-6 / -3.2e-7
// and what a shorter chain costs at the headline shape (n = 40 960: C is 6.7 GB, every flush is HBM traffic that
// competes with the operand panels for the L2 / Infinity Cache): 8192 -> 4096: + 2 %, -> 2048: + 6 %, -> 1024: + 10 %;
// diagonal tiles at 512: + 1-2 % per launch, + 5 % at the headline shape (140 ms).  Default: 4096 k (1.4 x the fp32 MFMA
// kernel's random-sign error) on ALL tiles -- the same-sign sums of a Gram matrix are its diagonal ENTRIES, which the
// public SYRK computes separately in fp64 (syrk_diag_kernel: 16 ms instead of 140) --, 1024 k in the split-K form for
// small outputs (whose yardstick is the 128-tile fp32 kernel with its chains of 2048); the eigensolver's internal
// products on orthogonal factors (random signs, the measured off-diagonal case) keep 8192.  The chain lengths were swept
// in profiles/r03_flush_sweep_n5120.log.
constexpr int bx_flush_tiles = 4096 / BK;
constexpr int bx_flush_diag = 4096 / BK;
constexpr int bx_flush_internal = 8192 / BK;
constexpr int bx_flush_splitk = 1024 / BK;

// columns of an operand split at a time (workspace: 6 bytes per element of the chunk and operand)
// Public products (the Gram SYRKs of the caller) take ONE accumulation chain per launch (round 4): 4096 columns instead of
// 65 536 made the headline Gram build 3-4 % faster on four boxes (2.78-2.80 -> 2.67-2.71 s; 32 768: - 1.5 %, 16 384: - 2.5 %,
// 6144 = a chain and a half: worse than either neighbour, 2048: + 5 %) -- no flush in the middle of a launch, and the
// workgroups of an XCD start every chain together again (they drift apart by whole tiles otherwise, which is what the
// re-fetch traffic of section 4.1b pays for; a start barrier per XCD group on top of that was 1 % slower,
// profiles/r06_syrk_env_sync.log).  The eigensolver's internal products keep 65 536 (their step was 12 ms slower with the
// short chunks).
static int64_t bx_chunk_cols(int64_t K, bool pub) {
  const int64_t kc = pub ? (int64_t)bx_flush_tiles * BK : 65536;
  return K < kc ? K : kc;
}

// bytes of the three bf16 pieces of `cols` columns of the operands (32-row blocks); *b_off: where B's pieces start
static size_t bx_carve_pieces(const GemmShape &sh, int64_t cols, size_t *b_off) {
  const int64_t ra = cdiv(sh.M, 32) * 32, rb = cdiv(sh.N, 32) * 32;
  *b_off = sh.same ? 0 : (size_t)6 * (size_t)cols * (size_t)ra;
  return (size_t)6 * (size_t)cols * (size_t)(sh.same ? ra : ra + rb);
}

// Tile256Bx: the shapes of Tile256, K in chunks of pl.kchunk columns, per chunk the operand pieces (bx_split_kernel) and one
// pure-bf16 launch that accumulates into C.  No split-K: a last round of workgroups that is not full costs less than the
// bf16 pipe's 1.6x speed.  Workspace: the pieces of one chunk + one range flag per chunk (BX_GATE).
// (the public workspace queries run inside a BxStrictScope like the public launches: 1 GB of pieces instead of 16 GB at
// n = 40 960; the eigensolver's own queries and launches see the long chunk)
bool plan_tile256_bx(const GemmShape &sh, GemmPlan &pl) {
  if (gemm_split_mode() == 0 || !plan_tile256(sh, pl)) return false;
  pl.route = GemmRoute::Tile256Bx;
  pl.ksplit = 1;
  pl.kchunk = bx_chunk_cols(sh.K, sh.pub);
  pl.slab_bytes = 0;
  const size_t pieces = bx_carve_pieces(sh, pl.kchunk, &pl.b_off);
  pl.flags_off = align_up(pieces, 256);
  const size_t nch = (size_t)cdiv(sh.K, bx_chunk_cols(sh.K, true));   // (the larger of the two counts)
  // (both + 256 are slack: ws_at does not align the base, and every piece size is a multiple of 6 x 16 x 32 bytes, so the flags
  // sit at align_up(pieces, 256) = pieces and the launch ends 512 bytes before pl.bytes)
  pl.bytes = pieces + 256 + 4 * nch + 256;
  return true;
}

// Splits columns [k0, k0 + kc) of the operands into their bf16 pieces (piece rows of `kcap` columns at pl.a_off / pl.b_off,
// range bits ORed into *flag) and launches the bf16-pipe kernel on them.  The caller has filled what differs between the
// routes: alpha, beta, syrk, sbw, slab, kt_split and the chain lengths of q.
static int launch_bx(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, const GemmArgs &p, void *workspace, int64_t k0,
                     int64_t kc, int64_t kcap, int *flag, GemmBxArgs q, dim3 grid, hipStream_t stream) {
  const int64_t nrbA = cdiv(p.M, 32), nrbB = sh.same ? nrbA : cdiv(p.N, 32);
  const int64_t strideA = nrbA * 32 * kcap, strideB = nrbB * 32 * kcap;
  unsigned short *PA = ws_at<unsigned short>(workspace, pl.a_off), *PB = ws_at<unsigned short>(workspace, pl.b_off);
  const unsigned gy = (unsigned)cdiv(kc / 16, 4);
  with_layout(alay, [&](auto L) {
    bx_split_kernel<L><<<dim3((unsigned)nrbA, gy), 256, 0, stream>>>(p.A, p.M, p.lda, k0, kc, PA, strideA, nrbA, flag);
  });
  if (!sh.same)
    with_layout(blay, [&](auto L) {
      bx_split_kernel<L><<<dim3((unsigned)nrbB, gy), 256, 0, stream>>>(p.B, p.N, p.ldb, k0, kc, PB, strideB, nrbB, flag);
    });
  q.A = PA; q.B = PB; q.strideA = strideA; q.strideB = strideB;
  q.nrbA = nrbA; q.nrbB = nrbB;
  q.C = p.C; q.M = p.M; q.N = p.N; q.K = kc; q.ldc = p.ldc;
  q.tiles_m = p.tiles_m; q.tiles_n = p.tiles_n;
  q.gate = flag; q.gate_mask = tls_bx_gate_mask;
  const int bx = gemm_split_mode();
  if (bx == 6 && bx_asm_enabled())
    gemm256_bx_kernel<6, true><<<grid, 256, GEMM256BX_LDS_BYTES, stream>>>(q);
  else if (bx == 6)
    gemm256_bx_kernel<6><<<grid, 256, GEMM256BX_LDS_BYTES, stream>>>(q);
  else if (bx == 9)
    gemm256_bx_kernel<9><<<grid, 256, GEMM256BX_LDS_BYTES, stream>>>(q);
  else
    gemm256_bx_kernel<3><<<grid, 256, GEMM256BX_LDS_BYTES, stream>>>(q);
  return launch_status();
}

int launch_tile256_bx(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, hipStream_t stream) {
  p.ksplit = 1;
  p.kchunk = cdiv(p.K, BK) * BK;
  p.slab = nullptr;
  p.tiles_m = (int)cdiv(p.M, B2);
  p.tiles_n = (int)cdiv(p.N, B2);
  p.syrk = sh.syrk ? 1 : 0;
  p.desc = nullptr;
  const int64_t nsb = tile_grid(p.tiles_m, p.tiles_n, sh.syrk, &p.sbw);
  if (nsb < 0) return VIVIT_E_UNSUPPORTED;
  if (!tile256_attrs() || !tile256_bx_attrs()) return VIVIT_E_LAUNCH;
  dim3 grid((unsigned)(nsb * 256), 1, 1);
  const bool prof = sh.syrk && p.A == p.B && prof_enabled() && sh.pub;
  if (prof) prof_begin(0, (double)p.M * (double)(p.M + 1) * (double)p.K, stream);
  const int64_t kc_max = pl.kchunk;
  int *flags = ws_at<int>(workspace, pl.flags_off);
  if (hipMemsetAsync(flags, 0, 4 * (size_t)cdiv(p.K, kc_max), stream) != hipSuccess) return VIVIT_E_LAUNCH;
  GemmBxArgs q;
  q.alpha = p.alpha; q.sbw = p.sbw;
  q.slab = nullptr; q.kt_split = 0;
  // the eigensolver's own products (orthogonal factors: sums of random signs, nothing correlated) keep chains of 8192
  q.flush_tiles = sh.pub ? bx_flush_tiles : bx_flush_internal;
  q.flush_diag = sh.pub ? bx_flush_diag : bx_flush_internal;
  float beta0 = p.beta;
  if (beta0 != 0.f && beta0 != 1.f) {   // the in-loop flushes add into C: C <- beta C once, then beta = 1
    launch_scale_c(p.C, p.M, p.N, p.ldc, beta0, stream);
    beta0 = 1.f;
  }
  int st = VIVIT_OK;
  int *flag = flags;
  for (int64_t k0 = 0; k0 < p.K && st == VIVIT_OK; k0 += kc_max, ++flag) {
    const int64_t kc = (p.K - k0) < kc_max ? (p.K - k0) : kc_max;
    q.beta = k0 == 0 ? beta0 : 1.f;
    // SYRK: only the last chunk mirrors the finished lower tiles into the upper triangle (2 = lower tiles, no mirror)
    q.syrk = (p.syrk == 1 && k0 + kc < p.K) ? 2 : p.syrk;
    st = launch_bx(pl, sh, alay, blay, p, workspace, k0, kc, kc_max, flag, q, grid, stream);
    if (st != VIVIT_OK) break;
    GemmArgs f = p;   // the same chunk on the fp32 MFMA kernel
    f.A = p.A + (alay == LAY_K ? k0 : k0 * p.lda);
    f.B = p.B + (blay == LAY_K ? k0 : k0 * p.ldb);
    f.K = kc; f.kchunk = kc;
    f.beta = q.beta; f.syrk = q.syrk;
    st = launch_fp32_standin(alay, blay, f, grid, flag, stream);
  }
  if (st == VIVIT_OK && p.syrk == 1) {
    bx_sym_diag_kernel<<<(unsigned)p.tiles_m, 256, 0, stream>>>(p.C, p.M, p.ldc);
    st = launch_status();
  }
  if (prof) prof_end(0, stream);
  return st;
}

// ---- BxSplitK: bf16-pipe split-K for SMALL outputs with a deep contraction (Gram matrices of small batches: n = 1280,
// P = 4e5 has 15 lower 256-tiles).  The whole operand is split into its three bf16 pieces once (blocked layout: a k
// tile of a 256-row block is 8 KB contiguous per piece, so a K split streams long runs, unlike the 1280 row streams
// 1.6 MB apart of the fp32 operand), one launch with the k tiles divided over blockIdx.y writes partial tiles to a slab,
// and the fixed-order reduce mirrors the lower tiles of a SYRK.
// Workspace: whole-K pieces, the slab, one range flag.
bool plan_bx_splitk(const GemmShape &sh, GemmPlan &pl) {
  const int64_t M = sh.M, N = sh.N, K = sh.K;
  const bool syrk = sh.syrk;
  if (!bx_splitk_enabled() || gemm_split_mode() != 6) return false;
  if (K < 16384 || (K % BK) != 0 || M < 256 || N < 256) return false;
  const int64_t tm = cdiv(M, B2), tn = cdiv(N, B2);
  const int64_t tiles = syrk ? tm * (tm + 1) / 2 : tm * tn;
  if (tiles > 100) return false;                       // enough tiles: the plain bf16-pipe launch fills the chip
  pl = GemmPlan{};
  pl.route = GemmRoute::BxSplitK;
  const size_t pieces = bx_carve_pieces(sh, K, &pl.b_off);
  if (pieces > ((size_t)8 << 30)) return false;        // whole-K pieces: bounded scratch
  const int64_t nt = K / BK;
  int64_t s = 512 / tiles;                             // ~2 rounds of one workgroup per CU
  if (s > nt / 64) s = nt / 64;                        // at least 64 k tiles per split
  if (s < 2) return false;
  {
    // Compact grid (map_tile_z: one super-block, every split's tiles on ONE XCD, splits dealt round-robin to the 8 XCDs): the
    // number of splits is 8 g, and what counts is the busiest XCD -- ceil(tiles g / 32) rounds of ceil(nt / 8 g) K tiles on its 32
    // CUs -- plus the slab the reduce has to read back.  (34 splits of 15 tiles gave two XCDs 75 workgroups and six 60: three
    // rounds where the others needed two.)
    int sbw;
    if (tile_grid(tm, tn, syrk, &sbw) == 1) {
      double best = 0.0;
      int64_t gbest = 0;
      for (int64_t g = 1; g <= 16 && nt / (8 * g) >= 64; ++g) {
        const double tile_us = 1.85, slab_us = 8.0 * (double)g * (double)M * (double)N * 8.0 / 5.0e6;
        const double cost = (double)(cdiv(tiles * g, 32) * cdiv(nt, 8 * g)) * tile_us + slab_us;
        if (gbest == 0 || cost < best * 0.97) { best = cost; gbest = g; }   // (fewer splits unless more are worth 3 %)
      }
      if (gbest > 0) s = 8 * gbest;
    }
  }
  const int64_t kts = cdiv(nt, s);
  s = cdiv(nt, kts);
  pl.ksplit = (int)s;
  pl.kt_split = (int)kts;
  pl.kchunk = kts * BK;
  pl.slab_off = align_up(pieces, 256);
  pl.slab_bytes = (size_t)s * (size_t)M * (size_t)N * sizeof(float);
  pl.flags_off = align_up(pl.slab_off + pl.slab_bytes, 256);
  pl.bytes = pieces + 256 + pl.slab_bytes + 256 + 256;  // + range flag
  return true;
}

int launch_bx_splitk(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, hipStream_t stream) {
  const int nsplit = pl.ksplit;
  float *slab = ws_at<float>(workspace, pl.slab_off);
  int *flag = ws_at<int>(workspace, pl.flags_off);
  p.tiles_m = (int)cdiv(p.M, B2);
  p.tiles_n = (int)cdiv(p.N, B2);
  p.desc = nullptr;
  GemmBxArgs q;
  q.alpha = 1.f; q.beta = 0.f;
  q.syrk = sh.syrk ? 2 : 0;   // lower tiles only; the reduce mirrors
  const int64_t nsb = tile_grid(p.tiles_m, p.tiles_n, sh.syrk, &q.sbw);
  if (nsb < 0) return VIVIT_E_UNSUPPORTED;
  q.slab = slab; q.kt_split = pl.kt_split;
  q.flush_tiles = bx_flush_splitk;
  q.flush_diag = bx_flush_diag;
  dim3 grid((unsigned)(nsb * 256), (unsigned)nsplit);
  if (nsb == 1) {   // one (partial) super-block: the compact grid of map_tile_z, all tiles of a split on one XCD
    const int64_t d = p.tiles_m < p.tiles_n ? p.tiles_m : p.tiles_n;
    const int64_t v = sh.syrk ? d * (d + 1) / 2 : (int64_t)p.tiles_m * p.tiles_n;
    grid = dim3((unsigned)(8 * v * cdiv(nsplit, 8)), 1);
    q.sbw = -q.sbw;
  }
  if (!tile256_attrs() || !tile256_bx_attrs()) return VIVIT_E_LAUNCH;
  if (hipMemsetAsync(flag, 0, 4, stream) != hipSuccess) return VIVIT_E_LAUNCH;
  const bool prof = sh.syrk && sh.same && prof_enabled() && sh.pub;
  if (prof) prof_begin(0, (double)p.M * (double)(p.M + 1) * (double)p.K, stream);
  int st = launch_bx(pl, sh, alay, blay, p, workspace, 0, p.K, p.K, flag, q, grid, stream);
  if (st != VIVIT_OK) return st;
  GemmArgs f = p;   // the fp32 MFMA kernel with the same K split and slab
  f.ksplit = nsplit; f.kchunk = pl.kchunk; f.slab = slab;
  f.syrk = q.syrk; f.sbw = q.sbw;
  st = launch_fp32_standin(alay, blay, f, grid, flag, stream);
  if (st != VIVIT_OK) return st;
  launch_gemm_reduce(slab, p.C, p.M, p.N, p.ldc, nsplit, p.alpha, p.beta, sh.syrk ? 1 : 0, stream, B2);
  st = launch_status();
  if (st == VIVIT_OK && sh.syrk) {
    bx_sym_diag_kernel<<<(unsigned)p.tiles_m, 256, 0, stream>>>(p.C, p.M, p.ldc);
    st = launch_status();
  }
  if (prof) prof_end(0, stream);
  return st;
}

} // namespace vivit

#if defined(BX_STAMP)
using namespace vivit;

extern "C" int vivit_debug_bx_stamp_buffer(void *buf, unsigned int capacity) {
  unsigned long long *b = static_cast<unsigned long long *>(buf);
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_bx_stamp), &b, sizeof(b)) != hipSuccess) return VIVIT_E_LAUNCH;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_bx_stamp_cap), &capacity, sizeof(capacity)) != hipSuccess) return VIVIT_E_LAUNCH;
  return VIVIT_OK;
}
#endif
