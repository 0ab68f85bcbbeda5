// Large-output variant: 256 x 256 x 16 tile, 4 waves in a 2 x 2 grid, each wave a 128 x 128 block =
// 4 x 4 MFMA tiles (256 accumulator registers: one wave per SIMD, the unified 512-register file).
// Half the LDS operand traffic per flop of the 128 x 128 tile and 128 MFMAs (8192 cycles) per wave
// between barriers.  With a single wave per SIMD nothing else hides latency, so:
//  * operands go global -> LDS directly (`global_load_lds_dwordx4`: lane i's 16 bytes land at
//    M0 + 16 i, probed in scripts/probe/lds_probe.hip), no staging registers, three LDS stages: the
//    loads of tile t+2 are issued at the top of tile t (two K tiles ~ 16 000 cycles of latency cover;
//    a register-staged version with half a tile of cover stalled on HBM round trips).  The LDS image
//    of a wave instruction is one contiguous KB, so K-major tiles cannot be padded; instead each lane
//    fetches the 16-byte chunk `pos ^ ((row >> 2) & 3)` of its row (the lane -> global address map is
//    free), which makes the ds_read_b128 fragment reads conflict-free.  The DMA is issued through
//    inline asm with hand-placed `s_waitcnt vmcnt` (the compiler would wait for vmcnt(0) in front of
//    every LDS read that follows an LDS-DMA it knows about).
//  * the K loop is software-pipelined in half K tiles (8 k): the fragment reads of the next half are
//    issued in front of the 64 MFMAs of the current one; one barrier per K tile.
// Ragged edge tiles read clamped (duplicate) rows instead of zeros: those accumulators are never stored.
// The second accumulation level lives in C itself: every 8192 k the accumulators are added into the
// output tile (read-modify-write through L2, 128 KB per wave every ~10^6 cycles) and cleared - the same
// pairwise-like rounding as the register `tot` of the small tile, without the registers.
#include "gemm_plan.h"

namespace vivit {

constexpr int T2 = B2 * BK;                         // 4096 floats (16 KB) per operand tile, unpadded
constexpr int STG2 = 2 * T2;                        // one stage: A tile, B tile
constexpr int GEMM256_LDS_BYTES = 3 * STG2 * 4;     // 96 KB
constexpr int FLUSH2_TILES = 8192 / BK;             // second-level accumulation period of this kernel

template <int ALAY, int BLAY>
__global__ __launch_bounds__(256, 1) void gemm256_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem2[];
  // stand-in for a bf16-pipe launch whose operand chunk is out of the split's range: runs only when the chunk is flagged
  if (p.gate && (*p.gate & p.gate_mask) == 0) return;
  int ti, tj, zsplit;
  if (!map_tile_z(p.syrk, p.sbw, p.tiles_m, p.tiles_n, p.ksplit, ti, tj, zsplit)) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)ti * B2, col0 = (int64_t)tj * B2;
  // split-K (few tiles, deep K: Gram matrices of small batches): split zsplit owns [kbeg, kend) and writes a slab
  const int64_t kbeg = (int64_t)zsplit * p.kchunk;
  const int64_t kend = (kbeg + p.kchunk < p.K) ? kbeg + p.kchunk : p.K;
  const int nt = (int)((kend - kbeg) / BK);  // K and kchunk are multiples of 16 (host)
  const bool partial = p.ksplit > 1;

#define S2A(st) (smem2 + (st) * STG2)
#define S2B(st) (smem2 + (st) * STG2 + T2)

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  gptr Cout = (gptr)(partial ? p.slab + (int64_t)zsplit * p.M * p.N : p.C);
  const int64_t ldc = partial ? p.N : p.ldc;
  const float alpha_ = partial ? 1.f : p.alpha, beta_ = partial ? 0.f : p.beta;
  const bool full_tile = row0 + B2 <= p.M && col0 + B2 <= p.N;
  // C <- C' + alpha * acc with C' = beta * C on the first flush and C afterwards; acc <- final value
  auto flush_to_c = [&](bool first) __attribute__((always_inline)) {
    const float beta = first ? beta_ : 1.f;
    // the 256 output addresses are loop-invariant: without an opaque term LICM hoists them out of the
    // K loop (512 registers of addresses -> scratch spills in the hot loop)
    int opaque = 0;
    __asm__ volatile("" : "+v"(opaque));
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        __asm__ volatile("" ::: "memory");  // one tile (16 loads, 16 stores) at a time
        const int64_t rbase = row0 + wm * 128 + i * 32 + 4 * h + opaque, col = col0 + wn * 128 + j * 32 + r;
        if (full_tile) {
          gptr cbase = Cout + rbase * ldc + col;
          float old[16];
          if (beta != 0.f) {
#pragma unroll
            for (int e = 0; e < 16; ++e) old[e] = cbase[(int64_t)((e & 3) + 8 * (e >> 2)) * ldc];
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            float v = alpha_ * acc[i][j][e];
            if (beta != 0.f) v += beta * old[e];
            cbase[(int64_t)((e & 3) + 8 * (e >> 2)) * ldc] = v;
            acc[i][j][e] = v;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int64_t row = rbase + (e & 3) + 8 * (e >> 2);
            float v = alpha_ * acc[i][j][e];
            if (row < p.M && col < p.N) {
              gptr c = Cout + row * ldc + col;
              if (beta != 0.f) v += beta * *c;
              *c = v;
            }
            acc[i][j][e] = v;
          }
        }
      }
  };
  auto clear_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  };

  float fa[2][4][4], fb[2][4][4];  // [half parity][tile][k pair]
  auto frags = [&](int st, int q, int par) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) frag_half<ALAY>(S2A(st), wm * 128 + i * 32 + r, q, h, fa[par][i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) frag_half<BLAY>(S2B(st), wn * 128 + j * 32 + r, q, h, fb[par][j]);
  };
  // DMA sources: wave w moves blocks w, w+4, w+8, w+12 of each operand tile; pointers advance per K tile
  gcptr srcA[4], srcB[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    srcA[u] = dma_src<ALAY>(p.A, p.lda, row0, p.M, wave + 4 * u, lane) + (ALAY == LAY_K ? kbeg : kbeg * p.lda);
    srcB[u] = dma_src<BLAY>(p.B, p.ldb, col0, p.N, wave + 4 * u, lane) + (BLAY == LAY_K ? kbeg : kbeg * p.ldb);
  }
  const int64_t stepA = (ALAY == LAY_K) ? BK : (int64_t)BK * p.lda, stepB = (BLAY == LAY_K) ? BK : (int64_t)BK * p.ldb;
  // LDS byte address of this wave's first block (wave-uniform: SGPR for M0)
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)smem2 +
                                                       (unsigned)(wave * 256 * 4));
  // issue the 8 DMA instructions of the next not yet requested K tile into stage st
  auto issue = [&](int st) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dma16(srcA[u], lds0 + (unsigned)((st * STG2 + 4 * u * 256) * 4));
      srcA[u] += stepA;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dma16(srcB[u], lds0 + (unsigned)((st * STG2 + T2 + 4 * u * 256) * 4));
      srcB[u] += stepB;
    }
  };

  // One K tile at stage S.  LOAD: request tile t+2 into stage S+2; NEXT: tile t+1 exists.  Tile t+1's DMA
  // was requested one K tile (8192 MFMA cycles) ago; every wave waits for its own part at the top of the
  // tile, BEFORE requesting tile t+2, and the barrier between the two halves publishes it to the other
  // waves.  That wait is the compiler-visible `s_waitcnt` builtin on purpose: hipcc cannot see the asm DMA,
  // but it does see its own spill reloads / flush accesses in the loop preheader, and with those pending in
  // its scoreboard it would put a vmcnt(0) in front of the first MFMA of every trip - after the DMA request.
  // The LDS reads (8 per half) and DMA requests (8 per tile) are spread over the four 16-MFMA k-steps of a
  // half instead of being issued back to back (the LDS / VMEM issue queues are short: a burst stalls the
  // wave at issue and drains the MFMA pipe); sched_barrier(0) fences keep hipcc from regrouping them.
  auto frag1 = [&](int st, int q, int par, int u) __attribute__((always_inline)) {  // A tile u and B tile u
    frag_half<ALAY>(S2A(st), wm * 128 + u * 32 + r, q, h, fa[par][u]);
    frag_half<BLAY>(S2B(st), wn * 128 + u * 32 + r, q, h, fb[par][u]);
  };
  auto mfma_step = [&](int par, int tt) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[par][i][tt], fb[par][j][tt], acc[i][j], 0, 0, 0);
  };
  auto issue2 = [&](int st, int u) __attribute__((always_inline)) {  // DMA blocks u of A and B
    dma16(srcA[u], lds0 + (unsigned)((st * STG2 + 4 * u * 256) * 4));
    srcA[u] += stepA;
    dma16(srcB[u], lds0 + (unsigned)((st * STG2 + T2 + 4 * u * 256) * 4));
    srcB[u] += stepB;
  };
  auto body = [&](auto stage, bool do_load, bool has_next) __attribute__((always_inline)) {
    constexpr int S = decltype(stage)::value, S1 = (S + 1) % 3, S2 = (S + 2) % 3;
    __builtin_amdgcn_sched_barrier(0);   // tile boundary: the wait below stays behind the previous tile's MFMAs
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      if (do_load) issue2(S2, tt);
      frag1(S, 1, 1, tt);
      mfma_step(0, tt);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (has_next) __syncthreads();
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      if (has_next) frag1(S1, 0, 0, tt);
      mfma_step(1, tt);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  // K is processed in chunks of FLUSH2_TILES tiles: a clean software-pipelined loop per chunk (the
  // accumulators stay in AGPRs), then the chunk sum is added into C.
  auto chunk = [&](int t0, int t1) __attribute__((always_inline)) {
    __syncthreads();  // every wave is done with the LDS stages of the previous chunk
    issue(0);
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t0 + 1 < t1) issue(1);
    __syncthreads();
    frags(0, 0, 0);
    int t = t0;
    for (; t + 4 < t1; t += 3) {  // steady state: three tiles per trip, every one requests tile t+2
      body(I0{}, true, true);
      body(I1{}, true, true);
      body(I2{}, true, true);
    }
    // at most 4 tiles left
    if (t < t1) { body(I0{}, t + 2 < t1, t + 1 < t1); ++t; }
    if (t < t1) { body(I1{}, t + 2 < t1, t + 1 < t1); ++t; }
    if (t < t1) { body(I2{}, t + 2 < t1, t + 1 < t1); ++t; }
    if (t < t1) { body(I0{}, false, false); ++t; }
  };
  bool first_flush = true;
  for (int t0 = 0; t0 < nt; t0 += FLUSH2_TILES) {
    const int t1 = t0 + FLUSH2_TILES < nt ? t0 + FLUSH2_TILES : nt;
    if (t0 > 0) clear_acc();
    chunk(t0, t1);
    flush_to_c(first_flush);  // after the last chunk acc holds the final values of the tile
    first_flush = false;
  }

  if (p.syrk == 1 && ti != tj && !partial) {
    // Mirror image through LDS (32 x 33 floats per wave), as in the small-tile kernel
    __syncthreads();  // the last K tile has no barrier: every wave must be done reading the LDS stages
    float *ts = smem2 + wave * (32 * 33);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // own patch: wave-local ordering suffices
#pragma unroll
        for (int e = 0; e < 16; ++e) ts[r * 33 + (e & 3) + 8 * (e >> 2) + 4 * h] = acc[i][j][e];
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
}

// hipFuncAttributeMaxDynamicSharedMemorySize of gemm256_kernel, once per device
bool tile256_attrs() {
  static unsigned long long attr_done = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (attr_done & (1ull << (dev & 63))) return true;
  const struct { const void *fn; int bytes; } kernels[] = {
      {reinterpret_cast<const void *>(gemm256_kernel<LAY_K, LAY_K>), GEMM256_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm256_kernel<LAY_K, LAY_M>), GEMM256_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm256_kernel<LAY_M, LAY_K>), GEMM256_LDS_BYTES},
      {reinterpret_cast<const void *>(gemm256_kernel<LAY_M, LAY_M>), GEMM256_LDS_BYTES}};
  for (const auto &k : kernels)
    if (!ensure_dynamic_lds(k.fn, k.bytes, attr_done)) return false;
  attr_done |= 1ull << (dev & 63);
  return true;
}

// ---- Tile256: gemm256_kernel, split-K over blockIdx.y
// The 256 x 256 tile pays off once the output has enough of them to fill the chip (one per CU).
// Small outputs with a deep contraction stay on the 128 x 128 tile: measured with the 256 tile's split-K on the Gram
// matrices of small batches (n = 1280, P = 4e5) the streamed K-major operand reached only 0.2 TB/s - 17 splits x 1280
// row streams 1.6 MB apart - and the 128 x 128 tile with its 2 workgroups per CU was twice as fast (27 ms vs 59 ms).
// Split-K here only fills the last round of workgroups of a large output (at most 4 splits, and never more than
// `max_split`: gemm_launch passes what the caller's workspace holds).
bool plan_tile256(const GemmShape &sh, GemmPlan &pl, int max_split) {
  const int64_t M = sh.M, N = sh.N, K = sh.K;
  const bool syrk = sh.syrk;
  pl = GemmPlan{};
  pl.route = GemmRoute::Tile256;
  pl.ksplit = 1;
  pl.kchunk = cdiv(K, BK) * BK;
  if (!gemm256_enabled() || K < 512) return false;
  const int64_t tm = cdiv(M, B2), tn = cdiv(N, B2);
  const int64_t tiles = syrk ? tm * (tm + 1) / 2 : tm * tn;
  // one workgroup per CU: prologue (first DMA round trip) and epilogue (256 KB of C) are not overlapped with
  // another workgroup's main loop, so the contraction must be long enough to amortise them
  if (tiles < 200) return false;
  if (max_split > 4) max_split = 4;
  if (M < 512 || N < 512) return false;
  const int64_t ktiles = K / BK;
  const double flops = (syrk ? 1.0 : 2.0) * (double)M * (double)N * (double)K;
  const double t_mfma = flops / 140e12;
  double best = 0.0;
  int best_s = 0;
  for (int s = 1; s <= max_split; ++s) {
    if (s > 1 && ktiles / s < 128) break;  // every split keeps >= 2048 k
    if (s > 1 && (size_t)s * (size_t)M * (size_t)N * 4 > ((size_t)1 << 30)) break;  // slab cap (no slab for s = 1)
    const int64_t wgs = tiles * s;
    const double fill = (double)wgs / (double)(256 * cdiv(wgs, 256));
    const double t_slab = s > 1 ? 2.0 * s * (double)M * (double)N * 4.0 / 3e12 : 0.0;
    const double eff = fill / (1.0 + t_slab / t_mfma);
    if (eff > best + 1e-9) { best = eff; best_s = s; }
  }
  if (best_s == 0 || best < 0.6) return false;
  if (best_s > 1) {
    pl.kchunk = cdiv(ktiles, best_s) * BK;
    pl.ksplit = (int)cdiv(K, pl.kchunk);
    pl.slab_bytes = (size_t)pl.ksplit * (size_t)M * (size_t)N * sizeof(float);
  }
  pl.bytes = pl.slab_bytes;
  return true;
}

int launch_tile256(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, hipStream_t stream) {
  p.ksplit = pl.ksplit;
  p.kchunk = pl.kchunk;
  p.slab = pl.ksplit > 1 ? ws_at<float>(workspace, pl.slab_off) : nullptr;
  p.tiles_m = (int)cdiv(p.M, B2);
  p.tiles_n = (int)cdiv(p.N, B2);
  p.syrk = sh.syrk ? 1 : 0;
  p.a_vec = operand_vec(p.A, p.lda);
  p.b_vec = operand_vec(p.B, p.ldb);
  p.desc = nullptr;
  const int64_t nsb = tile_grid(p.tiles_m, p.tiles_n, sh.syrk, &p.sbw);
  if (nsb < 0) return VIVIT_E_UNSUPPORTED;
  if (!tile256_attrs()) return VIVIT_E_LAUNCH;
  dim3 grid((unsigned)(nsb * 256), (unsigned)p.ksplit, 1);
  const bool prof = sh.syrk && p.A == p.B && prof_enabled() && sh.pub;
  if (prof) prof_begin(0, (double)p.M * (double)(p.M + 1) * (double)p.K, stream);
  with_layouts(alay, blay, [&](auto LA, auto LB) { gemm256_kernel<LA, LB><<<grid, 256, GEMM256_LDS_BYTES, stream>>>(p); });
  int st = launch_status();
  if (st == VIVIT_OK && p.ksplit > 1) {
    launch_gemm_reduce(p.slab, p.C, p.M, p.N, p.ldc, p.ksplit, p.alpha, p.beta, p.syrk, stream, B2);
    st = launch_status();
  }
  if (prof) prof_end(0, stream);
  return st;
}

// BX_GATE: the fp32 MFMA kernel on the grid of the bf16-pipe launch it stands in for; every workgroup returns at once unless
// the range flag of the chunk is set
int launch_fp32_standin(int alay, int blay, GemmArgs f, dim3 grid, const int *flag, hipStream_t stream) {
  f.a_vec = operand_vec(f.A, f.lda);
  f.b_vec = operand_vec(f.B, f.ldb);
  f.gate = flag; f.gate_mask = tls_bx_gate_mask;
  with_layouts(alay, blay, [&](auto LA, auto LB) { gemm256_kernel<LA, LB><<<grid, 256, GEMM256_LDS_BYTES, stream>>>(f); });
  return launch_status();
}

} // namespace vivit
