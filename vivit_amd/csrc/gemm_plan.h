// Host contract between the GEMM dispatcher (gemm_f32.hip) and its routes, one translation unit each.
#pragma once
#include <cstdlib>

#include "gemm_tile.h"

namespace vivit {

// Host half.  Every route has ONE plan_<route> (shape predicate, split heuristic, workspace carve) and ONE launch_<route>
// that reads splits and offsets from the plan only; the workspace query and the dispatcher are both built on the plans.
//
// gemm_launch takes the first route of this table whose plan succeeds and whose extra conditions hold;
// gemm_workspace_bytes is the largest plan.bytes over the routes whose plan succeeds (it knows neither pointers nor
// layouts, so the extra conditions are the dispatcher's alone).  K of the first three routes is K / BK whole tiles; a
// ragged tail (< 16 k) goes through Tile128, accumulating.
//
//   route      kernels                                        extra conditions                     workspace < plan.bytes
//   Tile256Bx  bx_split_kernel, gemm256_bx_kernel,            16-byte operands (vec)               falls back to Tile256
//              gated gemm256_kernel
//   Tile256    gemm256_kernel                                 vec                                  fewer splits (down to one, which needs none)
//   BxSplitK   bx_split_kernel, gemm256_bx_kernel,            vec                                  skipped
//              gated gemm256_kernel, gemm_reduce_kernel
//   Gemm64     g64_split_a_kernel, gemm64_bx_kernel,          VIVIT_GEMM64 != 0, vec, M >= 4 for   VIVIT_E_WORKSPACE
//              gemm64_dma_kernel, gemm_reduce_kernel          row-major A, N >= 4 for row-major B
//   Tsk        gemm_tsk_kernel, gemm_tsk_reduce_kernel        VIVIT_GEMM_TSK != 0, vec, both       VIVIT_E_WORKSPACE
//                                                             operands K-contiguous
//   Tile128    gemm_kernel, gemm_reduce_kernel                none                                 VIVIT_E_WORKSPACE
//
// The asymmetry of the last column is deliberate: callers size one workspace for their largest problem, and the bf16-pipe
// routes of the 256 tile have an fp32 route of the same tile behind them that needs less; the last three routes have
// nothing behind them whose result (summation order) would be the same.  Every launch_<route> finishes its argument and
// workspace checks before its first HIP call.
// What the column does not say (tests/test_gemm_output_gpu.py runs every row of it):
//   - BxSplitK skipped means Tile128 with its own slab, i.e. VIVIT_E_WORKSPACE once that slab does not fit either.
//   - vivit_gram_syrk_f32 keeps the n floats of its fp64 diagonal (p >= 1024) in FRONT of this workspace.  A workspace shorter
//     than its query still gives them their room whenever the rows above accept what is left behind them (asked with a probe
//     of the dispatcher, before anything is launched); the diagonal is then the fp64 value rounded once, as on the whole
//     query.  Only where not even the n floats fit (a NULL workspace) or the rest would be refused does the product get all
//     of it, and the diagonal is the product's own: a k-ordered fp32 sum within the bound of every other entry.
enum class GemmRoute { Tile256Bx, Tile256, BxSplitK, Gemm64, Tsk, Tile128 };

struct GemmShape {
  int64_t M, N, K;
  bool syrk;   // lower tiles only, mirrored
  bool same;   // A and B are one operand (one set of bf16 pieces)
  bool pub;    // public product (BxStrictScope) or one of the eigensolver's own
};

struct GemmPlan {
  GemmRoute route;
  int ksplit;                    // parts of the contraction (1: no slab); nsplit of BxSplitK and Tsk
  int64_t kchunk;                // columns of K per part; Tile256Bx: per chunk of operand pieces (one launch each)
  int kt_split;                  // BxSplitK: K tiles per part
  size_t slab_off, slab_bytes;   // partial sums [ksplit][M][N]
  size_t a_off, b_off;           // bf16 pieces of the operands (b_off == a_off when they are one operand)
  size_t flags_off;              // range flags (BX_GATE): one per chunk
  size_t bytes;                  // all of it
};

template <class T>
static T *ws_at(void *workspace, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(workspace) + off); }

// Calls f with the operand layouts as std::integral_constant arguments, so that a launch can pass them on as template
// arguments: with_layouts(alay, blay, [&](auto LA, auto LB) { kernel<LA, LB><<<...>>>(...); })
template <class F>
static void with_layouts(int alay, int blay, F &&f) {
  using K = std::integral_constant<int, LAY_K>;
  using M = std::integral_constant<int, LAY_M>;
  if (alay == LAY_K && blay == LAY_K) f(K{}, K{});
  else if (alay == LAY_K && blay == LAY_M) f(K{}, M{});
  else if (alay == LAY_M && blay == LAY_K) f(M{}, K{});
  else f(M{}, M{});
}
// the same for one operand
template <class F>
static void with_layout(int lay, F &&f) {
  if (lay == LAY_K) f(std::integral_constant<int, LAY_K>{});
  else f(std::integral_constant<int, LAY_M>{});
}

// 16-byte loads are legal for the operand
static int operand_vec(const float *X, int64_t ld) { return ((reinterpret_cast<uintptr_t>(X) & 15) == 0 && (ld & 3) == 0) ? 1 : 0; }

// Super-block grid of a tile map (map_tile): *sbw = width of a super-block in tiles; returns the number of super-blocks
// (256 workgroup slots each), or -1 when the slots do not fit a 32-bit grid dimension.
static int64_t tile_grid(int64_t tiles_m, int64_t tiles_n, bool syrk, int *sbw) {
  const int w = syrk ? 16 : sb_width((int)tiles_m, (int)tiles_n), h = 256 / w;
  *sbw = w;
  const int64_t sbm = cdiv(tiles_m, h), sbn = cdiv(tiles_n, w);
  const int64_t nsb = syrk ? sbm * (sbm + 1) / 2 : sbm * sbn;
  return nsb * 256 > 0x7fffffffLL ? -1 : nsb;
}

// ---- the environment switches, each read once per process (inline: one cached value for the whole library)
static int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline bool gemm256_enabled() { static const int v = env_int("VIVIT_GEMM256", -1); return v != 0; }
inline bool bx_splitk_enabled() { static const int v = env_int("VIVIT_GEMM_BXSPLITK", -1); return v != 0; }
inline bool gemm64_enabled() { static const int v = env_int("VIVIT_GEMM64", -1); return v != 0; }
inline bool tsk_enabled() { static const int v = env_int("VIVIT_GEMM_TSK", -1); return v != 0; }
// Which matrix pipe the 256-tile NT products (Gram SYRK, K-contiguous GEMMs) use: 6 (default) = bf16 pipe with exact
// three-way operand splits and the 6 partial products that are >= 2^-16 of a product; 9 = all nine; 0 = fp32 MFMA
// (gemm256_kernel); 3 = hi hi + hi mid + mid hi of the three-way split (per-product error 2^-16: experiments only).
// VIVIT_GEMM_SPLIT overrides.
inline int gemm_split_mode() {
  static const int v = env_int("VIVIT_GEMM_SPLIT", 6);
  return (v == 0 || v == 3 || v == 6 || v == 9) ? v : 6;
}
// VIVIT_BX_ASM=1 / 0: the hand-scheduled K loop (gemm256_bx_kernel<6, true>) or the C++ loop (the reference implementation)
inline bool bx_asm_enabled() { static const int v = env_int("VIVIT_BX_ASM", 1); return v != 0; }
// products of the 64-row streaming kernel on the bf16 pipe (exact three-way splits) unless the fp32 pipe is asked for
// (VIVIT_GEMM_SPLIT=0 or VIVIT_GEMM64_BX=0)
inline bool gemm64_bx_enabled() { static const int v = env_int("VIVIT_GEMM64_BX", 1); return v != 0 && gemm_split_mode() != 0; }

// ---- the range gate of the bf16-pipe routes (the bits: bx_split_kernel, gemm_tile256_bx.hip)
constexpr int BX_GATE_RANGE = 1, BX_GATE_TINY = 2;
// Which range flags send a chunk to the fp32 MFMA kernel.  The public products (vivit_gram_syrk_f32, vivit_gemm_*_f32)
// honour both bits and so keep fp32-MFMA semantics for every input; the eigensolver's internal products on orthogonal
// factors only reroute non-finite / out-of-range chunks (a localised eigenvector has entries below 2^-100 whose
// 2^-126-level piece is immaterial, and the reroute would cost that chunk the bf16 pipe's 2.7x).
inline thread_local int tls_bx_gate_mask = BX_GATE_RANGE;   // (inline: one object per thread for the whole library)
// true inside a public product (vivit_gram_syrk_f32 / vivit_gemm_*_f32): the profile (roofline.achieved of bench.py) counts
// the Gram SYRKs of the caller, not the reflector Gram matrices the eigensolver's back-transformation builds internally
inline bool bx_public_product() { return (tls_bx_gate_mask & BX_GATE_TINY) != 0; }

struct BxStrictScope {
  int saved;
  BxStrictScope() : saved(tls_bx_gate_mask) { tls_bx_gate_mask = BX_GATE_RANGE | BX_GATE_TINY; }
  ~BxStrictScope() { tls_bx_gate_mask = saved; }
};

// ---- the routes, in the order of the table (definitions: the file named on the right)
bool plan_tile256_bx(const GemmShape &sh, GemmPlan &pl);                                                   // gemm_tile256_bx.hip
int launch_tile256_bx(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, hipStream_t stream);
bool plan_tile256(const GemmShape &sh, GemmPlan &pl, int max_split = 4);                                   // gemm_tile256.hip
int launch_tile256(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, hipStream_t stream);
bool plan_bx_splitk(const GemmShape &sh, GemmPlan &pl);                                                    // gemm_tile256_bx.hip
int launch_bx_splitk(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, hipStream_t stream);
bool plan_gemm64(const GemmShape &sh, GemmPlan &pl);                                                       // gemm64.hip
int launch_gemm64(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, size_t workspace_bytes,
                  hipStream_t stream);
bool plan_tsk(const GemmShape &sh, GemmPlan &pl);                                                          // gemm_tsk.hip
int launch_tsk(const GemmPlan &pl, const GemmArgs &g, void *workspace, size_t workspace_bytes, hipStream_t stream);
bool plan_tile128(const GemmShape &sh, GemmPlan &pl);                                                      // gemm_tile128.hip
int launch_tile128(const GemmPlan &pl, const GemmShape &sh, int alay, int blay, GemmArgs p, void *workspace, size_t workspace_bytes,
                   hipStream_t stream);

// ---- what the bf16-pipe routes of the 256 tile launch from gemm_tile256.hip: the gated gemm256_kernel, and its dynamic-LDS
// attribute (once per device; a route ensures the attributes of EVERY file it launches from before its first launch)
int launch_fp32_standin(int alay, int blay, GemmArgs f, dim3 grid, const int *flag, hipStream_t stream);
bool tile256_attrs();

// ---- gemm_f32.hip: the two small kernels that four routes and the dispatcher share (launch only: the caller asks launch_status())
void launch_gemm_reduce(const float *slab, float *C, int64_t M, int64_t N, int64_t ldc, int ksplit, float alpha, float beta, int syrk,
                        hipStream_t stream, int tile = BM);
void launch_scale_c(float *C, int64_t M, int64_t N, int64_t ldc, float beta, hipStream_t stream);

} // namespace vivit
