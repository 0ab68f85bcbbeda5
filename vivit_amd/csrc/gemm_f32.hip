// fp32 GEMM / SYRK for gfx950 (MI355X): every large product of the library -- the Gram SYRK, the public
// vivit_gemm_nt/nn/tn_f32 and the eigensolver's internal products.  One translation unit per route:
//   gemm_tile.h           what the device code of more than one kernel family uses (tile constants, tile maps, DMA tiles)
//   gemm_plan.h           the host contract between the dispatcher and the routes: GemmShape, GemmPlan, the route table, the
//                         environment switches, the range gate, every plan_<route> / launch_<route>
//   gemm_tile128.hip      gemm_kernel: 128 x 128 (or 64 x 256) fp32 MFMA tile, every shape and layout; batched mode;
//                         gemm_lower_launch, gemm_batched_launch
//   gemm_tile256.hip      gemm256_kernel: 256 x 256 fp32 MFMA tile fed by global -> LDS DMA, for large outputs
//   gemm_tile256_bx.hip   bx_split_kernel, gemm256_bx_kernel: the same tile on the bf16 pipe, exact three-way operand splits
//                         (bx_kloop_asm.inc: its hand-scheduled K loop); bx_sym_diag_kernel; the split-K form for small outputs
//   gemm64.hip            gemm64_dma_kernel, g64_split_a_kernel, gemm64_bx_kernel: 64-row streaming kernels (M <= 64, wide N)
//                         on the fp32 and the bf16 pipe
//   gemm_tsk.hip          gemm_tsk_kernel, gemm_tsk_reduce_kernel: deep-K products with a small output
// This file: the fixed-order split-K reduction and the scaling of C that the routes share, the workspace query and the
// dispatcher built on the plans, the fp64 diagonal of the public SYRK, the C entry points.
#include "gemm_plan.h"

namespace vivit {

// C = alpha * sum_z slab[z] + beta * C  (fixed summation order); SYRK slabs hold the lower
// tiles only, the upper triangle is read from the transposed position.
__global__ __launch_bounds__(256) void gemm_reduce_kernel(const float *__restrict__ slab, float *__restrict__ C,
                                                          int64_t M, int64_t N, int64_t ldc, int ksplit,
                                                          float alpha, float beta, int syrk, int tile = BM) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * N) return;
  const int64_t i = idx / N, j = idx - i * N;
  int64_t src = idx;
  if (syrk && (j / tile) > (i / tile)) src = j * N + i;
  float s = 0.f;
  for (int z = 0; z < ksplit; ++z) s += slab[(int64_t)z * M * N + src];
  float v = alpha * s;
  if (beta != 0.f) v += beta * C[i * ldc + j];
  C[i * ldc + j] = v;
}
void launch_gemm_reduce(const float *slab, float *C, int64_t M, int64_t N, int64_t ldc, int ksplit, float alpha, float beta, int syrk,
                        hipStream_t stream, int tile) {
  gemm_reduce_kernel<<<(unsigned)cdiv(M * N, 256), 256, 0, stream>>>(slab, C, M, N, ldc, ksplit, alpha, beta, syrk, tile);
}

__global__ __launch_bounds__(256) void scale_c_kernel(float *__restrict__ C, int64_t M, int64_t N, int64_t ldc, float beta) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * N) return;
  const int64_t i = idx / N, j = idx - i * N;
  C[i * ldc + j] = beta == 0.f ? 0.f : beta * C[i * ldc + j];
}
void launch_scale_c(float *C, int64_t M, int64_t N, int64_t ldc, float beta, hipStream_t stream) {
  scale_c_kernel<<<(unsigned)cdiv(M * N, 256), 256, 0, stream>>>(C, M, N, ldc, beta);
}

// ---- the two callers of the plans
size_t gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, bool syrk) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const GemmShape sh{M, N, K, syrk, syrk, bx_public_product()};
  GemmShape whole = sh;   // the routes of the 256 tile and the 64-row route take K / BK whole tiles
  whole.K = K / BK * BK;
  size_t b = 0;
  GemmPlan pl;
  if (plan_tile256_bx(whole, pl) && pl.bytes > b) b = pl.bytes;
  if (plan_tile256(whole, pl) && pl.bytes > b) b = pl.bytes;
  if (plan_bx_splitk(whole, pl) && pl.bytes > b) b = pl.bytes;
  if (plan_gemm64(whole, pl) && pl.bytes > b) b = pl.bytes;
  if (plan_tsk(sh, pl) && pl.bytes > b) b = pl.bytes;
  if (plan_tile128(sh, pl) && pl.bytes > b) b = pl.bytes;
  return b;
}

// `probe`: launch nothing and return what the argument and workspace checks of the launch would return (vivit_gram_syrk_f32
// asks before it puts its diagonal kernel in front of a product on a short workspace).  SYRK only: of the routes a SYRK
// can take, Tile128 with a slab is the one that refuses a workspace.
static int gemm_dispatch(int alay, int blay, const float *A, const float *B, float *C, int64_t M, int64_t N,
                         int64_t K, int64_t lda, int64_t ldb, int64_t ldc, float alpha, float beta, bool syrk,
                         void *workspace, size_t workspace_bytes, hipStream_t stream, bool probe) {
  if (probe && !syrk) return VIVIT_E_UNSUPPORTED;
  if (M < 0 || N < 0 || K < 0) return VIVIT_E_BADARG;
  if (M == 0 || N == 0) return VIVIT_OK;
  if (!C || ldc < N) return VIVIT_E_BADARG;
  if (K == 0) {  // empty contraction: C = beta * C
    if (probe) return VIVIT_OK;
    launch_scale_c(C, M, N, ldc, beta, stream);
    return launch_status();
  }
  if (!A || !B) return VIVIT_E_BADARG;
  if (lda < (alay == LAY_K ? K : M) || ldb < (blay == LAY_K ? K : N)) return VIVIT_E_BADARG;
  if (syrk && (M != N || alay != blay)) return VIVIT_E_BADARG;

  GemmArgs p;
  p.A = A; p.B = B; p.C = C;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.alpha = alpha; p.beta = beta;
  const GemmShape sh{M, N, K, syrk, A == B && lda == ldb && M == N && alay == blay, bx_public_product()};
  const bool ptr_vec = operand_vec(A, lda) && operand_vec(B, ldb);
  const auto holds = [&](const GemmPlan &q) { return workspace && workspace_bytes >= q.bytes; };
  GemmPlan pl;
  // the 256-tile kernels take K / BK whole tiles
  if (ptr_vec && (alay == LAY_K || (M & 3) == 0) && (blay == LAY_K || (N & 3) == 0)) {
    GemmShape whole = sh;
    whole.K = p.K = K / BK * BK;
    bool on256 = true;
    int st = VIVIT_OK;
    if (plan_tile256_bx(whole, pl) && holds(pl)) {
      if (!probe) st = launch_tile256_bx(pl, whole, alay, blay, p, workspace, stream);
    } else if (plan_tile256(whole, pl)) {
      // never more splits than the caller's workspace holds (callers size it for their largest problem; the plan
      // of a smaller one may differ)
      if (pl.ksplit > 1 && !holds(pl)) {
        const size_t fit = workspace ? workspace_bytes / ((size_t)M * (size_t)N * sizeof(float)) : 1;
        plan_tile256(whole, pl, fit < 1 ? 1 : (int)(fit < 4 ? fit : 4));
      }
      if (!probe) st = launch_tile256(pl, whole, alay, blay, p, workspace, stream);
    } else if (plan_bx_splitk(whole, pl) && holds(pl)) {
      if (!probe) st = launch_bx_splitk(pl, whole, alay, blay, p, workspace, stream);
    } else {
      on256 = false;
      p.K = K;
    }
    if (on256) {
      if (st != VIVIT_OK || whole.K == K) return st;
      // ragged K tail (< 16) through the small-tile kernel, accumulating
      const float *At = A + (alay == LAY_K ? whole.K : whole.K * lda), *Bt = B + (blay == LAY_K ? whole.K : whole.K * ldb);
      return gemm_dispatch(alay, blay, At, Bt, C, M, N, K - whole.K, lda, ldb, ldc, alpha, 1.f, syrk, workspace, workspace_bytes, stream,
                           probe);
    }
  }
  if (gemm64_enabled() && ptr_vec && (alay == LAY_K || ((M & 3) == 0 && M >= 4)) && (blay == LAY_K || ((N & 3) == 0 && N >= 4)) &&
      plan_gemm64(sh, pl))
    return launch_gemm64(pl, sh, alay, blay, p, workspace, workspace_bytes, stream);
  if (tsk_enabled() && ptr_vec && alay == LAY_K && blay == LAY_K && plan_tsk(sh, pl))
    return launch_tsk(pl, p, workspace, workspace_bytes, stream);
  plan_tile128(sh, pl);
  if (probe) return (pl.ksplit > 1 && !holds(pl)) ? VIVIT_E_WORKSPACE : VIVIT_OK;   // (the check of launch_tile128)
  return launch_tile128(pl, sh, alay, blay, p, workspace, workspace_bytes, stream);
}

int gemm_launch(int alay, int blay, const float *A, const float *B, float *C, int64_t M, int64_t N,
                int64_t K, int64_t lda, int64_t ldb, int64_t ldc, float alpha, float beta, bool syrk,
                void *workspace, size_t workspace_bytes, hipStream_t stream) {
  return gemm_dispatch(alay, blay, A, B, C, M, N, K, lda, ldb, ldc, alpha, beta, syrk, workspace, workspace_bytes, stream, false);
}

// dout[i] = beta G[i][i] + alpha sum_k A[i][k]^2, fp64 accumulation, one workgroup per row (16 float4 loads in flight per thread)
template <bool VEC>
__global__ __launch_bounds__(256) void syrk_diag_kernel(const float *__restrict__ A, int64_t K, int64_t lda, const float *__restrict__ G,
                                                        int64_t ldg, float alpha, float beta, float *__restrict__ dout) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float *a = A + row * lda;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if constexpr (VEC) {
    const int64_t K4 = K / 4;
    int64_t c = tid;
    for (; c + 3 * 256 < K4; c += 4 * 256) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4 *>(a + 4 * (c + 256 * u));
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[0] = fma((double)v[u].x, (double)v[u].x, acc[0]);
        acc[1] = fma((double)v[u].y, (double)v[u].y, acc[1]);
        acc[2] = fma((double)v[u].z, (double)v[u].z, acc[2]);
        acc[3] = fma((double)v[u].w, (double)v[u].w, acc[3]);
      }
    }
    for (; c < K4; c += 256) {
      const float4 v = *reinterpret_cast<const float4 *>(a + 4 * c);
      acc[0] = fma((double)v.x, (double)v.x, acc[0]);
      acc[1] = fma((double)v.y, (double)v.y, acc[1]);
      acc[2] = fma((double)v.z, (double)v.z, acc[2]);
      acc[3] = fma((double)v.w, (double)v.w, acc[3]);
    }
    for (int64_t k = 4 * K4 + tid; k < K; k += 256) acc[0] = fma((double)a[k], (double)a[k], acc[0]);
  } else {
    for (int64_t k = tid; k < K; k += 256) acc[k & 3] = fma((double)a[k], (double)a[k], acc[k & 3]);
  }
  double sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    const double tot = (red[0] + red[1]) + (red[2] + red[3]);
    const double old = beta != 0.f ? (double)beta * (double)G[row * ldg + row] : 0.0;
    dout[row] = (float)(old + (double)alpha * tot);
  }
}

__global__ __launch_bounds__(256) void syrk_diag_store_kernel(float *__restrict__ G, int64_t ldg, int64_t n, const float *__restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) G[i * ldg + i] = d[i];
}

}  // namespace vivit

using namespace vivit;

extern "C" {

int vivit_gemm_split_mode(void) { return gemm_split_mode(); }

// The DIAGONAL of the public Gram product is computed on its own: G[i][i] = beta G[i][i] + alpha sum_k a_ik^2 is the one
// place where every term of the sum has the same sign, i.e. where the bf16 MFMA's truncation of aligned partial sums
// (see bx_flush_tiles) adds up to a bias instead of averaging out -- the reason the diagonal TILES ran chains of 512 k
// (+ 140 ms of flushes at the headline shape).  One streaming pass over A (66.7 GB: ~16 ms) with fp64 accumulation
// gives correctly rounded diagonal entries for every path, and the diagonal tiles keep the chain length of all others.
static size_t syrk_diag_bytes(int64_t n) { return align_up(sizeof(float) * (size_t)n, 256) + 256; }
constexpr int64_t SYRK_DIAG_MIN_K = 1024;   // below: the product's own diagonal (chains never end; nothing to fix)

size_t vivit_gram_syrk_f32_workspace_bytes(int64_t n, int64_t p) {
  BxStrictScope strict;   // sized for the public launch (one accumulation chain per chunk of the operand pieces)
  return gemm_workspace_bytes(n, n, p, true) + syrk_diag_bytes(n);
}

int vivit_gram_syrk_f32(const float *A, int64_t n, int64_t p, int64_t lda, float *G, int64_t ldg, float alpha,
                        float beta, void *workspace, size_t workspace_bytes, void *stream) {
  BxStrictScope strict;  // public product: both range bits reroute a chunk to the fp32 MFMA kernel
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (the leading dimensions are checked here too: gemm_launch refuses lda < p / ldg < n, and nothing may be launched before it does)
  bool fix_diag = A && G && workspace && n > 0 && p >= SYRK_DIAG_MIN_K && lda >= p && ldg >= n && workspace_bytes >= syrk_diag_bytes(n);
  // A workspace shorter than the query still gives the diagonal its n floats when the product accepts what is left behind them
  // (its routes cope with a short workspace: gemm_plan.h); asked first, since nothing may be launched in front of a refusal.
  // Where the rest is refused the product gets all of it, as it does when not even the diagonal fits, and the diagonal is its own.
  if (fix_diag && workspace_bytes < syrk_diag_bytes(n) + gemm_workspace_bytes(n, n, p, true))
    fix_diag = gemm_dispatch(LAY_K, LAY_K, A, A, G, n, n, p, lda, lda, ldg, alpha, beta, true, static_cast<char *>(workspace) + syrk_diag_bytes(n),
                             workspace_bytes - syrk_diag_bytes(n), s, true) == VIVIT_OK;
  float *diag = nullptr;
  if (fix_diag) {
    diag = reinterpret_cast<float *>(align_up(reinterpret_cast<uintptr_t>(workspace), 256));
    if (operand_vec(A, lda)) syrk_diag_kernel<true><<<(unsigned)n, 256, 0, s>>>(A, p, lda, G, ldg, alpha, beta, diag);
    else syrk_diag_kernel<false><<<(unsigned)n, 256, 0, s>>>(A, p, lda, G, ldg, alpha, beta, diag);
    workspace = reinterpret_cast<char *>(workspace) + syrk_diag_bytes(n);
    workspace_bytes -= syrk_diag_bytes(n);
  }
  const int st = gemm_launch(LAY_K, LAY_K, A, A, G, n, n, p, lda, lda, ldg, alpha, beta, true, workspace, workspace_bytes, s);
  if (st != VIVIT_OK || !fix_diag) return st;
  syrk_diag_store_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(G, ldg, n, diag);
  return launch_status();
}

size_t vivit_gemm_f32_workspace_bytes(int64_t m, int64_t n, int64_t k) {
  BxStrictScope strict;   // sized for the public launch
  size_t b = gemm_workspace_bytes(m, n, k, false);
  if (skinny_applicable(m, n, k)) {
    const size_t sb = skinny_workspace_bytes(m, k, n);
    if (sb > b) b = sb;
  }
  return b;
}

int vivit_gemm_nt_f32(const float *A, const float *B, float *C, int64_t m, int64_t n, int64_t k, int64_t lda,
                      int64_t ldb, int64_t ldc, float alpha, float beta, void *workspace, size_t workspace_bytes,
                      void *stream) {
  BxStrictScope strict;  // public product: both range bits reroute a chunk to the fp32 MFMA kernel
  return gemm_launch(LAY_K, LAY_K, A, B, C, m, n, k, lda, ldb, ldc, alpha, beta, false, workspace, workspace_bytes,
                     static_cast<hipStream_t>(stream));
}

int vivit_gemm_nn_f32(const float *A, const float *B, float *C, int64_t m, int64_t n, int64_t k, int64_t lda,
                      int64_t ldb, int64_t ldc, float alpha, float beta, void *workspace, size_t workspace_bytes,
                      void *stream) {
  BxStrictScope strict;
  // few output rows: HBM-bound streaming kernel instead of a mostly idle MFMA tile (K7/K8)
  if (skinny_applicable(m, n, k) && A && B && C && lda >= k && ldb >= n && ldc >= n &&
      workspace_bytes >= skinny_workspace_bytes(m, k, n) && workspace)
    return skinny_nn_launch(A, lda, B, ldb, C, ldc, m, k, n, alpha, beta, workspace, workspace_bytes,
                            static_cast<hipStream_t>(stream));
  return gemm_launch(LAY_K, LAY_M, A, B, C, m, n, k, lda, ldb, ldc, alpha, beta, false, workspace, workspace_bytes,
                     static_cast<hipStream_t>(stream));
}

int vivit_gemm_tn_f32(const float *A, const float *B, float *C, int64_t m, int64_t n, int64_t k, int64_t lda,
                      int64_t ldb, int64_t ldc, float alpha, float beta, void *workspace, size_t workspace_bytes,
                      void *stream) {
  BxStrictScope strict;  // public product: both range bits reroute a chunk to the fp32 MFMA kernel
  return gemm_launch(LAY_M, LAY_M, A, B, C, m, n, k, lda, ldb, ldc, alpha, beta, false, workspace, workspace_bytes,
                     static_cast<hipStream_t>(stream));
}

} // extern "C"
