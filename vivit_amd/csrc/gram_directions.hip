// Gram-space epilogue of the directional derivatives (K5 + K6) for a batch of per-layer groups, gfx950.
//
// One launch, blockIdx.y = problem.  Per problem b with K = K[b] kept directions (rows of Zt):
//   gammas[j, k]  = alpha_gamma * sum_i VtG[i, j] Zt[k, i] * (1 / sqrt(evals[k]))
//   lambdas[m, k] = lambda_scale * sum_c (alpha_gram * sum_i G[(c, m), i] Zt[k, i])^2 / evals[k]
// G E never reaches memory: a workgroup owns ONE sample m and GD_KT directions across all C classes, its four
// wavefronts take the classes c = w, w + 4, ... (one row of G each, streamed coalesced; G is symmetric, so the row IS
// the column the formula asks for), square the finished dot products in registers and add them over c; the four
// partial sums meet in LDS in a fixed order.  The gamma workgroups own 16 columns j x GD_KT directions: 16 slices of the
// i range per column, reduced through LDS in a fixed order.  No atomics; what a problem's workgroups compute does not
// depend on the rest of the batch (the grid is sized by the largest K, surplus workgroups leave at once).
// The work is latency bound (2 n K (n + M) flop per problem, G read once per GD_KT directions); Zt (K n floats) is
// re-read through L1/L2 by every workgroup instead of being staged, which keeps LDS use at 8 KB and any n legal.
#include "common.h"

namespace vivit {

constexpr int GD_BLOCK = 256;       // 4 wavefronts
constexpr int GD_WAVES = GD_BLOCK / 64;
constexpr int GD_KT = 8;            // directions per workgroup
constexpr int GD_JT = 16;           // gamma columns per workgroup
constexpr int GD_IS = GD_BLOCK / GD_JT;   // slices of the i range per gamma column
constexpr int GD_MAX_BATCH = 64;    // problems per launch: the descriptors travel as kernel arguments (56 B each, 4 KB limit)

struct GramDirProblem {
  const float *G, *Zt, *evals, *VtG;
  float *gammas, *lambdas;
  int64_t K;
};
struct GramDirBatch {
  GramDirProblem p[GD_MAX_BATCH];
};

__global__ __launch_bounds__(GD_BLOCK) void gram_directions_batched_kernel(GramDirBatch bb, int64_t n, int64_t ldg, int64_t ldz,
                                                                           int64_t ldv, int64_t C, int64_t N, int64_t M,
                                                                           int64_t lam_blocks, int64_t kchunks, float alpha_gram,
                                                                           float alpha_gamma, float lambda_scale) {
  __shared__ float red[GD_IS][GD_KT][GD_JT];   // 8 KB; the lambda role uses red[w][kk][0]
  const GramDirProblem &p = bb.p[blockIdx.y];
  const int64_t K = p.K;
  const bool is_lambda = (int64_t)blockIdx.x < lam_blocks;
  const int64_t local = is_lambda ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - lam_blocks;
  const int64_t tile = local / kchunks, k0 = (local - tile * kchunks) * GD_KT;
  if (k0 >= K) return;   // the whole workgroup: no barrier is missed
  const int tid = threadIdx.x;
  const float *__restrict__ Zt = p.Zt;
  // rows of Zt of this chunk; directions past K read row K - 1 (valid memory) and are never stored
  const float *zrow[GD_KT];
#pragma unroll
  for (int kk = 0; kk < GD_KT; ++kk) zrow[kk] = Zt + (k0 + kk < K ? k0 + kk : K - 1) * ldz;

  if (is_lambda) {
    const int64_t m = tile;   // < N by the grid
    const int lane = tid & 63, w = tid >> 6;
    float lam[GD_KT];
#pragma unroll
    for (int kk = 0; kk < GD_KT; ++kk) lam[kk] = 0.f;
    for (int64_t c = w; c < C; c += GD_WAVES) {
      const float *__restrict__ grow = p.G + (c * N + m) * ldg;
      float acc[GD_KT];
#pragma unroll
      for (int kk = 0; kk < GD_KT; ++kk) acc[kk] = 0.f;
#pragma unroll 4
      for (int64_t i = lane; i < n; i += 64) {
        const float g = grow[i];
#pragma unroll
        for (int kk = 0; kk < GD_KT; ++kk) acc[kk] += g * zrow[kk][i];
      }
#pragma unroll
      for (int kk = 0; kk < GD_KT; ++kk) {
        float d = acc[kk];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
        d *= alpha_gram;
        lam[kk] += d * d;
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int kk = 0; kk < GD_KT; ++kk) red[w][kk][0] = lam[kk];
    }
    __syncthreads();
    if (tid < GD_KT && k0 + tid < K) {
      const float s = (red[0][tid][0] + red[1][tid][0]) + (red[2][tid][0] + red[3][tid][0]);
      p.lambdas[m * K + k0 + tid] = lambda_scale * s / p.evals[k0 + tid];
    }
    return;
  }

  // gamma role: columns j0 .. j0 + 15 of VtG, i split over GD_IS interleaved slices
  const int jl = tid & (GD_JT - 1), is = tid / GD_JT;
  const int64_t j = tile * GD_JT + jl;
  const bool jok = j < M;
  const float *__restrict__ vcol = p.VtG + (jok ? j : 0);
  float acc[GD_KT];
#pragma unroll
  for (int kk = 0; kk < GD_KT; ++kk) acc[kk] = 0.f;
#pragma unroll 4
  for (int64_t i = is; i < n; i += GD_IS) {
    const float v = jok ? vcol[i * ldv] : 0.f;
#pragma unroll
    for (int kk = 0; kk < GD_KT; ++kk) acc[kk] += v * zrow[kk][i];
  }
#pragma unroll
  for (int kk = 0; kk < GD_KT; ++kk) red[is][kk][jl] = acc[kk];
  __syncthreads();
  if (tid < GD_KT * GD_JT) {
    const int kk = tid / GD_JT, jo = tid & (GD_JT - 1);
    const int64_t jj = tile * GD_JT + jo, k = k0 + kk;
    if (jj < M && k < K) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < GD_IS; ++q) s += red[q][kk][jo];
      p.gammas[jj * K + k] = (alpha_gamma * s) * (1.f / sqrtf(p.evals[k]));
    }
  }
}

} // namespace vivit

using namespace vivit;

extern "C" {

int vivit_gram_directions_batched_f32(const float *const *G, int64_t batch, int64_t n, int64_t ldg, const float *const *Zt,
                                      int64_t ldz, const float *const *evals, const float *const *VtG, int64_t ldv,
                                      const int64_t *K, int64_t C, int64_t N, int64_t M, float alpha_gram, float alpha_gamma,
                                      float lambda_scale, float *const *gammas, float *const *lambdas, void *stream) {
  if (batch < 0 || n < 0 || C < 0 || N < 0 || M < 0) return VIVIT_E_BADARG;
  if (C > 0 && N > INT64_MAX / C) return VIVIT_E_BADARG;
  if (C * N != n || ldg < n || ldz < n || ldv < M) return VIVIT_E_BADARG;
  if (batch == 0) return VIVIT_OK;
  if (!G || !Zt || !evals || !VtG || !K || !gammas || !lambdas) return VIVIT_E_BADARG;
  int64_t kmax_all = 0;
  for (int64_t b = 0; b < batch; ++b) {   // everything is checked before anything is launched
    if (K[b] < 0 || K[b] > n) return VIVIT_E_BADARG;
    if (K[b] == 0) continue;
    if (!G[b] || !Zt[b] || !evals[b] || !lambdas[b]) return VIVIT_E_BADARG;
    if (M > 0 && (!VtG[b] || !gammas[b])) return VIVIT_E_BADARG;
    if (K[b] > kmax_all) kmax_all = K[b];
  }
  if (kmax_all == 0) return VIVIT_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int64_t b0 = 0; b0 < batch; b0 += GD_MAX_BATCH) {
    const int64_t nb = batch - b0 < GD_MAX_BATCH ? batch - b0 : GD_MAX_BATCH;
    GramDirBatch bb = {};
    int64_t kmax = 0;
    for (int64_t q = 0; q < nb; ++q) {
      const int64_t b = b0 + q;
      bb.p[q].K = K[b];
      if (K[b] == 0) continue;
      bb.p[q].G = G[b]; bb.p[q].Zt = Zt[b]; bb.p[q].evals = evals[b]; bb.p[q].VtG = VtG[b];
      bb.p[q].gammas = gammas[b]; bb.p[q].lambdas = lambdas[b];
      if (K[b] > kmax) kmax = K[b];
    }
    if (kmax == 0) continue;
    const int64_t kchunks = cdiv(kmax, GD_KT);
    const int64_t lam_blocks = N * kchunks, gam_blocks = cdiv(M, GD_JT) * kchunks;
    if (lam_blocks + gam_blocks > 0x7fffffffLL) return VIVIT_E_UNSUPPORTED;
    gram_directions_batched_kernel<<<dim3((unsigned)(lam_blocks + gam_blocks), (unsigned)nb), GD_BLOCK, 0, s>>>(
        bb, n, ldg, ldz, ldv, C, N, M, lam_blocks, kchunks, alpha_gram, alpha_gamma, lambda_scale);
    const int st = launch_status();
    if (st != VIVIT_OK) return st;
  }
  return VIVIT_OK;
}

} // extern "C"
