// Blocked Householder tridiagonalisation  A = Q T Q^T  for n above the single-workgroup size.
//
// Right-looking panels of PB columns (LAPACK ssytrd/slatrd ordering, lower triangle).  Per
// column j the chip-wide work is one symmetric matrix-vector product with the trailing matrix
// -- the HBM-bound heart of the eigensolver: (2/3) n^3 bytes over the whole reduction because
// only the lower triangle is streamed, each 128x256 tile being read once and used for both
// y_row += A v_col and y_col += A^T v_row -- plus O(n * PB) panel corrections; after a panel the
// trailing matrix receives one rank-2*PB update on MFMA (gemm_lower_launch).
//
// Launch structure: 5 small launches per column on one stream (column update + norm partials,
// reflector, symv tiles + panel dots, dot reduce, finish).  A dependent kernel boundary costs
// ~1.5-2 us on MI355X, cheaper than an in-kernel grid barrier (4-10 us), so the column loop is a
// stream of plain launches rather than a persistent cooperative kernel.  Cross-workgroup
// reductions go through partial slabs with a fixed summation order: no float atomics, results
// are bit-reproducible.
//
// Storage: A is n x n row-major; only A[i][j], i >= j is read.  Reflector j (v_j, v_j[j+1] = 1)
// is written to the dead upper-triangle row j: A[j][j+1 .. n-1]; tau, d, e go to vectors.
#include <cstdlib>

#include "common.h"
#include "device_utils.h"
#include "eig_internal.h"

namespace vivit {

constexpr int PB = 64;          // panel width
constexpr int TC = 256;         // symv wave tile: cols (64 lanes x float4)


// ------------------------------------------------------------------------------------------
// Scan: max |a_ij| over the lower triangle and a non-finite flag (for LAPACK-style scaling).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trd_scan_kernel(const float *__restrict__ A, int64_t lda, int n,
                                                       float *__restrict__ part) {
  __shared__ float red[4];
  const int i = blockIdx.x;  // one row per block
  float amax = 0.f, bad = 0.f;
  for (int c = threadIdx.x; c <= i; c += 256) {
    const float v = A[(int64_t)i * lda + c];
    amax = fmaxf(amax, fabsf(v));
    if (!(fabsf(v) <= 3.0e38f)) bad = 1.f;
  }
  amax = block_max(amax, red, threadIdx.x);
  bad = block_max(bad, red, threadIdx.x);
  if (threadIdx.x == 0) { part[2 * i] = amax; part[2 * i + 1] = bad; }
}

__global__ __launch_bounds__(256) void trd_sigma_kernel(const float *__restrict__ part, int n, float *__restrict__ scal) {
  __shared__ float red[4];
  float amax = 0.f, bad = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) { amax = fmaxf(amax, part[2 * i]); bad = fmaxf(bad, part[2 * i + 1]); }
  amax = block_max(amax, red, threadIdx.x);
  bad = block_max(bad, red, threadIdx.x);
  if (threadIdx.x == 0) {
    // power-of-two sigma (exact) into [1, 2) outside [2^-20, 2^51]: see csrc/symeig_small.hip for the lower end
    const float rmin = 9.5367432e-7f, rmax = 2.2517998e15f;
    float sigma = 1.f;
    if (amax > 0.f && (amax < rmin || amax > rmax)) {
      int ex;
      (void)frexpf(amax, &ex);
      ex = 1 - ex;
      sigma = ldexpf(1.f, ex > 127 ? 127 : (ex < -126 ? -126 : ex));   // (denormal amax: as far as fp32 goes)
    }
    scal[1] = sigma; scal[2] = bad; scal[3] = amax;
  }
}

__global__ __launch_bounds__(256) void trd_scale_kernel(float *__restrict__ A, int64_t lda, int n,
                                                        const float *__restrict__ scal) {
  const float sigma = scal[1];
  if (sigma == 1.f) return;
  const int i = blockIdx.x;
  for (int c = threadIdx.x; c <= i; c += 256) A[(int64_t)i * lda + c] *= sigma;
}

// ------------------------------------------------------------------------------------------
// K1: finalise W_{jj-1} (w = w' - 1/2 tau (w'.v) v) and form column j with the pending panel
//     update applied:  x[i] = A[i][j] - sum_{t<jj} V_t[i] W_t[j] + W_t[i] V_t[j],   i >= j.
//     Also emits the partial sums of squares of x[j+2:].
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trd_col_kernel(const float *__restrict__ A, int64_t lda, int n, int j, int jj,
                                                      int finalize_only, SytrdWs ws, int nprev) {
  __shared__ float red[4];
  __shared__ float s_w[PB], s_v[PB];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)j + (int64_t)blockIdx.x * 256 + tid;
  const int64_t N = n;
  float *V = ws.vw, *W = ws.vw + (int64_t)PB * N;
  float a2 = 0.f;
  if (jj > 0) {
    float s = 0.f;
    for (int t = tid; t < nprev; t += 256) s += ws.wdotpart[t];
    s = block_sum(s, red, tid);
    a2 = -0.5f * ws.tau[j - 1] * s;
  }
  float wfin = 0.f;
  if (jj > 0 && i < N) {
    const int64_t o = (int64_t)(jj - 1) * N + i;
    wfin = W[o] + a2 * V[o];
    // Element j of this row is read by every block below (s_w[jj-1]) and never needed again
    // afterwards: leave it un-finalised instead of racing with those reads.
    if (finalize_only || i != j) W[o] = wfin;
  }
  if (finalize_only) return;
  if (tid < jj) {
    const int64_t o = (int64_t)tid * N + j;
    float wj = W[o];
    if (tid == jj - 1) wj = wj + a2 * V[o];  // row j of W_{jj-1} may not be written back yet
    s_w[tid] = wj;
    s_v[tid] = V[o];
  }
  __syncthreads();
  float x = 0.f;
  if (i < N) {
    x = A[i * lda + j];
    for (int t = 0; t < jj; ++t) {
      const float wt = (t == jj - 1) ? wfin : W[(int64_t)t * N + i];
      x -= V[(int64_t)t * N + i] * s_w[t] + wt * s_v[t];
    }
    ws.xbuf[i] = x;
    if (i == j) ws.d[j] = x;
    if (i == j + 1) ws.scal[0] = x;
  }
  const float sq = (i < N && i >= j + 2) ? x * x : 0.f;
  const float ss = block_sum(sq, red, tid);
  if (tid == 0) ws.ssqpart[blockIdx.x] = ss;
}

// ------------------------------------------------------------------------------------------
// Householder scalars of column j, recomputed by every wavefront from the K1 partials (same
// instruction stream, same inputs: bit-identical in every wave, no extra launch, no broadcast).
// ------------------------------------------------------------------------------------------
struct Refl {
  float beta, tau, sc;
};

__device__ __forceinline__ Refl wave_reflector(const SytrdWs &ws, int npart, int lane) {
  float s = 0.f;
  for (int t = lane; t < npart; t += 64) s += ws.ssqpart[t];
  const float alpha = ws.scal[0];
  const float ssq = wave_sum_dpp(s);
  Refl r;
  r.beta = alpha; r.tau = 0.f; r.sc = 0.f;
  if (ssq > 0.f) {
    r.beta = -copysignf(sqrt_nr(alpha * alpha + ssq), alpha);
    r.tau = (r.beta - alpha) * rcp_nr(r.beta);
    r.sc = rcp_nr(alpha - r.beta);
  }
  return r;
}

// Guarded 4-wide load, BRANCH-FREE (out-of-range lanes read a dummy in-range address and select
// zero): a branch per load makes hipcc drain vmcnt(0) in front of every load, which serialises
// the stream.  VEC requires p 16-byte aligned, c % 4 == 0 and n % 4 == 0 (so c < n <=> c+3 < n).
template <bool VEC>
__device__ __forceinline__ float4 ld4_guard(const float *__restrict__ p, int64_t c, int64_t n) {
  if constexpr (VEC) {
    const bool ok = c < n;
    const float4 a = *reinterpret_cast<const float4 *>(p + (ok ? c : 0));
    return ok ? a : make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = c + k < n;
      const float x = p[ok ? c + k : 0];
      e[k] = ok ? x : 0.f;
    }
    return make_float4(e[0], e[1], e[2], e[3]);
  }
}

// v[idx] for idx = c .. c+3 from the un-scaled column x:  0 (idx <= j), 1 (idx == j+1), x * sc.
__device__ __forceinline__ float v_of(float x, int64_t idx, int j, float sc) {
  return idx <= j ? 0.f : (idx == j + 1 ? 1.f : x * sc);
}
template <bool VEC>
__device__ __forceinline__ float4 v4_of(const float *__restrict__ xbuf, int64_t c, int64_t n, int j, float sc) {
  const float4 x = ld4_guard<VEC>(xbuf, c, n);
  return make_float4(v_of(x.x, c, j, sc), v_of(x.y, c + 1, j, sc), v_of(x.z, c + 2, j, sc), v_of(x.w, c + 3, j, sc));
}

// Reduce 8 per-lane values over the 64 lanes; on return every lane holds the total of row
// rho(lane) = 4*bit5 + 2*bit4 + bit3 of its lane index.
__device__ __forceinline__ float reduce8(const float (&v)[8], int lane) {
  const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
  float a[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float send = b5 ? v[k] : v[k + 4];
    const float keep = b5 ? v[k + 4] : v[k];
    a[k] = keep + __shfl_xor(send, 32, 64);
  }
  float b[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float send = b4 ? a[k] : a[k + 2];
    const float keep = b4 ? a[k + 2] : a[k];
    b[k] = keep + __shfl_xor(send, 16, 64);
  }
  float c;
  {
    const float send = b3 ? b[0] : b[1];
    const float keep = b3 ? b[1] : b[0];
    c = keep + __shfl_xor(send, 8, 64);
  }
  c += __shfl_xor(c, 4, 64);
  c += __shfl_xor(c, 2, 64);
  c += __shfl_xor(c, 1, 64);
  return c;
}
__device__ __forceinline__ int rho_of(int lane) {
  return ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);
}

// One TRR x 256 tile: returns the lane's 4 column sums, leaves the TRR row sums in `rowsum`.
// FAST = strictly-lower in-bounds tile: unconditional 16-byte loads, no masks.
template <bool VEC, bool FAST>
__device__ __forceinline__ void symv_load_group(const float *__restrict__ A, int64_t lda, int64_t N, int64_t R0, int64_t c, int g,
                                                float4 (&dst)[8]) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int64_t i = R0 + g * 8 + u;
    if constexpr (FAST) {
      dst[u] = *reinterpret_cast<const float4 *>(A + i * lda + c);
    } else {
      const bool rowok = i < N;
      const float4 a = ld4_guard<VEC>(A + (rowok ? i : 0) * lda, c, N);
      dst[u] = rowok ? a : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

// `bufa` arrives with row group 0 already requested (symv_load_group<..>(.., 0, bufa) by the caller, in front of the
// reflector scalars: one memory round trip less on the launch's critical path).
template <bool VEC, int TRR, bool FAST>
__device__ __forceinline__ float4 symv_tile(const float *__restrict__ A, int64_t lda, int64_t N, int64_t R0, int64_t c,
                                            float4 vc, const float (&vr)[(TRR + 63) / 64], int lane,
                                            float *__restrict__ rowsum, float4 (&bufa)[8]) {
  float4 colacc = make_float4(0.f, 0.f, 0.f, 0.f);
  auto load_group = [&](int g, float4(&dst)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t i = R0 + g * 8 + u;
      if constexpr (FAST) {
        dst[u] = *reinterpret_cast<const float4 *>(A + i * lda + c);
      } else {
        const bool rowok = i < N;
        const float4 a = ld4_guard<VEC>(A + (rowok ? i : 0) * lda, c, N);
        dst[u] = rowok ? a : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  auto compute_group = [&](int g, const float4(&src)[8]) {
    float racc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = g * 8 + u;
      const int64_t i = R0 + r;
      const float vsel = (TRR > 64 && r >= 64) ? vr[(TRR + 63) / 64 - 1] : vr[0];
      const float vi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vsel), r & 63));
      float4 x = src[u];
      if constexpr (!FAST) {
        // triangle mask: keep c+e <= i for the row product ...
        x.x = (c + 0 > i) ? 0.f : x.x;
        x.y = (c + 1 > i) ? 0.f : x.y;
        x.z = (c + 2 > i) ? 0.f : x.z;
        x.w = (c + 3 > i) ? 0.f : x.w;
      }
      racc[u] = x.x * vc.x + x.y * vc.y + x.z * vc.z + x.w * vc.w;
      if constexpr (!FAST) {
        // ... and c+e < i for the column product (the diagonal counts once)
        x.x = (c + 0 == i) ? 0.f : x.x;
        x.y = (c + 1 == i) ? 0.f : x.y;
        x.z = (c + 2 == i) ? 0.f : x.z;
        x.w = (c + 3 == i) ? 0.f : x.w;
      }
      colacc.x += x.x * vi; colacc.y += x.y * vi; colacc.z += x.z * vi; colacc.w += x.w * vi;
    }
    const float tot = reduce8(racc, lane);
    if ((lane & 7) == 0) rowsum[g * 8 + rho_of(lane)] = tot;
  };
  constexpr int NG = TRR / 8;
  float4 bufb[8];
#pragma unroll 1
  for (int g = 0; g < NG; g += 2) {
    load_group(g + 1, bufb);
    compute_group(g, bufa);
    if (g + 2 < NG) load_group(g + 2, bufa);
    compute_group(g + 1, bufb);
  }
  return colacc;
}

constexpr int NAUX = 16;  // auxiliary wavefronts: write v / reflector row, panel dot products

// ------------------------------------------------------------------------------------------
// K2: symmetric matrix-vector product over the lower triangle (+ reflector write, panel dots).
//     One wavefront per TRR x 256 tile (TRR = 128 for large trailing matrices: 1.2 % slab
//     overhead; 32 for small ones: 4x more waves to hide latency); lanes span 4 columns each
//     (16-byte loads), rows are walked 8 at a time with the next 8 rows' loads already in flight.
//     Row sums need a cross-lane reduction (recursive halving, 10 shuffles per 8 rows), column
//     sums accumulate in registers.  Every tile writes TRR row partials and 256 column partials
//     to slabs; K3 adds them in a fixed order.
// ------------------------------------------------------------------------------------------
template <bool VEC, int TRR>
__global__ __launch_bounds__(256) void trd_symv_kernel(float *__restrict__ A, int64_t lda, int n, int j, int jj,
                                                       SytrdWs ws, int rt0, int nrt, int ct0, int nct, int npart) {
  __shared__ float rowsum[4][TRR];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t N = n;
  const int ntile = nrt * nct;
  const int widx = blockIdx.x * 4 + wave;
  const float *__restrict__ xb = ws.xbuf;
  // tile coordinates, and everything the tile reads that does not depend on the reflector scalars (first row group of
  // A, the x values behind v) requested BEFORE those scalars are reduced: the launch is latency-bound (4-5 dependent
  // round trips at 12.9 us per column for n ~ 1000) and this takes one round trip off the chain
  const bool is_tile = widx < ntile;
  const int rt = rt0 + (is_tile ? widx / nct : 0), ct = ct0 + (is_tile ? widx % nct : 0);
  const int64_t R0 = (int64_t)rt * TRR, C0 = (int64_t)ct * TC;
  const bool active = is_tile && !(C0 > R0 + TRR - 1);   // (entirely above the diagonal: no partials are ever read from it)
  const int64_t c = C0 + 4 * lane;
  const bool interior = VEC && (C0 + TC - 1 < R0) && (R0 + TRR - 1 < N);  // strictly below the diagonal, in bounds
  float4 bufa[8];
  float4 xc4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float xr[(TRR + 63) / 64];
  if (active) {
    if (interior) symv_load_group<VEC, true>(A, lda, N, R0, c, 0, bufa);
    else symv_load_group<VEC, false>(A, lda, N, R0, c, 0, bufa);
    xc4 = ld4_guard<VEC>(xb, c, N);
#pragma unroll
    for (int k = 0; k < (TRR + 63) / 64; ++k) {
      const int64_t i = R0 + 64 * k + lane;
      xr[k] = xb[(i < N && 64 * k + lane < TRR) ? i : 0];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  const Refl rf = wave_reflector(ws, npart, lane);

  if (widx >= ntile) {
    // ---- auxiliary wave: materialise v for its chunks, then the panel dots V^T v, W^T v
    const int aw = widx - ntile;
    const int naux = nct < NAUX ? nct : NAUX;
    if (aw >= naux) return;
    for (int chunk = aw; chunk < nct; chunk += naux) {
      const int64_t c = (int64_t)(ct0 + chunk) * TC + 4 * lane;
      const float4 v4 = v4_of<VEC>(xb, c, N, j, rf.sc);
      const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t idx = c + e;
        if (idx < N && idx > j) {
          ws.vw[(int64_t)jj * N + idx] = vv[e];
          ws.vw[(int64_t)(2 * PB + jj) * N + idx] = vv[e];
          A[(int64_t)j * lda + idx] = vv[e];  // reflector storage: dead upper-triangle row j
        }
      }
    }
    if (aw == 0 && lane == 0) { ws.e[j] = rf.beta; ws.tau[j] = rf.tau; }
    float *out = ws.dotpart + (int64_t)aw * (2 * PB);
    for (int t0 = 0; t0 < jj; t0 += 8) {
      float pv[8], pw[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { pv[u] = 0.f; pw[u] = 0.f; }
      for (int chunk = aw; chunk < nct; chunk += naux) {
        const int64_t c = (int64_t)(ct0 + chunk) * TC + 4 * lane;
        const float4 vc = v4_of<VEC>(xb, c, N, j, rf.sc);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int t = t0 + u;
          if (t < jj) {
            const float4 a = ld4_guard<VEC>(ws.vw + (int64_t)t * N, c, N);
            const float4 b = ld4_guard<VEC>(ws.vw + (int64_t)(PB + t) * N, c, N);
            pv[u] += a.x * vc.x + a.y * vc.y + a.z * vc.z + a.w * vc.w;
            pw[u] += b.x * vc.x + b.y * vc.y + b.z * vc.z + b.w * vc.w;
          }
        }
      }
      const float rv = reduce8(pv, lane);
      const float rw = reduce8(pw, lane);
      if ((lane & 7) == 0 && t0 + rho_of(lane) < jj) {
        out[t0 + rho_of(lane)] = rv;
        out[PB + t0 + rho_of(lane)] = rw;
      }
    }
    return;
  }

  // ---- symv tile
  if (!active) return;
  const float4 vc = make_float4(v_of(xc4.x, c, j, rf.sc), v_of(xc4.y, c + 1, j, rf.sc), v_of(xc4.z, c + 2, j, rf.sc),
                                v_of(xc4.w, c + 3, j, rf.sc));   // v[c..c+3]  (zero up to j and beyond n)
  float vr[(TRR + 63) / 64];                          // v[R0 + 64*k + lane]
#pragma unroll
  for (int k = 0; k < (TRR + 63) / 64; ++k) {
    const int64_t i = R0 + 64 * k + lane;
    const bool ok = i < N && 64 * k + lane < TRR;
    vr[k] = ok ? v_of(xr[k], i, j, rf.sc) : 0.f;
  }
  float4 colacc;
  if (interior)
    colacc = symv_tile<VEC, TRR, true>(A, lda, N, R0, c, vc, vr, lane, rowsum[wave], bufa);
  else
    colacc = symv_tile<VEC, TRR, false>(A, lda, N, R0, c, vc, vr, lane, rowsum[wave], bufa);
  // column partials: one coalesced 1 KiB store per wave
  float *cp = ws.colpart + (int64_t)(rt - rt0) * N;
  if (VEC) {
    if (c < N) *reinterpret_cast<float4 *>(cp + c) = colacc;
  } else {
    if (c < N) cp[c] = colacc.x;
    if (c + 1 < N) cp[c + 1] = colacc.y;
    if (c + 2 < N) cp[c + 2] = colacc.z;
    if (c + 3 < N) cp[c + 3] = colacc.w;
  }
  // row partials (same wave wrote rowsum: LDS ops of one wave are ordered)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  float *rp = ws.rowpart + (int64_t)(ct - ct0) * N;
#pragma unroll
  for (int k = 0; k < (TRR + 63) / 64; ++k)
    if (64 * k + lane < TRR && R0 + 64 * k + lane < N) rp[R0 + 64 * k + lane] = rowsum[wave][64 * k + lane];
}

// Deterministic strided partial sum: terms first, first + step, ... < count, 4 accumulators.
__device__ __forceinline__ float sum_strided(const float *__restrict__ p, int64_t stride, int first, int step,
                                             int count) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int k = first;
  for (; k + 3 * step < count; k += 4 * step) {
    s0 += p[(int64_t)k * stride];
    s1 += p[(int64_t)(k + step) * stride];
    s2 += p[(int64_t)(k + 2 * step) * stride];
    s3 += p[(int64_t)(k + 3 * step) * stride];
  }
  for (; k < count; k += step) s0 += p[(int64_t)k * stride];
  return (s0 + s1) + (s2 + s3);
}

// ------------------------------------------------------------------------------------------
// K3: y = sum of partials;  w' = tau (y - V c_w - W c_v);  partial w'.v.   Rows i >= j+1.
//     64 rows per workgroup (lane = row); the 4 waves split the partial/panel index 4 ways to
//     shorten the dependent chains, their sums are combined through LDS in a fixed order.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trd_finish_kernel(int n, int j, int jj, SytrdWs ws, int rt0, int nrt, int ct0,
                                                         int nct, int tr) {
  __shared__ float s_c[2 * PB];
  __shared__ float part[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 2 * PB) {
    const int naux = nct < NAUX ? nct : NAUX;
    const int tt = tid < PB ? tid : tid - PB;
    float s = 0.f;
    if (tt < jj)
      for (int a = 0; a < naux; ++a) s += ws.dotpart[(int64_t)a * (2 * PB) + tid];
    s_c[tid] = s;
  }
  __syncthreads();
  const int64_t N = n;
  const int64_t i = (int64_t)j + 1 + (int64_t)blockIdx.x * 64 + lane;
  const float *V = ws.vw, *W = ws.vw + (int64_t)PB * N;
  float y = 0.f;
  if (i < N) {
    const int ctl = (int)(i / TC);
    y = sum_strided(ws.rowpart + i, N, wave, 4, ctl - ct0 + 1);
    int rtf = (int)(i / tr);
    if (rtf < rt0) rtf = rt0;
    y += sum_strided(ws.colpart + (int64_t)(rtf - rt0) * N + i, N, wave, 4, rt0 + nrt - rtf);
    float c0 = 0.f, c1 = 0.f;
    int t = wave;
    for (; t + 4 < jj; t += 8) {
      c0 += V[(int64_t)t * N + i] * s_c[PB + t] + W[(int64_t)t * N + i] * s_c[t];
      c1 += V[(int64_t)(t + 4) * N + i] * s_c[PB + t + 4] + W[(int64_t)(t + 4) * N + i] * s_c[t + 4];
    }
    if (t < jj) c0 += V[(int64_t)t * N + i] * s_c[PB + t] + W[(int64_t)t * N + i] * s_c[t];
    y -= c0 + c1;
  }
  part[wave][lane] = y;
  __syncthreads();
  if (wave == 0) {
    float wv = 0.f;
    if (i < N) {
      const float yt = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
      const float w = ws.tau[j] * yt;
      ws.vw[(int64_t)(PB + jj) * N + i] = w;
      wv = w * V[(int64_t)jj * N + i];
    }
    const float s = wave_sum(wv);
    if (lane == 0) ws.wdotpart[blockIdx.x] = s;
  }
}

// Tail: d[n-2], e[n-2], d[n-1] from the last 2x2 block with the pending panel applied.
__global__ void trd_tail_kernel(const float *__restrict__ A, int64_t lda, int n, int jjcount, SytrdWs ws) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t N = n;
  const float *V = ws.vw, *W = ws.vw + (int64_t)PB * N;
  const int64_t rows[3] = {N - 2, N - 1, N - 1}, cols[3] = {N - 2, N - 2, N - 1};
  float out[3];
  for (int q = 0; q < 3; ++q) {
    const int64_t i = rows[q], k = cols[q];
    float x = A[i * lda + k];
    for (int t = 0; t < jjcount; ++t)
      x -= V[(int64_t)t * N + i] * W[(int64_t)t * N + k] + W[(int64_t)t * N + i] * V[(int64_t)t * N + k];
    out[q] = x;
  }
  ws.d[n - 2] = out[0];
  ws.e[n - 2] = out[1];
  ws.d[n - 1] = out[2];
  ws.e[n - 1] = 0.f;
  ws.tau[n - 2] = 0.f;
  ws.tau[n - 1] = 0.f;
}

// ------------------------------------------------------------------------------------------
// The block's buffers, in order.  The arena of a launch hands out 16-byte regions; sytrd_workspace_floats measures the
// plain lengths and its slack of 64 floats covers the 13 roundings (3 floats each at most).
SytrdLayout sytrd_layout(Arena &a, int64_t n) {
  const int64_t nct = cdiv(n, TC), nrt = cdiv(n, 32), nwg = cdiv(n, 64) + 1;
  SytrdLayout L;
  SytrdWs &ws = L.ws;
  ws.vw = a.take<float>(3 * PB * n);
  ws.xbuf = a.take<float>(n);
  ws.rowpart = a.take<float>(nct * n);
  ws.colpart = a.take<float>(nrt * n);
  ws.dotpart = a.take<float>(NAUX * 2 * PB);
  ws.cvw = a.take<float>(2 * PB);
  ws.ssqpart = a.take<float>(nwg);
  ws.wdotpart = a.take<float>(nwg);
  ws.scal = a.take<float>(16);
  ws.d = a.take<float>(n);
  ws.e = a.take<float>(n);
  ws.tau = a.take<float>(n);
  L.scanpart = a.take<float>(2 * n);
  return L;
}

size_t sytrd_workspace_floats(int64_t n) {
  Arena m(sizeof(float));
  sytrd_layout(m, n);
  return (m.used() / sizeof(float) + 64) / 4 * 4 + 64;
}

int prescale_launch(float *A, int64_t n, int64_t lda, float *scal, float *part, hipStream_t stream) {
  const int ni = (int)n;
  trd_scan_kernel<<<ni, 256, 0, stream>>>(A, lda, ni, part);
  trd_sigma_kernel<<<1, 256, 0, stream>>>(part, ni, scal);
  trd_scale_kernel<<<ni, 256, 0, stream>>>(A, lda, ni, scal);
  return launch_status();
}

int sytrd_batched_launch(float *const *A, int batch, int64_t n, int64_t lda, const SytrdLayout *L, hipStream_t stream) {
  if (batch < 1 || batch > PERSIST_MAX_BATCH) return VIVIT_E_UNSUPPORTED;
  SytrdWs ws[PERSIST_MAX_BATCH];
  for (int q = 0; q < batch; ++q) {
    ws[q] = L[q].ws;
    prescale_launch(A[q], n, lda, ws[q].scal, L[q].scanpart, stream);
  }
  return sytrd_persist_batched_launch(A, batch, n, lda, ws, stream);
}

// Tridiagonalise A (n x n, lda).  On return ws.d / ws.e / ws.tau hold T and the reflector
// scalars, A's upper-triangle rows hold the reflectors, ws.scal[1] the applied scaling sigma
// and ws.scal[2] the non-finite-input flag.
int sytrd_launch(float *A, int64_t n, int64_t lda, const SytrdLayout &L, hipStream_t stream) {
  const SytrdWs ws = L.ws;
  const int ni = (int)n;
  const bool vec = ((reinterpret_cast<uintptr_t>(A) & 15) == 0) && (lda % 4 == 0) && (n % 4 == 0);

  prescale_launch(A, n, lda, ws.scal, L.scanpart, stream);
  if (sytrd_persist_ok(n)) return sytrd_persist_launch(A, n, lda, ws, stream);   // one persistent launch on one XCD

  for (int64_t j0 = 0; j0 < n - 2; j0 += PB) {
    const int bb = (int)((n - 2 - j0) < PB ? (n - 2 - j0) : PB);
    if (hipMemsetAsync(ws.vw, 0, sizeof(float) * 3 * PB * n, stream) != hipSuccess) return VIVIT_E_LAUNCH;
    for (int jj = 0; jj < bb; ++jj) {
      const int j = (int)(j0 + jj);
      const int g1 = (int)cdiv(n - j, 256);      // rows i >= j
      const int nprev = (int)cdiv(n - j, 64);    // finish-kernel grid of column j-1 (rows >= j, 64 per block)
      trd_col_kernel<<<g1, 256, 0, stream>>>(A, lda, ni, j, jj, 0, ws, nprev);
      const int64_t mtrail = n - j - 1;
      const int tr = mtrail > 16384 ? 128 : 32;
      const int rt0 = (j + 1) / tr, nrt = (int)cdiv(n, tr) - rt0;
      const int ct0 = (j + 1) / TC, nct = (int)cdiv(n, TC) - ct0;
      const int nwave = nrt * nct + (nct < NAUX ? nct : NAUX);
      const unsigned g = (unsigned)cdiv(nwave, 4);
      const bool prof = prof_enabled() && (j % prof_stride() == 0);
      if (prof) prof_begin(1, 2.0 * (double)(n - j - 1) * (double)(n - j), stream);  // 4 B * m(m+1)/2
      if (vec && tr == 128)
        trd_symv_kernel<true, 128><<<g, 256, 0, stream>>>(A, lda, ni, j, jj, ws, rt0, nrt, ct0, nct, g1);
      else if (vec)
        trd_symv_kernel<true, 32><<<g, 256, 0, stream>>>(A, lda, ni, j, jj, ws, rt0, nrt, ct0, nct, g1);
      else if (tr == 128)
        trd_symv_kernel<false, 128><<<g, 256, 0, stream>>>(A, lda, ni, j, jj, ws, rt0, nrt, ct0, nct, g1);
      else
        trd_symv_kernel<false, 32><<<g, 256, 0, stream>>>(A, lda, ni, j, jj, ws, rt0, nrt, ct0, nct, g1);
      if (prof) prof_end(1, stream);
      trd_finish_kernel<<<(unsigned)cdiv(n - j - 1, 64), 256, 0, stream>>>(ni, j, jj, ws, rt0, nrt, ct0, nct, tr);
    }
    // finalise the last W of the panel (rows >= j0 + bb)
    {
      const int j = (int)(j0 + bb);
      const int g1 = (int)cdiv(n - j, 256);
      trd_col_kernel<<<g1, 256, 0, stream>>>(A, lda, ni, j, bb, 1, ws, (int)cdiv(n - j, 64));
    }
    const int64_t off = j0 + bb;
    if (off < n - 2) {
      // trailing update A[off:, off:] -= V W^T + W V^T  (lower tiles, MFMA, K = 2*PB)
      const int st = gemm_lower_launch(ws.vw + off, ws.vw + (int64_t)PB * n + off, A + off * lda + off, n - off, 2 * PB,
                                       n, n, lda, -1.f, 1.f, stream);
      if (st != VIVIT_OK) return st;
    } else {
      trd_tail_kernel<<<1, 64, 0, stream>>>(A, lda, ni, bb, ws);
    }
  }
  return launch_status();
}

} // namespace vivit
