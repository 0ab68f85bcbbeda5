// Mamba-2 state-space-dual layer (SSD): the forward pass and, from ONE visit of the factor, the input rule and the three parameter
// rules.  vivit_ssd_forward_f32 and vivit_ssd_rules_f32 (include/vivit_hip.h: formulas and layouts).  One scalar A per head makes a
// chunk of time steps a handful of dense products, and these run on the fp32 matrix pipe (__builtin_amdgcn_mfma_f32_16x16x4f32, as
// attention_common.h uses it); no bf16 splits, no packed fp32, no atomics.
//
// Notation, per (n, h) and inside a chunk of Q steps: Delta_t, A = -exp(A_log_h), l_t = sum_{r <= t} Delta_r A (inclusive, <= 0),
// Xd_t = Delta_t x_t, Hin the P x S state at the chunk's start, lQ = l_{Q-1}.  Steps beyond T have Delta = 0 and x = B = C = M = 0:
// they change nothing and are never stored.  P is a compile-time variant PP in {32, 64}, S a variant SP in {64, 128}; smaller sizes
// are padded with zero columns that are never stored.  Every product is ssd_tile: 16 x 16 tiles, operands in LDS (row pitch + 4).
//
// PRECISION.  Delta (softplus), A, the sigmoid and the prefix sums l_t are fp64; every exponent is an fp64 difference l_t - l_s <= 0
// rounded once to fp32 before expf.  Everything else is fp32.
//
// FORWARD  ssd_forward_kernel<PP, SP, Q = 64, false>, 256 lanes, one workgroup per (n, h) for the whole sequence.  Hs [PP x SP] lives
// in MFMA accumulators (tile id = wave + 4 i: 32 registers a lane at 64 x 128) and is copied to LDS at a chunk's start as an operand.
//   W_ts = expf(l_t - l_s) (C_t . B_s) Delta_s for s <= t, else 0                      (Q x SP x Q, tiles above the diagonal skipped)
//   y_t = expf(l_t) (C Hin^T)_t + (W X)_t + Dk x_t                                    (Q x SP x PP, then Q x Q x PP up to the diagonal)
//   Hs = expf(lQ) Hs + (diag(Delta_t expf(lQ - l_t)) X)^T B                            (PP x Q x SP)
// It writes y and nothing else.  <.., Q = 32, true> is phase 1 of the rules: the state update alone, and Hs is stored to the
// workspace after every chunk but the last.
// SUMMATION ORDER of y: the MFMA chain over s ascending in steps of 4, scaled by expf(l_t), continued over the steps ascending, then
// fmaf(Dk, x, .).
//
// RULES  ssd_rules_kernel<PP, SP>, chunks of SSD_RCHUNK = 32 steps (see below), one workgroup per (v, n, h), chunks in reverse.  The
// adjoint of the chunk boundary Lt = a_{t+1} Lam_{t+1} [PP x SP] is carried in MFMA accumulators as Hs is in the forward pass (and
// copied to LDS as an operand); Hin comes from the workspace.  With d_rs = expf(l_r - l_s) for s <= r, else 0:
//   cb = C B^T, mx = (M X^T) diag(Delta);   W = d o cb,  G = d o mx,  Z = W o mx                                  (to LDS)
//   LB = diag(expf(lQ - l_t)) (B Lt^T) + W^T M  (= Lam_t B_t);   g_x = fmaf(Delta_t, LB, Dk M);   xlb_t = sum_p x LB
//   MH = M Hin;   g_C = diag(expf(l_t)) MH + G B;   q_t = expf(l_t) sum_s C o MH
//   XL = X Lt;    g_B = diag(Delta_t expf(lQ - l_t)) XL + G^T C;   p_t = Delta_t expf(lQ - l_t) sum_s B o XL
//   U = Z Tri with Tri_st = [s < t] (0/1, made in registers);   R_t = sum_{r >= t} U_rt
//   e_t = ((R_t + sum_{r >= t} q_r) + sum_{s < t} p_s) + expf(lQ) <Lt, Hin>       (= <Lam_t, a_t Hs_{t-1}>: four sums of terms of
//   the majorant, no difference of large sums: the state a_t Hs_{t-1} is taken with s < t strictly, not as Hs_t minus its last term)
//   g_dt = fmaf(A, e_t, xlb_t) sigmoid;   Lt = expf(lQ) Lt + (diag(expf(l_t)) M)^T C
// Row sums over p or s: 16 lanes by xor 1, 2, 4, 8, then the column tiles ascending; R_t: the four values of a lane, xor 16, 32, the
// row tiles ascending; <Lt, Hin>: lane, wave (xor 1 .. 32), waves ascending; suffix sums from r = Q - 1 down, prefix sums from 0 up.
// F_A = A sum e_t Delta_t, F_Dk = sum M_t . x_t (p ascending, fmaf), F_dtb = sum g_dt: per step of a chunk over the chunks in
// reverse, then the 32 steps ascending.  g_B | g_C of a group with one head go straight into g; otherwise per-head partials go to the
// workspace and ssd_fold_kernel adds them in ascending head order.
// `want` only removes work (bit 0 clear: no g products or stores; want == 4: the dot products alone, no workspace) and the plan is a
// function of the sizes alone: the bytes of every result are the same on every run and for every `want`.
// LDS at 64 x 128: forward 138240 B, rules 137104 B: one workgroup per compute unit.  All element offsets are 64-bit.
// (vivit_amd/kernels.py repeats SSD_CHUNK, SSD_MAX_STATE and SSD_MAX_HEAD_DIM for the tests that name the edges.)
#include "common.h"

namespace vivit {

typedef float ssd_f32x4 __attribute__((ext_vector_type(4)));
constexpr int SSD_CHUNK = 64, SSD_RCHUNK = 32, SSD_THREADS = 256, SSD_WAVES = 4;
constexpr int SSD_MAX_STATE = 128, SSD_MAX_HEAD_DIM = 64;

struct SsdGeo {
  int64_t V, N, T, H, Wd, nchunk;   // Wd: width of a row of x and g; nchunk: chunks of SSD_RCHUNK steps
  int P, S, G, hpg, softplus, want;
};

__device__ inline double ssd_softplus(double v) { return v > 0.0 ? v + log1p(exp(-v)) : log1p(exp(v)); }
__device__ inline double ssd_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

// acc[i][j] += sum_{k < K} A(i0 + i, k) B(k, j0 + j) for one 16 x 16 tile, K a multiple of 4.  AT: A is stored [k][i], else [i][k];
// BT: B is stored [j][k], else [k][j].  The lane holds acc[4 (lane >> 4) + e][lane & 15], e < 4.
template <bool AT, bool BT>
__device__ __forceinline__ ssd_f32x4 ssd_tile(const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb, int i0, int j0,
                                              int K, int lane, ssd_f32x4 acc) {
  const int r = lane & 15, q = lane >> 4;
  const float *a = AT ? A + q * lda + i0 + r : A + (i0 + r) * lda + q;
  const float *b = BT ? B + (j0 + r) * ldb + q : B + q * ldb + j0 + r;
  const int sa = AT ? 4 * lda : 4, sb = BT ? 4 : 4 * ldb;
  for (int k = 0; k < K; k += 4) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(*a, *b, acc, 0, 0, 0);
    a += sa;
    b += sb;
  }
  return acc;
}

__device__ __forceinline__ float ssd_red16(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// The scalars of a chunk: l (fp64), Delta, sigmoid (or 1), expf(l_t), expf(lQ - l_t).  Ends with a barrier.
template <int Q>
__device__ __forceinline__ void ssd_stage_scalars(const float *__restrict__ row0, int64_t Wd, int64_t off_dt, double bias, double A,
                                                  int len, int softplus, double *sDd, double *sL, float *sDl, float *sSg, float *sEL,
                                                  float *sER) {
  const int tid = threadIdx.x;
  if (tid < Q) {
    double dl = 0.0, sg = 1.0;
    if (tid < len) {
      const double dt = (double)row0[(int64_t)tid * Wd + off_dt] + bias;
      dl = softplus ? ssd_softplus(dt) : dt;
      if (softplus) sg = ssd_sigmoid(dt);
    }
    sDd[tid] = dl;
    sDl[tid] = (float)dl;
    sSg[tid] = (float)sg;
  }
  __syncthreads();
  if (tid == 0) {
    double l = 0.0;
    for (int t = 0; t < Q; ++t) {
      l += sDd[t] * A;
      sL[t] = l;
    }
  }
  __syncthreads();
  if (tid < Q) {
    sEL[tid] = expf((float)sL[tid]);
    sER[tid] = expf((float)(sL[Q - 1] - sL[tid]));
  }
  __syncthreads();
}

// rows t < Q of a [.., Wd] matrix from column `off`, `cols` live columns of CP, into dst[Q][CP + 4]; zero beyond len and cols
template <int Q, int CP>
__device__ __forceinline__ void ssd_load(float *__restrict__ dst, const float *__restrict__ row0, int64_t stride, int64_t off, int cols,
                                         int len) {
  for (int idx = threadIdx.x; idx < Q * CP; idx += SSD_THREADS) {
    const int t = idx / CP, c = idx - t * CP;
    dst[t * (CP + 4) + c] = (t < len && c < cols) ? row0[(int64_t)t * stride + off + c] : 0.f;
  }
}

template <int PP, int SP, int Q> struct SsdFwdLds {
  static constexpr int LDB = SP + 4, LDX = PP + 4, LDW = Q + 4;
  static constexpr int FLOATS = 2 * Q * LDB + Q * LDX + Q * LDW + PP * LDB + 4 * Q;
  static constexpr int BYTES = 2 * Q * 8 + FLOATS * 4;
};

template <int PP, int SP, int Q, bool STORE>
__global__ __launch_bounds__(SSD_THREADS) void ssd_forward_kernel(const float *__restrict__ x, const float *__restrict__ A_log,
                                                                  const float *__restrict__ Dk, const float *__restrict__ dt_bias,
                                                                  float *__restrict__ y, float *__restrict__ ws, SsdGeo geo) {
  using L = SsdFwdLds<PP, SP, Q>;
  constexpr int LDB = L::LDB, LDX = L::LDX, LDW = L::LDW, ST = SP / 16, NST = (PP / 16) * ST / SSD_WAVES, QT = Q / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char ssd_smem[];
  double *sDd = reinterpret_cast<double *>(ssd_smem), *sL = sDd + Q;
  float *sB = reinterpret_cast<float *>(sL + Q), *sC = sB + Q * LDB, *sX = sC + Q * LDB, *sW = sX + Q * LDX, *sH = sW + Q * LDW;
  float *sDl = sH + PP * LDB, *sSg = sDl + Q, *sEL = sSg + Q, *sER = sEL + Q;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int P = geo.P, S = geo.S;
  const int64_t T = geo.T, H = geo.H, Wd = geo.Wd, h = blockIdx.x % H, n = blockIdx.x / H, grp = h / geo.hpg;
  const int64_t offX = h * P, offdt = H * P + h, offB = H * P + H + grp * S, offC = offB + (int64_t)geo.G * S;
  const double A = -exp((double)A_log[h]), bias = (double)dt_bias[h];
  const float dk = Dk[h];
  const int64_t nchunk = (T + Q - 1) / Q;

  ssd_f32x4 hs[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) hs[i] = ssd_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t c = 0; c < nchunk; ++c) {
    const int64_t t0 = c * Q;
    const int len = T - t0 < Q ? (int)(T - t0) : Q;
    const float *row0 = x + (n * T + t0) * Wd;
    __syncthreads();   // the previous chunk has been read
    ssd_load<Q, SP>(sB, row0, Wd, offB, S, len);
    ssd_load<Q, PP>(sX, row0, Wd, offX, P, len);
    if constexpr (!STORE) {
      ssd_load<Q, SP>(sC, row0, Wd, offC, S, len);
#pragma unroll
      for (int i = 0; i < NST; ++i) {
        const int id = wave + SSD_WAVES * i, p0 = 16 * (id / ST), s0 = 16 * (id % ST);
#pragma unroll
        for (int e = 0; e < 4; ++e) sH[(p0 + 4 * q + e) * LDB + s0 + r] = hs[i][e];
      }
    }
    ssd_stage_scalars<Q>(row0, Wd, offdt, bias, A, len, geo.softplus, sDd, sL, sDl, sSg, sEL, sER);
    if constexpr (!STORE) {
      for (int id = wave; id < QT * QT; id += SSD_WAVES) {
        const int rt = id / QT, ct = id % QT;
        ssd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (ct <= rt) acc = ssd_tile<false, true>(sC, LDB, sB, LDB, 16 * rt, 16 * ct, SP, lane, acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int tr = 16 * rt + 4 * q + e, ts = 16 * ct + r;
          sW[tr * LDW + ts] = ts <= tr ? expf((float)(sL[tr] - sL[ts])) * acc[e] * sDl[ts] : 0.f;
        }
      }
      __syncthreads();
      for (int id = wave; id < QT * (PP / 16); id += SSD_WAVES) {
        const int tt = id / (PP / 16), pt = id % (PP / 16);
        ssd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = ssd_tile<false, true>(sC, LDB, sH, LDB, 16 * tt, 16 * pt, SP, lane, acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] *= sEL[16 * tt + 4 * q + e];
        acc = ssd_tile<false, false>(sW, LDW, sX, LDX, 16 * tt, 16 * pt, 16 * (tt + 1), lane, acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t = 16 * tt + 4 * q + e, p = 16 * pt + r;
          if (t < len && p < P) y[((n * T + t0 + t) * H + h) * P + p] = fmaf(dk, sX[t * LDX + p], acc[e]);
        }
      }
      __syncthreads();   // x has been read unscaled
    }
    for (int idx = tid; idx < Q * PP; idx += SSD_THREADS) {
      const int t = idx / PP, p = idx - t * PP;
      sX[t * LDX + p] *= sDl[t] * sER[t];
    }
    __syncthreads();
    const float eQ = sEL[Q - 1];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int id = wave + SSD_WAVES * i, p0 = 16 * (id / ST), s0 = 16 * (id % ST);
      hs[i] = ssd_tile<true, false>(sX, LDX, sB, LDB, p0, s0, Q, lane, hs[i] * eQ);
      if constexpr (STORE) {
        if (c + 1 < nchunk) {
          float *dst = ws + ((n * H + h) * (nchunk - 1) + c) * (PP * SP);
#pragma unroll
          for (int e = 0; e < 4; ++e) dst[(p0 + 4 * q + e) * SP + s0 + r] = hs[i][e];
        }
      }
    }
  }
}

template <int PP, int SP> struct SsdRulesLds {
  static constexpr int Q = SSD_RCHUNK, LDB = SP + 4, LDX = PP + 4, LDW = Q + 4;
  static constexpr int SMALL = 6 * Q + (2 * (SP / 16) + PP / 16 + Q / 16 + 3) * Q + SSD_WAVES;
  static constexpr int FLOATS = 2 * Q * LDB + 2 * Q * LDX + 3 * Q * LDW + 2 * PP * LDB + SMALL;
  static constexpr int BYTES = 2 * Q * 8 + FLOATS * 4;
};

template <int PP, int SP>
__global__ __launch_bounds__(SSD_THREADS) void ssd_rules_kernel(const float *__restrict__ M, const float *__restrict__ x,
                                                                const float *__restrict__ A_log, const float *__restrict__ Dk,
                                                                const float *__restrict__ dt_bias, float *__restrict__ g,
                                                                float *__restrict__ F_A, float *__restrict__ F_Dk,
                                                                float *__restrict__ F_dtb, const float *__restrict__ ws,
                                                                float *__restrict__ part, SsdGeo geo) {
  using L = SsdRulesLds<PP, SP>;
  constexpr int Q = L::Q, LDB = L::LDB, LDX = L::LDX, LDW = L::LDW, ST = SP / 16, PT = PP / 16, QT = Q / 16;
  constexpr int NST = PT * ST / SSD_WAVES;
  extern __shared__ __attribute__((aligned(16))) unsigned char ssd_smem[];
  double *sDd = reinterpret_cast<double *>(ssd_smem), *sL = sDd + Q;
  float *sB = reinterpret_cast<float *>(sL + Q), *sC = sB + Q * LDB, *sX = sC + Q * LDB, *sM = sX + Q * LDX;
  float *sW = sM + Q * LDX, *sG = sW + Q * LDW, *sZ = sG + Q * LDW, *sH = sZ + Q * LDW, *sLt = sH + PP * LDB;
  float *sDl = sLt + PP * LDB, *sSg = sDl + Q, *sEL = sSg + Q, *sER = sEL + Q, *sq = sER + Q, *sp = sq + Q;
  float *sQp = sp + Q, *sPp = sQp + ST * Q, *sXp = sPp + ST * Q, *sRp = sXp + PT * Q, *sFin = sRp + QT * Q, *sRed = sFin + 3 * Q;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int P = geo.P, S = geo.S;
  const int64_t V = geo.V, N = geo.N, T = geo.T, H = geo.H, Wd = geo.Wd;
  const int64_t h = blockIdx.x % H, n = (blockIdx.x / H) % N, v = blockIdx.x / H / N, grp = h / geo.hpg, hl = h % geo.hpg;
  const int64_t offX = h * P, offdt = H * P + h, offB = H * P + H + grp * S, offC = offB + (int64_t)geo.G * S;
  const double A = -exp((double)A_log[h]), bias = (double)dt_bias[h];
  const float Af = (float)A, dk = Dk[h];
  const bool wantG = geo.want & 1, full = geo.want != 4;
  const int64_t nchunk = geo.nchunk;

  ssd_f32x4 lt[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) lt[i] = ssd_f32x4{0.f, 0.f, 0.f, 0.f};
  float fa = 0.f, fd = 0.f, fb = 0.f;   // of step tid of every chunk (tid < Q)

  for (int64_t c = nchunk - 1; c >= 0; --c) {
    const int64_t t0 = c * Q;
    const int len = T - t0 < Q ? (int)(T - t0) : Q;
    const float *row0 = x + (n * T + t0) * Wd;
    float *grow0 = wantG ? g + ((v * N + n) * T + t0) * Wd : nullptr;
    __syncthreads();   // the previous chunk has been read
    ssd_load<Q, PP>(sX, row0, Wd, offX, P, len);
    ssd_load<Q, PP>(sM, M + ((v * N + n) * T + t0) * (H * P), H * P, offX, P, len);
    if (full) {
      ssd_load<Q, SP>(sB, row0, Wd, offB, S, len);
      ssd_load<Q, SP>(sC, row0, Wd, offC, S, len);
      const float *hin = c > 0 ? ws + ((n * H + h) * (nchunk - 1) + (c - 1)) * (PP * SP) : nullptr;
      for (int idx = tid; idx < PP * SP; idx += SSD_THREADS) {
        const int p = idx / SP, s = idx - p * SP;
        sH[p * LDB + s] = hin ? hin[idx] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < NST; ++i) {
        const int id = wave + SSD_WAVES * i, p0 = 16 * (id / ST), s0 = 16 * (id % ST);
#pragma unroll
        for (int e = 0; e < 4; ++e) sLt[(p0 + 4 * q + e) * LDB + s0 + r] = lt[i][e];
      }
    }
    ssd_stage_scalars<Q>(row0, Wd, offdt, bias, A, len, geo.softplus, sDd, sL, sDl, sSg, sEL, sER);
    if (tid < Q) {
      for (int p = 0; p < PP; ++p) fd = fmaf(sM[tid * LDX + p], sX[tid * LDX + p], fd);
    }
    if (!full) continue;   // (uniform over the workgroup)

    // ---- W, G, Z
    for (int id = wave; id < QT * QT; id += SSD_WAVES) {
      const int rt = id / QT, ct = id % QT;
      ssd_f32x4 cb = {0.f, 0.f, 0.f, 0.f}, mx = {0.f, 0.f, 0.f, 0.f};
      if (ct <= rt) {
        cb = ssd_tile<false, true>(sC, LDB, sB, LDB, 16 * rt, 16 * ct, SP, lane, cb);
        mx = ssd_tile<false, true>(sM, LDX, sX, LDX, 16 * rt, 16 * ct, PP, lane, mx);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int tr = 16 * rt + 4 * q + e, ts = 16 * ct + r;
        const float d = ts <= tr ? expf((float)(sL[tr] - sL[ts])) : 0.f;
        const float m = mx[e] * sDl[ts], w = d * cb[e];
        sW[tr * LDW + ts] = w;
        sG[tr * LDW + ts] = d * m;
        sZ[tr * LDW + ts] = w * m;
      }
    }
    __syncthreads();

    // ---- LB = Lam_t B_t: g_x and the row sums of x o LB
    for (int id = wave; id < QT * PT; id += SSD_WAVES) {
      const int tt = id / PT, pt = id % PT;
      ssd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = ssd_tile<false, true>(sB, LDB, sLt, LDB, 16 * tt, 16 * pt, SP, lane, acc);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] *= sER[16 * tt + 4 * q + e];
      acc = ssd_tile<true, false>(sW, LDW, sM, LDX, 16 * tt, 16 * pt, Q, lane, acc);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = 16 * tt + 4 * q + e, p = 16 * pt + r;
        if (wantG && t < len && p < P) grow0[(int64_t)t * Wd + offX + p] = fmaf(sDl[t], acc[e], dk * sM[t * LDX + p]);
        const float sum = ssd_red16(sX[t * LDX + p] * acc[e]);
        if (r == 0) sXp[pt * Q + t] = sum;
      }
    }
    // ---- MH = M Hin (g_C, q) and XL = X Lt (g_B, p)
    for (int id = wave; id < 2 * QT * ST; id += SSD_WAVES) {
      const bool isB = id >= QT * ST;
      const int jd = isB ? id - QT * ST : id, tt = jd / ST, st = jd % ST;
      ssd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = isB ? ssd_tile<false, false>(sX, LDX, sLt, LDB, 16 * tt, 16 * st, PP, lane, acc)
                : ssd_tile<false, false>(sM, LDX, sH, LDB, 16 * tt, 16 * st, PP, lane, acc);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = 16 * tt + 4 * q + e, s = 16 * st + r;
        const float sum = ssd_red16((isB ? sB : sC)[t * LDB + s] * acc[e]);
        if (r == 0) (isB ? sPp : sQp)[st * Q + t] = sum;
        acc[e] *= isB ? sER[t] * sDl[t] : sEL[t];
      }
      if (wantG) {
        acc = isB ? ssd_tile<true, false>(sG, LDW, sC, LDB, 16 * tt, 16 * st, Q, lane, acc)
                  : ssd_tile<false, false>(sG, LDW, sB, LDB, 16 * tt, 16 * st, Q, lane, acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t = 16 * tt + 4 * q + e, s = 16 * st + r;
          if (t < len && s < S) {
            if (geo.hpg == 1)
              grow0[(int64_t)t * Wd + (isB ? offB : offC) + s] = acc[e];
            else
              part[((((hl * V + v) * N + n) * T + t0 + t) * geo.G + grp) * (2 * S) + (isB ? 0 : S) + s] = acc[e];
          }
        }
      }
    }
    // ---- R_t = sum_{r >= t > s} Z_rs
    for (int id = wave; id < QT * QT; id += SSD_WAVES) {
      const int rt = id / QT, tt = id % QT;
      ssd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (tt <= rt) {
        const float *a = sZ + (16 * rt + r) * LDW + q;
        for (int k = 0; k < Q; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], k + q < 16 * tt + r ? 1.f : 0.f, acc, 0, 0, 0);
      }
      float sum = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += 16 * rt + 4 * q + e >= 16 * tt + r ? acc[e] : 0.f;
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
      if (q == 0) sRp[rt * Q + 16 * tt + r] = sum;
    }
    // ---- <Lt, Hin>
    {
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < NST; ++i) {
        const int id = wave + SSD_WAVES * i, p0 = 16 * (id / ST), s0 = 16 * (id % ST);
#pragma unroll
        for (int e = 0; e < 4; ++e) sum = fmaf(lt[i][e], sH[(p0 + 4 * q + e) * LDB + s0 + r], sum);
      }
      sum = ssd_red16(sum);
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
      if (lane == 0) sRed[wave] = sum;
    }
    __syncthreads();
    if (tid < Q) {
      float qs = sQp[tid], ps = sPp[tid];
      for (int st = 1; st < ST; ++st) {
        qs += sQp[st * Q + tid];
        ps += sPp[st * Q + tid];
      }
      sq[tid] = sEL[tid] * qs;
      sp[tid] = sER[tid] * sDl[tid] * ps;
    }
    __syncthreads();
    const float eQ = sEL[Q - 1];
    if (tid < Q) {
      float xlb = sXp[tid], R = sRp[tid], suf = 0.f, pre = 0.f;
      for (int pt = 1; pt < PT; ++pt) xlb += sXp[pt * Q + tid];
      for (int rt = 1; rt < QT; ++rt) R += sRp[rt * Q + tid];
      for (int t = Q - 1; t >= tid; --t) suf += sq[t];
      for (int t = 0; t < tid; ++t) pre += sp[t];
      const float cc = eQ * (((sRed[0] + sRed[1]) + sRed[2]) + sRed[3]);
      const float e = ((R + suf) + pre) + cc;
      const float gdt = fmaf(Af, e, xlb) * sSg[tid];
      if (tid < len) {
        if (wantG) grow0[(int64_t)tid * Wd + offdt] = gdt;
        fb += gdt;
        fa = fmaf(e, sDl[tid], fa);
      }
    }
    // ---- Lt of the chunk before
    for (int idx = tid; idx < Q * PP; idx += SSD_THREADS) {
      const int t = idx / PP, p = idx - t * PP;
      sM[t * LDX + p] *= sEL[t];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int id = wave + SSD_WAVES * i, p0 = 16 * (id / ST), s0 = 16 * (id % ST);
      lt[i] = ssd_tile<true, false>(sM, LDX, sC, LDB, p0, s0, Q, lane, lt[i] * eQ);
    }
  }
  __syncthreads();
  if (tid < Q) {
    sFin[tid] = fa;
    sFin[Q + tid] = fd;
    sFin[2 * Q + tid] = fb;
  }
  __syncthreads();
  if (tid < 3) {
    float sum = 0.f;
    for (int t = 0; t < Q; ++t) sum += sFin[tid * Q + t];
    const int64_t o = (v * N + n) * H + h;
    if (tid == 0 && (geo.want & 2)) F_A[o] = Af * sum;
    if (tid == 1 && (geo.want & 4)) F_Dk[o] = sum;
    if (tid == 2 && (geo.want & 8)) F_dtb[o] = sum;
  }
}

// g_B | g_C of g[r] = sum over the heads of a group, ascending, of part[hl][r][grp][2][S];  r < rows = V N T
__global__ __launch_bounds__(256) void ssd_fold_kernel(const float *__restrict__ part, float *__restrict__ g, int64_t rows, int hpg, int G,
                                                       int S, int64_t Wd, int64_t off) {
  const int64_t per = (int64_t)G * 2 * S, total = rows * per;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / per, j = idx - row * per;
    const int grp = (int)(j / (2 * S)), k = (int)(j - (int64_t)grp * 2 * S), isC = k >= S, s = isC ? k - S : k;
    float sum = part[idx];
    for (int b = 1; b < hpg; ++b) sum += part[b * total + idx];
    g[row * Wd + off + (int64_t)isC * G * S + (int64_t)grp * S + s] = sum;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// Sizes and limits both entries share (V = 1 for the forward pass); fills geo when the status is VIVIT_OK.
static int ssd_check(int64_t V, int64_t N, int64_t T, int64_t H, int64_t P, int64_t S, int64_t G, int want, SsdGeo *geo) {
  if (V <= 0 || N <= 0 || T <= 0 || H <= 0 || P <= 0 || S <= 0 || G <= 0 || H % G != 0) return VIVIT_E_BADARG;
  const int64_t lim = 1LL << 30;
  if (S > SSD_MAX_STATE || P > SSD_MAX_HEAD_DIM || V > lim || N > lim || T > lim || H > lim) return VIVIT_E_UNSUPPORTED;
  if (N > 0x7fffffffLL / H || N * H > 0x7fffffffLL / V) return VIVIT_E_UNSUPPORTED;                 // the grid
  const int64_t Wd = H * P + H + 2 * G * S, hpg = H / G;
  if (V * N > (1LL << 56) / T / Wd / hpg) return VIVIT_E_UNSUPPORTED;                               // element offsets and byte counts fit 64 bits
  if (N * H > (1LL << 40) / cdiv(T, SSD_RCHUNK)) return VIVIT_E_UNSUPPORTED;                        // the boundary states' bytes
  *geo = SsdGeo{V, N, T, H, Wd, cdiv(T, SSD_RCHUNK), (int)P, (int)S, (int)G, (int)hpg, 0, want};
  return VIVIT_OK;
}

static size_t ssd_boundary_bytes(const SsdGeo &g) {
  if (g.want == 4) return 0;
  return align_up(sizeof(float) * (size_t)(g.N * g.H) * (size_t)(g.nchunk - 1) * (g.P <= 32 ? 32 : 64) * (g.S <= 64 ? 64 : 128), 256);
}
static size_t ssd_partial_bytes(const SsdGeo &g) {
  if (!(g.want & 1) || g.hpg == 1) return 0;
  return sizeof(float) * (size_t)g.hpg * (size_t)(g.V * g.N * g.T) * (size_t)(2 * g.G * g.S);
}

template <int PP, int SP>
static int ssd_forward_launch(const float *x, const float *A_log, const float *Dk, const float *dt_bias, float *y, const SsdGeo &geo,
                              hipStream_t s) {
  static unsigned long long attr_done = 0;
  constexpr int bytes = SsdFwdLds<PP, SP, SSD_CHUNK>::BYTES;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
  if (!ensure_dynamic_lds(reinterpret_cast<const void *>(ssd_forward_kernel<PP, SP, SSD_CHUNK, false>), bytes, attr_done)) return VIVIT_E_LAUNCH;
  attr_done |= 1ull << (dev & 63);
  ssd_forward_kernel<PP, SP, SSD_CHUNK, false><<<(unsigned)(geo.N * geo.H), SSD_THREADS, bytes, s>>>(x, A_log, Dk, dt_bias, y, nullptr, geo);
  return launch_status();
}

template <int PP, int SP>
static int ssd_rules_launch(const float *M, const float *x, const float *A_log, const float *Dk, const float *dt_bias, float *g, float *F_A,
                            float *F_Dk, float *F_dtb, float *wsH, float *part, const SsdGeo &geo, hipStream_t s) {
  static unsigned long long attr_done = 0;
  constexpr int fbytes = SsdFwdLds<PP, SP, SSD_RCHUNK>::BYTES, rbytes = SsdRulesLds<PP, SP>::BYTES;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
  if (!ensure_dynamic_lds(reinterpret_cast<const void *>(ssd_forward_kernel<PP, SP, SSD_RCHUNK, true>), fbytes, attr_done) ||
      !ensure_dynamic_lds(reinterpret_cast<const void *>(ssd_rules_kernel<PP, SP>), rbytes, attr_done))
    return VIVIT_E_LAUNCH;
  attr_done |= 1ull << (dev & 63);
  if (geo.want != 4 && geo.nchunk > 1) {
    ssd_forward_kernel<PP, SP, SSD_RCHUNK, true><<<(unsigned)(geo.N * geo.H), SSD_THREADS, fbytes, s>>>(x, A_log, Dk, dt_bias, nullptr, wsH, geo);
    if (launch_status() != VIVIT_OK) return VIVIT_E_LAUNCH;
  }
  ssd_rules_kernel<PP, SP><<<(unsigned)(geo.V * geo.N * geo.H), SSD_THREADS, rbytes, s>>>(M, x, A_log, Dk, dt_bias, g, F_A, F_Dk, F_dtb, wsH,
                                                                                         part, geo);
  return launch_status();
}

} // namespace vivit

using namespace vivit;

extern "C" {

int vivit_ssd_forward_f32(const float *x, const float *A_log, const float *Dk, const float *dt_bias, float *y, int64_t N, int64_t T,
                          int64_t H, int64_t P, int64_t S, int64_t G, int delta_softplus, void *stream) {
  if (!x || !A_log || !Dk || !dt_bias || !y) return VIVIT_E_BADARG;
  SsdGeo geo;
  const int st = ssd_check(1, N, T, H, P, S, G, 0, &geo);
  if (st != VIVIT_OK) return st;
  geo.softplus = delta_softplus != 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P <= 32) return S <= 64 ? ssd_forward_launch<32, 64>(x, A_log, Dk, dt_bias, y, geo, s) : ssd_forward_launch<32, 128>(x, A_log, Dk, dt_bias, y, geo, s);
  return S <= 64 ? ssd_forward_launch<64, 64>(x, A_log, Dk, dt_bias, y, geo, s) : ssd_forward_launch<64, 128>(x, A_log, Dk, dt_bias, y, geo, s);
}

size_t vivit_ssd_rules_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t P, int64_t S, int64_t G, int want) {
  SsdGeo geo;
  if (want < 1 || want > 15 || ssd_check(V, N, T, H, P, S, G, want, &geo) != VIVIT_OK) return 0;
  return ssd_boundary_bytes(geo) + ssd_partial_bytes(geo);
}

int vivit_ssd_rules_f32(const float *M, const float *x, const float *A_log, const float *Dk, const float *dt_bias, float *g, float *F_A,
                        float *F_Dk, float *F_dtb, int64_t V, int64_t N, int64_t T, int64_t H, int64_t P, int64_t S, int64_t G,
                        int delta_softplus, int want, void *workspace, size_t workspace_bytes, void *stream) {
  if (want < 1 || want > 15 || !M || !x || !A_log || !Dk || !dt_bias || ((want & 1) && !g) || ((want & 2) && !F_A) ||
      ((want & 4) && !F_Dk) || ((want & 8) && !F_dtb))
    return VIVIT_E_BADARG;
  SsdGeo geo;
  const int st = ssd_check(V, N, T, H, P, S, G, want, &geo);
  if (st != VIVIT_OK) return st;
  geo.softplus = delta_softplus != 0;
  const size_t hb = ssd_boundary_bytes(geo), need = hb + ssd_partial_bytes(geo);
  if (need > 0 && (!workspace || workspace_bytes < need)) return VIVIT_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float *wsH = reinterpret_cast<float *>(workspace);
  float *part = need > hb ? reinterpret_cast<float *>(static_cast<char *>(workspace) + hb) : nullptr;
  int rc;
  if (P <= 32)
    rc = S <= 64 ? ssd_rules_launch<32, 64>(M, x, A_log, Dk, dt_bias, g, F_A, F_Dk, F_dtb, wsH, part, geo, s)
                 : ssd_rules_launch<32, 128>(M, x, A_log, Dk, dt_bias, g, F_A, F_Dk, F_dtb, wsH, part, geo, s);
  else
    rc = S <= 64 ? ssd_rules_launch<64, 64>(M, x, A_log, Dk, dt_bias, g, F_A, F_Dk, F_dtb, wsH, part, geo, s)
                 : ssd_rules_launch<64, 128>(M, x, A_log, Dk, dt_bias, g, F_A, F_Dk, F_dtb, wsH, part, geo, s);
  if (rc != VIVIT_OK || !part) return rc;
  const int64_t rows = V * N * T, blocks = cdiv(rows * 2 * G * S, 256);
  ssd_fold_kernel<<<(unsigned)(blocks < 32768 ? blocks : 32768), 256, 0, s>>>(part, g, rows, geo.hpg, (int)G, (int)S, geo.Wd, H * P + H);
  return launch_status();
}

} // extern "C"
