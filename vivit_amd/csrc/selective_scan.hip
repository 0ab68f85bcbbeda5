// Selective state-space scan (Mamba S6): the forward pass and, from ONE visit of the factor, the input rule and both parameter
// rules.  vivit_selective_scan_forward_f32 and vivit_selective_scan_rules_f32 (include/vivit_hip.h: formulas and layouts).  The
// recurrence is elementwise in (channel d, state s); the only contractions run over s <= 64 (inside a lane) or over the 64
// channels of a block (one wave).  There is no matrix product to hand to the MFMA pipe: do not try MFMA here.  No atomics.
//
// Notation: x [N, T, 2 D + 2 S] = u | dt | B | C, Delta = softplus(dt) or dt, A = -exp(A_log), dA_t = exp(Delta_t A), p_t = dA_t h_{t-1},
// h_t = p_t + (Delta_t u_t) B_t.  S is a compile-time variant SP in {16, 32, 64}; a smaller S is padded with states whose A_log, B, C
// are 0 (they stay 0 and are never stored).  A channel block is SS_CHAN = 64 consecutive d: the lanes of one wave, so that u, dt, M,
// y, g_u and g_dt are read and written coalesced.  Channels beyond D read 0 and are never stored.
//
// PRECISION.  A, Delta and sigmoid(dt) are evaluated in fp64 (once per (d, s) resp. (t, d): 1 / S of the work) and the argument of
// the decay is the fp64 product Delta A rounded once, so that a decay carries |Delta A| 2^-24 from its argument and expf's 1 ulp,
// nothing from softplus or from A.  Everything else is fp32 with explicit fmaf.
//
// FORWARD  ss_forward_kernel<SP>, one wave per (n, channel block).  A lane owns one channel: h[SP] and A[SP] (fp64) in registers.
// Time runs in tiles of SS_FWD_TILE = 8 steps: B_t | C_t of the tile are staged in LDS and read as broadcasts, u and dt of the tile
// are fetched into registers before its first step.  It writes y and nothing else.
// SUMMATION ORDER of y[n, t, d]: sum = +0, s ascending sum = fmaf(C_t[s], h_t[s], sum), then fmaf(Dk, u, sum).
//
// RULES  ss_rules_kernel<SP, WG, WA>, 256 lanes = SS_WAVES = 4 waves.  A workgroup owns (n, channel block, group of 4 factor
// columns) for the whole sequence; time is cut in chunks of L = 128 / SP steps (SS_CHUNK = 8 at SP = 16; 4; 2).
//   Phase 1 (forward sweep): thread (d = tid & 63, q = tid >> 6) owns the SP / 4 states q SP / 4 .. of channel d and writes h at the
//   start of every chunk but the first to the workspace.
//   Phase 2 (chunks in reverse): the same threads recompute, from the chunk's boundary state, dA_t and p_t of every step into LDS
//   ([t][s][d], d fastest: conflict-free for a wave that reads one s).  Then wave w serves column v = 4 group + w: lane = channel,
//   the carried adjoint dA_{t+1} a_{t+1} [SP], the sums of F_A [SP] and of F_Dk live in registers across all chunks; dA, p come
//   from LDS, B_t, C_t and the per-(t, d) values Delta, u, Delta u, sigmoid as staged; h_t is fmaf(Delta u, B, p) again.  One
//   recomputation of h serves the four columns.  g_B / g_C: per step and 16 states, the 64 channels are folded by a
//   transpose-reduce (ss_fold16: at xor 32, 16, 8, 4 the partners halve what they hold, then xor 2, 1 add: 17 exchanges per 16
//   values); one channel block writes them into g, several write partials that ss_fold_kernel adds in ascending block order.
// LDS of a workgroup: dA and p 2 x 128 x 64 x 4 = 65536 B, Delta (fp64) 8 x 64 x 8 = 4096 B, Delta, u, Delta u, sigmoid (fp32)
// 4 x 8 x 64 x 4 = 8192 B, B and C 2 x 128 x 4 = 1024 B: 78848 B, so that TWO workgroups share the 163840 B of a compute unit.
// SUMMATION ORDERS (t runs from T - 1 down to 0 wherever it is summed; s ascending; every sum starts at +0):
//   a_t[s] = fmaf(C_t[s], M_t, fl(dA_{t+1}[s] a_{t+1}[s]));  e = fl(a p);  sB = fmaf(a, B[s], sB);  sA = fmaf(e, A[s], sA)
//   g_u = fmaf(Delta, sB, fl(Dk M));  g_dt = fl(fmaf(u, sB, sA) sigmoid);  F_A[d, s] = fl(A[s] sum_t fmaf(e, Delta, .));
//   F_Dk[d] = sum_t fmaf(M, u, .);  g_B[t, s]: terms fl(a fl(Delta u)), g_C[t, s]: terms fl(M h_t[s]), the 64 channels of a block by the
//   tree of ss_fold16, then the blocks ascending.
// The plan (chunks, blocks, groups) is a function of the sizes alone and `want` only removes work: the bytes of every result are a
// function of the arguments, the same on every run and for every `want`.
// want == 4 (F_Dk alone) takes ss_fdk_kernel (one thread per (v, n, d), the same order).  All element offsets are 64-bit.
// (vivit_amd/kernels.py repeats SS_CHUNK, SS_CHAN and SS_WAVES for the tests that name the edges: change them together.)
#include "common.h"

namespace vivit {

constexpr int SS_CHAN = 64, SS_WAVES = 4, SS_THREADS = SS_CHAN * SS_WAVES;
constexpr int SS_TILE = 128;                      // L SP: (step, state) pairs of a chunk
constexpr int SS_CHUNK = SS_TILE / 16;            // L of the smallest variant (the longest chunk)
constexpr int SS_FWD_TILE = 8;
constexpr int SS_MAX_STATE = 64;
constexpr int SS_LDS_BYTES = 2 * SS_TILE * SS_CHAN * 4 + SS_CHUNK * SS_CHAN * (8 + 4 * 4) + 2 * SS_TILE * 4;
static_assert(2 * SS_LDS_BYTES <= 160 * 1024, "two workgroups per compute unit");
// SP = 64 keeps A [SP][64] in LDS as well (16 KB more; its registers allow one workgroup per compute unit anyway): carry, F_A and A
// at 64 registers each do not fit the 512 of a lane next to the operands of a step.  (Build output: every variant is free of scratch
// except <64, input rule, F_A> together, which spills 46 registers, 188 B per lane.)
constexpr int ss_lds_bytes(int SP) { return SS_LDS_BYTES + (SP > 32 ? SP * SS_CHAN * 4 : 0); }

struct SsGeo {
  int64_t V, N, T, D, nchunk;
  int S, softplus, want, nblk, ngrp;
};

__device__ inline double ss_softplus(double v) { return v > 0.0 ? v + log1p(exp(-v)) : log1p(exp(v)); }
__device__ inline double ss_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

template <int SP>
__global__ __launch_bounds__(SS_CHAN) void ss_forward_kernel(const float *__restrict__ x, const float *__restrict__ A_log,
                                                             const float *__restrict__ Dk, float *__restrict__ y, SsGeo geo) {
  __shared__ float sBC[SS_FWD_TILE][2 * SP];
  const int lane = threadIdx.x, S = geo.S;
  const int64_t blk = blockIdx.x % geo.nblk, n = blockIdx.x / geo.nblk, D = geo.D, T = geo.T, W = 2 * D + 2 * S;
  const int64_t d = blk * SS_CHAN + lane;
  const bool dok = d < D;
  double A[SP];
  float h[SP];
#pragma unroll
  for (int s = 0; s < SP; ++s) {
    A[s] = -exp((double)(dok && s < S ? A_log[d * S + s] : 0.f));
    h[s] = 0.f;
  }
  const float dk = dok ? Dk[d] : 0.f;
  for (int64_t t0 = 0; t0 < T; t0 += SS_FWD_TILE) {
    const int len = T - t0 < SS_FWD_TILE ? (int)(T - t0) : SS_FWD_TILE;
    const float *row0 = x + (n * T + t0) * W;
    __syncthreads();   // the previous tile has been read
    for (int idx = lane; idx < SS_FWD_TILE * 2 * SP; idx += SS_CHAN) {
      const int t = idx / (2 * SP), j = idx - t * 2 * SP, s = j < SP ? j : j - SP;
      sBC[t][j] = (t < len && s < S) ? row0[(int64_t)t * W + 2 * D + (j < SP ? s : S + s)] : 0.f;
    }
    float ur[SS_FWD_TILE], dr[SS_FWD_TILE];
#pragma unroll
    for (int t = 0; t < SS_FWD_TILE; ++t) {
      const bool ok = dok && t < len;
      ur[t] = ok ? row0[(int64_t)t * W + d] : 0.f;
      dr[t] = ok ? row0[(int64_t)t * W + D + d] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < SS_FWD_TILE; ++t) {
      if (t < len) {
        const double dl = geo.softplus ? ss_softplus((double)dr[t]) : (double)dr[t];
        const float du = (float)dl * ur[t];
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < SP; ++s) {
          const float p = expf((float)(dl * A[s])) * h[s];
          h[s] = fmaf(du, sBC[t][s], p);
          sum = fmaf(sBC[t][SP + s], h[s], sum);
        }
        if (dok) y[(n * T + t0 + t) * D + d] = fmaf(dk, ur[t], sum);
      }
    }
  }
}

// Sums of 16 values over the 64 lanes of a wave, a fixed tree (as dw_wave_fold of depthwise.hip): afterwards v[0] of every lane
// is the wave's sum of value (lane >> 2) & 15.
__device__ inline void ss_fold16(float (&v)[16], int lane) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int off = 32 >> s, cnt = 8 >> s;
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < cnt; ++i) {
      const float lo = v[i], hi = v[i + cnt];
      const float got = __shfl_xor(up ? lo : hi, off);
      v[i] = (up ? hi : lo) + got;
    }
  }
  v[0] += __shfl_xor(v[0], 2);
  v[0] += __shfl_xor(v[0], 1);
}

template <int SP, bool WG, bool WA>
__global__ __launch_bounds__(SS_THREADS) void ss_rules_kernel(const float *__restrict__ M, const float *__restrict__ x,
                                                              const float *__restrict__ A_log, const float *__restrict__ Dk,
                                                              float *__restrict__ g, float *__restrict__ F_A, float *__restrict__ F_Dk,
                                                              float *__restrict__ wsH, float *__restrict__ part, SsGeo geo) {
  constexpr int L = SS_TILE / SP, SPT = SP / SS_WAVES;
  extern __shared__ __attribute__((aligned(16))) unsigned char ss_smem[];
  double *sDd = reinterpret_cast<double *>(ss_smem);                 // [L][64]  Delta, fp64
  float *sDA = reinterpret_cast<float *>(sDd + SS_CHUNK * SS_CHAN);   // [L][SP][64]
  float *sP = sDA + SS_TILE * SS_CHAN;                                // [L][SP][64]
  float *sDf = sP + SS_TILE * SS_CHAN;                                // [L][64]  Delta
  float *sU = sDf + SS_CHUNK * SS_CHAN;                               // [L][64]  u
  float *sDU = sU + SS_CHUNK * SS_CHAN;                               // [L][64]  fl(Delta u)
  float *sSg = sDU + SS_CHUNK * SS_CHAN;                              // [L][64]  sigmoid(dt), or 1
  float *sB = sSg + SS_CHUNK * SS_CHAN;                               // [L][SP]
  float *sC = sB + SS_TILE;                                           // [L][SP]
  float *sA = sC + SS_TILE;                                           // [SP][64]  A (SP = 64 only)
  constexpr bool A_LDS = SP > 32;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, S = geo.S;
  const int64_t V = geo.V, N = geo.N, T = geo.T, D = geo.D, W = 2 * D + 2 * S;
  const int64_t id = blockIdx.x, grp = id % geo.ngrp, blk = (id / geo.ngrp) % geo.nblk, n = id / geo.ngrp / geo.nblk;
  const int64_t d = blk * SS_CHAN + lane;   // the channel of this thread in both of its roles
  const bool dok = d < D;
  float *hws = wsH + id * (geo.nchunk - 1) * (SP * SS_CHAN);

  double Aq[SPT];   // role 1: the states wave * SPT .. of channel d
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = wave * SPT + j;
    Aq[j] = -exp((double)(dok && s < S ? A_log[d * S + s] : 0.f));
    if constexpr (A_LDS) sA[s * SS_CHAN + lane] = (float)Aq[j];   // (read after the barriers of phase 2)
  }

  auto stage = [&](int64_t t0, int len) {
    const float *row0 = x + (n * T + t0) * W;
    for (int idx = tid; idx < L * SS_CHAN; idx += SS_THREADS) {
      const int t = idx >> 6;
      const int64_t dd = blk * SS_CHAN + (idx & 63);
      float u = 0.f, dt = 0.f;
      if (t < len && dd < D) {
        u = row0[(int64_t)t * W + dd];
        dt = row0[(int64_t)t * W + D + dd];
      }
      const double dl = geo.softplus ? ss_softplus((double)dt) : (double)dt;
      const float dlf = (float)dl;
      sDd[idx] = dl;
      sDf[idx] = dlf;
      sU[idx] = u;
      sDU[idx] = dlf * u;
      sSg[idx] = geo.softplus ? (float)ss_sigmoid((double)dt) : 1.f;
    }
    for (int idx = tid; idx < L * SP; idx += SS_THREADS) {
      const int t = idx / SP, s = idx - t * SP;
      const bool ok = t < len && s < S;
      sB[idx] = ok ? row0[(int64_t)t * W + 2 * D + s] : 0.f;
      sC[idx] = ok ? row0[(int64_t)t * W + 2 * D + S + s] : 0.f;
    }
  };
  // role 1: h of this thread's states through the staged chunk; WRITE: dA and p of every step to LDS
  auto advance = [&](float (&h)[SPT], int len, bool write) {
    for (int t = 0; t < len; ++t) {
      const double dl = sDd[t * SS_CHAN + lane];
      const float du = sDU[t * SS_CHAN + lane];
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        const int s = wave * SPT + j;
        const float dA = expf((float)(dl * Aq[j]));
        const float p = dA * h[j];
        if (write) {
          sDA[(t * SP + s) * SS_CHAN + lane] = dA;
          sP[(t * SP + s) * SS_CHAN + lane] = p;
        }
        h[j] = fmaf(du, sB[t * SP + s], p);
      }
    }
  };

  // ---- phase 1: h at the start of the chunks 1 .. nchunk - 1
  {
    float h[SPT];
#pragma unroll
    for (int j = 0; j < SPT; ++j) h[j] = 0.f;
    for (int64_t c = 0; c + 1 < geo.nchunk; ++c) {
      __syncthreads();   // the previous chunk has been read
      stage(c * L, L);
      __syncthreads();
      advance(h, L, false);
#pragma unroll
      for (int j = 0; j < SPT; ++j) hws[c * (SP * SS_CHAN) + (wave * SPT + j) * SS_CHAN + lane] = h[j];
    }
  }

  // ---- phase 2: role 2, lane = channel, wave = column
  const int64_t v = grp * SS_WAVES + wave;
  const bool active = v < V;
  float Af[A_LDS ? 1 : SP], carry[SP], FA[WA ? SP : 1];
  float FD = 0.f;
#pragma unroll
  for (int s = 0; s < SP; ++s) {
    if constexpr (!A_LDS) Af[s] = (float)(-exp((double)(dok && s < S ? A_log[d * S + s] : 0.f)));
    carry[s] = 0.f;
    if constexpr (WA) FA[s] = 0.f;
  }
  const float dk = dok ? Dk[d] : 0.f;
  for (int64_t c = geo.nchunk - 1; c >= 0; --c) {
    const int64_t t0 = c * L;
    const int len = T - t0 < L ? (int)(T - t0) : L;
    __syncthreads();   // the previous chunk (or phase 1) has been read
    stage(t0, len);
    __syncthreads();
    {
      float h[SPT];
#pragma unroll
      for (int j = 0; j < SPT; ++j) h[j] = c > 0 ? hws[(c - 1) * (SP * SS_CHAN) + (wave * SPT + j) * SS_CHAN + lane] : 0.f;
      advance(h, len, true);
    }
    __syncthreads();
    if (!active) continue;   // (wave-uniform; no barrier below)
    const float *Mrow0 = M + ((v * N + n) * T + t0) * D;
    float m_next = dok ? Mrow0[(int64_t)(len - 1) * D + d] : 0.f;
#pragma unroll 1
    for (int t = len - 1; t >= 0; --t) {
      const float m = m_next;
      m_next = (dok && t > 0) ? Mrow0[(int64_t)(t - 1) * D + d] : 0.f;   // (fetched a step ahead)
      const float dlf = sDf[t * SS_CHAN + lane], u = sU[t * SS_CHAN + lane], du = sDU[t * SS_CHAN + lane];
      FD = fmaf(m, u, FD);
      float sBsum = 0.f, sAsum = 0.f;
      float *grow = WG ? g + ((v * N + n) * T + t0 + t) * W : nullptr;
      float *gbc = !WG ? nullptr : geo.nblk == 1 ? grow + 2 * D : part + (((blk * V + v) * N + n) * T + t0 + t) * (2 * S);
#pragma unroll
      for (int s0 = 0; s0 < SP; s0 += 16) {
        float vB[16], vC[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int s = s0 + j;
          const float dA = sDA[(t * SP + s) * SS_CHAN + lane], p = sP[(t * SP + s) * SS_CHAN + lane];
          const float Bs = sB[t * SP + s], Cs = sC[t * SP + s];
          const float a = fmaf(Cs, m, carry[s]);
          const float e = a * p;
          carry[s] = dA * a;
          if constexpr (WA) FA[s] = fmaf(e, dlf, FA[s]);
          if constexpr (WG) {
            sBsum = fmaf(a, Bs, sBsum);
            sAsum = fmaf(e, A_LDS ? sA[s * SS_CHAN + lane] : Af[A_LDS ? 0 : s], sAsum);
            vB[j] = a * du;
            vC[j] = m * fmaf(du, Bs, p);
          }
        }
        if constexpr (WG) {
          ss_fold16(vB, lane);
          ss_fold16(vC, lane);
          const int s = s0 + (lane >> 2);
          if ((lane & 3) == 0 && s < S) {
            gbc[s] = vB[0];
            gbc[S + s] = vC[0];
          }
        }
      }
      if (WG && dok) {
        grow[d] = fmaf(dlf, sBsum, dk * m);
        grow[D + d] = fmaf(u, sBsum, sAsum) * sSg[t * SS_CHAN + lane];
      }
    }
  }
  if (active && dok) {
    if constexpr (WA) {
      float *fa = F_A + ((v * N + n) * D + d) * S;
#pragma unroll
      for (int s = 0; s < SP; ++s)
        if (s < S) fa[s] = (A_LDS ? sA[s * SS_CHAN + lane] : Af[A_LDS ? 0 : s]) * FA[s];
    }
    if (geo.want & 4) F_Dk[(v * N + n) * D + d] = FD;
  }
}

// g[r, 2 D + j] = sum over the channel blocks, ascending, of part[b][r][j];  r < rows = V N T, j < 2 S
__global__ __launch_bounds__(256) void ss_fold_kernel(const float *__restrict__ part, float *__restrict__ g, int64_t rows, int nblk, int S2,
                                                      int64_t W, int64_t off) {
  const int64_t total = rows * S2;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t r = idx / S2, j = idx - r * S2;
    float sum = part[idx];
    for (int b = 1; b < nblk; ++b) sum += part[b * total + idx];
    g[r * W + off + j] = sum;
  }
}

// F_Dk alone: one thread per (v, n, d), t from T - 1 down to 0 as the rules kernel sums it
__global__ __launch_bounds__(256) void ss_fdk_kernel(const float *__restrict__ M, const float *__restrict__ x, float *__restrict__ F_Dk,
                                                     SsGeo geo) {
  const int64_t D = geo.D, T = geo.T, W = 2 * D + 2 * geo.S, total = geo.V * geo.N * D;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t d = idx % D, vn = idx / D, n = vn % geo.N;
    float sum = 0.f;
    for (int64_t t = T - 1; t >= 0; --t) sum = fmaf(M[(vn * T + t) * D + d], x[(n * T + t) * W + d], sum);
    F_Dk[idx] = sum;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static int ss_variant(int64_t S) { return S <= 16 ? 16 : S <= 32 ? 32 : 64; }

// Sizes and limits both entries share (V = 1 for the forward pass); fills geo when the status is VIVIT_OK.
static int ss_check(int64_t V, int64_t N, int64_t T, int64_t D, int64_t S, int want, SsGeo *geo) {
  if (V <= 0 || N <= 0 || T <= 0 || D <= 0 || S <= 0) return VIVIT_E_BADARG;
  const int64_t lim = 1LL << 30;
  if (S > SS_MAX_STATE || V > lim || N > lim || T > lim || D > lim) return VIVIT_E_UNSUPPORTED;
  const int64_t nblk = cdiv(D, SS_CHAN), ngrp = cdiv(V, SS_WAVES), L = SS_TILE / ss_variant(S);
  if (nblk > 0x7fffffffLL / N || nblk * N > 0x7fffffffLL / ngrp) return VIVIT_E_UNSUPPORTED;        // the grid
  if (V * N > (1LL << 56) / T / (2 * D + 2 * S) / nblk) return VIVIT_E_UNSUPPORTED;                 // element offsets and byte counts fit 64 bits
  if (nblk * N * ngrp > (1LL << 44) / cdiv(T, L)) return VIVIT_E_UNSUPPORTED;                        // the boundary states' bytes
  *geo = SsGeo{V, N, T, D, cdiv(T, L), (int)S, 0, want, (int)nblk, (int)ngrp};
  return VIVIT_OK;
}

// workspace: h at the chunk starts [workgroup][nchunk - 1][SP][64], then (several channel blocks, input rule) the partial sums of
// g_B | g_C [block][V][N][T][2 S]
static size_t ss_boundary_bytes(const SsGeo &g) {
  if (!(g.want & 3)) return 0;
  return align_up(sizeof(float) * (size_t)(g.N * g.nblk * g.ngrp) * (size_t)(g.nchunk - 1) * ss_variant(g.S) * SS_CHAN, 256);
}
static size_t ss_partial_bytes(const SsGeo &g) {
  if (!(g.want & 1) || g.nblk == 1) return 0;
  return sizeof(float) * (size_t)g.nblk * (size_t)(g.V * g.N * g.T) * (2 * g.S);
}

template <int SP>
static int ss_rules_launch(const float *M, const float *x, const float *A_log, const float *Dk, float *g, float *F_A, float *F_Dk,
                           float *wsH, float *part, const SsGeo &geo, hipStream_t s) {
  static unsigned long long attr_done = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
  if (!ensure_dynamic_lds(reinterpret_cast<const void *>(ss_rules_kernel<SP, true, true>), ss_lds_bytes(SP), attr_done) ||
      !ensure_dynamic_lds(reinterpret_cast<const void *>(ss_rules_kernel<SP, true, false>), ss_lds_bytes(SP), attr_done) ||
      !ensure_dynamic_lds(reinterpret_cast<const void *>(ss_rules_kernel<SP, false, true>), ss_lds_bytes(SP), attr_done))
    return VIVIT_E_LAUNCH;
  attr_done |= 1ull << (dev & 63);
  const unsigned grid = (unsigned)(geo.N * geo.nblk * geo.ngrp);
  if ((geo.want & 3) == 3)
    ss_rules_kernel<SP, true, true><<<grid, SS_THREADS, ss_lds_bytes(SP), s>>>(M, x, A_log, Dk, g, F_A, F_Dk, wsH, part, geo);
  else if (geo.want & 1)
    ss_rules_kernel<SP, true, false><<<grid, SS_THREADS, ss_lds_bytes(SP), s>>>(M, x, A_log, Dk, g, F_A, F_Dk, wsH, part, geo);
  else
    ss_rules_kernel<SP, false, true><<<grid, SS_THREADS, ss_lds_bytes(SP), s>>>(M, x, A_log, Dk, g, F_A, F_Dk, wsH, part, geo);
  return launch_status();
}

} // namespace vivit

using namespace vivit;

extern "C" {

int vivit_selective_scan_forward_f32(const float *x, const float *A_log, const float *Dk, float *y, int64_t N, int64_t T, int64_t D,
                                     int64_t S, int delta_softplus, void *stream) {
  if (!x || !A_log || !Dk || !y) return VIVIT_E_BADARG;
  SsGeo geo;
  const int st = ss_check(1, N, T, D, S, 0, &geo);
  if (st != VIVIT_OK) return st;
  geo.softplus = delta_softplus != 0;
  const unsigned grid = (unsigned)(N * geo.nblk);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (ss_variant(S)) {
    case 16: ss_forward_kernel<16><<<grid, SS_CHAN, 0, s>>>(x, A_log, Dk, y, geo); break;
    case 32: ss_forward_kernel<32><<<grid, SS_CHAN, 0, s>>>(x, A_log, Dk, y, geo); break;
    default: ss_forward_kernel<64><<<grid, SS_CHAN, 0, s>>>(x, A_log, Dk, y, geo); break;
  }
  return launch_status();
}

size_t vivit_selective_scan_rules_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t D, int64_t S, int want) {
  SsGeo geo;
  if (want < 1 || want > 7 || ss_check(V, N, T, D, S, want, &geo) != VIVIT_OK) return 0;
  return ss_boundary_bytes(geo) + ss_partial_bytes(geo);
}

int vivit_selective_scan_rules_f32(const float *M, const float *x, const float *A_log, const float *Dk, float *g, float *F_A, float *F_Dk,
                                   int64_t V, int64_t N, int64_t T, int64_t D, int64_t S, int delta_softplus, int want, void *workspace,
                                   size_t workspace_bytes, void *stream) {
  if (want < 1 || want > 7 || !M || !x || !A_log || !Dk || ((want & 1) && !g) || ((want & 2) && !F_A) || ((want & 4) && !F_Dk))
    return VIVIT_E_BADARG;
  SsGeo geo;
  const int st = ss_check(V, N, T, D, S, want, &geo);
  if (st != VIVIT_OK) return st;
  geo.softplus = delta_softplus != 0;
  const size_t hb = ss_boundary_bytes(geo), need = hb + ss_partial_bytes(geo);
  if (need > 0 && (!workspace || workspace_bytes < need)) return VIVIT_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (want == 4) {
    const int64_t blocks = cdiv(V * N * D, 256);
    ss_fdk_kernel<<<(unsigned)(blocks < 32768 ? blocks : 32768), 256, 0, s>>>(M, x, F_Dk, geo);
    return launch_status();
  }
  float *wsH = reinterpret_cast<float *>(workspace);
  float *part = need > hb ? reinterpret_cast<float *>(static_cast<char *>(workspace) + hb) : nullptr;
  int rc;
  switch (ss_variant(S)) {
    case 16: rc = ss_rules_launch<16>(M, x, A_log, Dk, g, F_A, F_Dk, wsH, part, geo, s); break;
    case 32: rc = ss_rules_launch<32>(M, x, A_log, Dk, g, F_A, F_Dk, wsH, part, geo, s); break;
    default: rc = ss_rules_launch<64>(M, x, A_log, Dk, g, F_A, F_Dk, wsH, part, geo, s); break;
  }
  if (rc != VIVIT_OK || !part) return rc;
  const int64_t rows = V * N * T, blocks = cdiv(rows * 2 * S, 256);
  ss_fold_kernel<<<(unsigned)(blocks < 32768 ? blocks : 32768), 256, 0, s>>>(part, g, rows, geo.nblk, (int)(2 * S), 2 * D + 2 * S, 2 * D);
  return launch_status();
}

} // extern "C"
