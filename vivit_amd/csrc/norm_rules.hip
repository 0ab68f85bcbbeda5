// LayerNorm and GroupNorm: the rules of the sqrt-GGN factor (f1).  A normalisation ROW is the set of L contiguous elements that
// share one mean and variance: LayerNorm on [N, *extra, *D] has rows = N A (A = prod(extra)) of L = prod(D) elements, GroupNorm(G, C)
// on [N, C, *spatial] has rows = N G of L = (C / G) S elements (S = prod(spatial)).  Per row
//   xhat = (x - mean) rstd,  rstd = 1 / sqrt(var + eps) with the biased variance,  h = gamma o M  (gamma = 1 without affine parameters),
// and the index of gamma inside a row is (row % G) (L / S) + l / S  (LayerNorm: G = 1, S = 1).
//   norm_stats_*:  mean, rstd per row, two-pass (mean first, then sum (x - mean)^2)
//   norm_rules_*:  input rule  out = rstd (h - mean_l(h) - xhat mean_l(h o xhat))  and the segment sums
//                  seg_w[row, j] = sum_{s < S} M xhat,  seg_b[row, j] = sum_{s < S} M  over the L / S segments of the row
//   norm_position_sums_kernel:  LayerNorm with A > 1:  pw[v, n, d] = sum_a M xhat,  pb[v, n, d] = sum_a M
// Routes: a row of L <= NORM_WAVE_L elements is held in the registers of ONE wavefront (16 elements per lane, four rows per
// workgroup); a longer row belongs to one workgroup of 256 threads whose second sweep over M and x comes from cache.  Each route
// has a 16-byte body (L % 4 == 0 and every operand 16-byte aligned) and a scalar body.  No atomics; every sum is a per-lane
// serial sum in index order, a butterfly over the 64 lanes and -- on the workgroup route -- the four wave sums added in order, so
// the bytes of a row's results depend on (L, S, body) only: not on V, on the number of rows or on where the row sits in the launch.
#include "common.h"

namespace vivit {

constexpr int NORM_WAVE_L = 1024;   // 16 elements per lane: 32 registers hold the row of M and of x
constexpr int NORM_PER_LANE = NORM_WAVE_L / 64;

__device__ __forceinline__ float wave_sum(float a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
  return a;
}

// sum over the 256 threads of a workgroup, the same bytes in every thread: butterfly per wave, then the four wave sums in order
__device__ __forceinline__ float block_sum(float a, float *red) {
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  a = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return a;
}

// position l of element e of a lane on the wave route: the 16-byte body holds four float4 (e = 4 k + c), the scalar body 16 floats
template <bool VEC>
__device__ __forceinline__ int wave_pos(int lane, int e) {
  return VEC ? 4 * (lane + 64 * (e >> 2)) + (e & 3) : lane + 64 * e;
}

template <bool VEC>
__device__ __forceinline__ void wave_load(const float *__restrict__ p, int L, int lane, float (&v)[NORM_PER_LANE]) {
  if (VEC) {
    const float4 *p4 = reinterpret_cast<const float4 *>(p);
#pragma unroll
    for (int k = 0; k < NORM_PER_LANE / 4; ++k) {
      const int l4 = lane + 64 * k;
      const float4 q = 4 * l4 < L ? p4[l4] : make_float4(0.f, 0.f, 0.f, 0.f);
      v[4 * k] = q.x, v[4 * k + 1] = q.y, v[4 * k + 2] = q.z, v[4 * k + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < NORM_PER_LANE; ++e) v[e] = lane + 64 * e < L ? p[lane + 64 * e] : 0.f;
  }
}

template <bool VEC>
__device__ __forceinline__ void wave_store(float *__restrict__ p, int L, int lane, const float (&v)[NORM_PER_LANE]) {
  if (VEC) {
    float4 *p4 = reinterpret_cast<float4 *>(p);
#pragma unroll
    for (int k = 0; k < NORM_PER_LANE / 4; ++k) {
      const int l4 = lane + 64 * k;
      if (4 * l4 < L) p4[l4] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < NORM_PER_LANE; ++e)
      if (lane + 64 * e < L) p[lane + 64 * e] = v[e];
  }
}

// ---- statistics ---------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void norm_stats_wave_kernel(const float *__restrict__ X, float *__restrict__ mean,
                                                              float *__restrict__ rstd, int64_t rows, int L, float eps) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  float x[NORM_PER_LANE];
  wave_load<VEC>(X + r * L, L, lane, x);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < NORM_PER_LANE; ++e) s += x[e];   // (positions beyond L hold 0)
  const float mu = wave_sum(s) / (float)L;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < NORM_PER_LANE; ++e) {
    const float d = wave_pos<VEC>(lane, e) < L ? x[e] - mu : 0.f;
    q = fmaf(d, d, q);
  }
  const float var = wave_sum(q) / (float)L;
  if (lane == 0) {
    mean[r] = mu;
    rstd[r] = 1.f / sqrtf(var + eps);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void norm_stats_block_kernel(const float *__restrict__ X, float *__restrict__ mean,
                                                               float *__restrict__ rstd, int L, float eps) {
  __shared__ float red[4];
  const float *x = X + (int64_t)blockIdx.x * L;
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  const int tid = threadIdx.x, L4 = L >> 2;
  float s = 0.f;
  if (VEC) {
    for (int l = tid; l < L4; l += 256) {
      const float4 u = x4[l];
      s += u.x, s += u.y, s += u.z, s += u.w;
    }
  } else {
    for (int l = tid; l < L; l += 256) s += x[l];
  }
  const float mu = block_sum(s, red) / (float)L;
  float q = 0.f;
  if (VEC) {
    for (int l = tid; l < L4; l += 256) {   // the second sweep: from cache
      const float4 u = x4[l];
      const float a = u.x - mu, b = u.y - mu, c = u.z - mu, d = u.w - mu;
      q = fmaf(a, a, q), q = fmaf(b, b, q), q = fmaf(c, c, q), q = fmaf(d, d, q);
    }
  } else {
    for (int l = tid; l < L; l += 256) {
      const float d = x[l] - mu;
      q = fmaf(d, d, q);
    }
  }
  const float var = block_sum(q, red) / (float)L;
  if (tid == 0) {
    mean[blockIdx.x] = mu;
    rstd[blockIdx.x] = 1.f / sqrtf(var + eps);
  }
}

// ---- rules ----------------------------------------------------------------------------------------------------------------------
struct NormRow {          // what one row of the rules launch needs besides its pointers
  float mu, rs;
  const float *gamma;     // null: gamma = 1
  uint32_t goff, S;       // gamma index of position l: goff + l / S
};

__device__ __forceinline__ float norm_gamma(const NormRow &c, uint32_t l) {
  return c.gamma ? c.gamma[c.goff + (c.S == 1 ? l : l / c.S)] : 1.f;
}

// Segment sums of one row (S > 1) by `nthreads` threads (64 or 256): W = min(64, the power of two >= S) lanes per segment, each a
// serial sum over s = lane, lane + W, ... and a butterfly over the W lanes; the trip count is the same for every lane of a wave, so
// that the shuffles run with all lanes.  The operands come from cache: the row has just been read.
__device__ __forceinline__ void norm_segment_sums(const float *__restrict__ m, const float *__restrict__ x, const NormRow &c,
                                                  float *__restrict__ sw, float *__restrict__ sb, int nseg, int tid, int nthreads) {
  const int S = (int)c.S;
  int W = 1;
  while (W < S && W < 64) W <<= 1;
  const int groups = nthreads / W, g = tid / W, sl = tid & (W - 1);
  for (int j0 = 0; j0 < nseg; j0 += groups) {
    const int j = j0 + g;
    float aw = 0.f, ab = 0.f;
    if (j < nseg) {
      const float *mj = m + (int64_t)j * S, *xj = x + (int64_t)j * S;
      for (int s = sl; s < S; s += W) {
        const float v = mj[s];
        aw = fmaf(v, (xj[s] - c.mu) * c.rs, aw);
        ab += v;
      }
    }
    for (int off = W >> 1; off > 0; off >>= 1) {
      aw += __shfl_xor(aw, off, 64);
      ab += __shfl_xor(ab, off, 64);
    }
    if (j < nseg && sl == 0) {
      if (sw) sw[j] = aw;
      if (sb) sb[j] = ab;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void norm_rules_wave_kernel(const float *__restrict__ M, const float *__restrict__ X,
                                                              const float *__restrict__ gamma, const float *__restrict__ mean,
                                                              const float *__restrict__ rstd, float *__restrict__ out,
                                                              float *__restrict__ seg_w, float *__restrict__ seg_b, int64_t vrows,
                                                              int64_t rows, int L, int G, int S) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= vrows) return;
  const int lane = threadIdx.x & 63;
  const int64_t rx = r % rows;
  const int nseg = L / S;
  const NormRow c{mean[rx], rstd[rx], gamma, (uint32_t)(rx % G) * (uint32_t)nseg, (uint32_t)S};
  const float *m = M + r * L, *x = X + rx * L;
  float *sw = seg_w ? seg_w + r * nseg : nullptr, *sb = seg_b ? seg_b + r * nseg : nullptr;
  if (out || S == 1) {
    float mv[NORM_PER_LANE], xh[NORM_PER_LANE];
    wave_load<VEC>(m, L, lane, mv);
    wave_load<VEC>(x, L, lane, xh);
#pragma unroll
    for (int e = 0; e < NORM_PER_LANE; ++e) xh[e] = (xh[e] - c.mu) * c.rs;
    if (S == 1 && sw) {
      float t[NORM_PER_LANE];
#pragma unroll
      for (int e = 0; e < NORM_PER_LANE; ++e) t[e] = mv[e] * xh[e];
      wave_store<VEC>(sw, L, lane, t);
    }
    if (S == 1 && sb) wave_store<VEC>(sb, L, lane, mv);
    if (out) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int e = 0; e < NORM_PER_LANE; ++e) {
        const int l = wave_pos<VEC>(lane, e);
        mv[e] = l < L ? norm_gamma(c, (uint32_t)l) * mv[e] : 0.f;   // h; 0 beyond the row
        s1 += mv[e];
        s2 = fmaf(mv[e], xh[e], s2);
      }
      const float c1 = wave_sum(s1) / (float)L, c2 = wave_sum(s2) / (float)L;
#pragma unroll
      for (int e = 0; e < NORM_PER_LANE; ++e) mv[e] = c.rs * ((mv[e] - c1) - xh[e] * c2);
      wave_store<VEC>(out + r * L, L, lane, mv);
    }
  }
  if (S > 1 && (sw || sb)) norm_segment_sums(m, x, c, sw, sb, nseg, lane, 64);
}

template <bool VEC>
__global__ __launch_bounds__(256) void norm_rules_block_kernel(const float *__restrict__ M, const float *__restrict__ X,
                                                               const float *__restrict__ gamma, const float *__restrict__ mean,
                                                               const float *__restrict__ rstd, float *__restrict__ out,
                                                               float *__restrict__ seg_w, float *__restrict__ seg_b, int64_t rows,
                                                               int L, int G, int S) {
  __shared__ float red[4];
  const int64_t r = blockIdx.x, rx = r % rows;
  const int tid = threadIdx.x, nseg = L / S, L4 = L >> 2;
  const NormRow c{mean[rx], rstd[rx], gamma, (uint32_t)(rx % G) * (uint32_t)nseg, (uint32_t)S};
  const float *m = M + r * L, *x = X + rx * L;
  const float4 *m4 = reinterpret_cast<const float4 *>(m), *x4 = reinterpret_cast<const float4 *>(x);
  float *sw = seg_w ? seg_w + r * nseg : nullptr, *sb = seg_b ? seg_b + r * nseg : nullptr;
  float c1 = 0.f, c2 = 0.f;
  if (out) {
    float s1 = 0.f, s2 = 0.f;
    if (VEC) {
      for (int l = tid; l < L4; l += 256) {
        const float4 p = m4[l], u = x4[l];
        const float pv[4] = {p.x, p.y, p.z, p.w}, uv[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float h = norm_gamma(c, (uint32_t)(4 * l + k)) * pv[k];
          s1 += h;
          s2 = fmaf(h, (uv[k] - c.mu) * c.rs, s2);
        }
      }
    } else {
      for (int l = tid; l < L; l += 256) {
        const float h = norm_gamma(c, (uint32_t)l) * m[l];
        s1 += h;
        s2 = fmaf(h, (x[l] - c.mu) * c.rs, s2);
      }
    }
    c1 = block_sum(s1, red) / (float)L;
    c2 = block_sum(s2, red) / (float)L;
  }
  if (out || S == 1) {   // the second sweep over M and x: from cache
    float *o = out ? out + r * L : nullptr;
    if (VEC) {
      float4 *o4 = reinterpret_cast<float4 *>(o), *sw4 = reinterpret_cast<float4 *>(sw), *sb4 = reinterpret_cast<float4 *>(sb);
      for (int l = tid; l < L4; l += 256) {
        const float4 p = m4[l], u = x4[l];
        const float pv[4] = {p.x, p.y, p.z, p.w}, uv[4] = {u.x, u.y, u.z, u.w};
        float ov[4], tv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float xh = (uv[k] - c.mu) * c.rs;
          tv[k] = pv[k] * xh;
          ov[k] = o ? c.rs * ((norm_gamma(c, (uint32_t)(4 * l + k)) * pv[k] - c1) - xh * c2) : 0.f;
        }
        if (o) o4[l] = make_float4(ov[0], ov[1], ov[2], ov[3]);
        if (S == 1 && sw) sw4[l] = make_float4(tv[0], tv[1], tv[2], tv[3]);
        if (S == 1 && sb) sb4[l] = p;
      }
    } else {
      for (int l = tid; l < L; l += 256) {
        const float p = m[l], xh = (x[l] - c.mu) * c.rs;
        if (o) o[l] = c.rs * ((norm_gamma(c, (uint32_t)l) * p - c1) - xh * c2);
        if (S == 1 && sw) sw[l] = p * xh;
        if (S == 1 && sb) sb[l] = p;
      }
    }
  }
  if (S > 1 && (sw || sb)) norm_segment_sums(m, x, c, sw, sb, nseg, tid, 256);
}

// LayerNorm with A > 1 positions per sample: one thread per d, a serial loop over a; neighbouring threads read neighbouring d
__global__ __launch_bounds__(256) void norm_position_sums_kernel(const float *__restrict__ M, const float *__restrict__ X,
                                                                 const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                 float *__restrict__ pw, float *__restrict__ pb, int64_t N, int A, int D,
                                                                 int dblocks) {
  const int64_t vn = blockIdx.x / dblocks, n = vn % N;
  const int d = (int)(blockIdx.x % dblocks) * 256 + threadIdx.x;
  if (d >= D) return;
  const float *m = M + vn * A * D + d, *x = X + n * A * D + d;
  const float *mu = mean + n * A, *rs = rstd + n * A;
  float aw = 0.f, ab = 0.f;
  for (int a = 0; a < A; ++a) {
    const float v = m[(int64_t)a * D];
    aw = fmaf(v, (x[(int64_t)a * D] - mu[a]) * rs[a], aw);
    ab += v;
  }
  if (pw) pw[vn * D + d] = aw;
  if (pb) pb[vn * D + d] = ab;
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

} // namespace vivit

using namespace vivit;

extern "C" {

int vivit_norm_stats_f32(const float *X, float *mean, float *rstd, int64_t rows, int64_t L, float eps, void *stream) {
  if (rows < 0 || L <= 0 || !(eps >= 0.f)) return VIVIT_E_BADARG;
  if (rows == 0) return VIVIT_OK;
  if (!X || !mean || !rstd) return VIVIT_E_BADARG;
  if (L > 0x7fffffffLL || rows > 0x7fffffffLL) return VIVIT_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = (L & 3) == 0 && aligned16(X);
  if (L <= NORM_WAVE_L) {
    const unsigned grid = (unsigned)cdiv(rows, 4);
    if (vec) norm_stats_wave_kernel<true><<<grid, 256, 0, s>>>(X, mean, rstd, rows, (int)L, eps);
    else norm_stats_wave_kernel<false><<<grid, 256, 0, s>>>(X, mean, rstd, rows, (int)L, eps);
  } else {
    if (vec) norm_stats_block_kernel<true><<<(unsigned)rows, 256, 0, s>>>(X, mean, rstd, (int)L, eps);
    else norm_stats_block_kernel<false><<<(unsigned)rows, 256, 0, s>>>(X, mean, rstd, (int)L, eps);
  }
  return launch_status();
}

int vivit_norm_rules_f32(const float *M, const float *X, const float *gamma, const float *mean, const float *rstd, float *out,
                         float *seg_w, float *seg_b, int64_t V, int64_t rows, int64_t L, int64_t G, int64_t S, void *stream) {
  if (V < 0 || rows < 0 || L <= 0 || G <= 0 || S <= 0 || L % S != 0 || rows % G != 0) return VIVIT_E_BADARG;
  if (V == 0 || rows == 0) return VIVIT_OK;
  if (!M || !X || !mean || !rstd || (!out && !seg_w && !seg_b)) return VIVIT_E_BADARG;
  const int64_t vrows = V * rows;
  if (L > 0x7fffffffLL || vrows > 0x7fffffffLL || G * (L / S) > 0x7fffffffLL) return VIVIT_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (the segment outputs are written 16 bytes at a time only where they are elementwise, S == 1: their rows then have L floats too)
  const bool vec = (L & 3) == 0 && aligned16(M) && aligned16(X) && aligned16(out) && (S != 1 || (aligned16(seg_w) && aligned16(seg_b)));
  if (L <= NORM_WAVE_L) {
    const unsigned grid = (unsigned)cdiv(vrows, 4);
    if (vec) norm_rules_wave_kernel<true><<<grid, 256, 0, s>>>(M, X, gamma, mean, rstd, out, seg_w, seg_b, vrows, rows, (int)L, (int)G, (int)S);
    else norm_rules_wave_kernel<false><<<grid, 256, 0, s>>>(M, X, gamma, mean, rstd, out, seg_w, seg_b, vrows, rows, (int)L, (int)G, (int)S);
  } else {
    if (vec) norm_rules_block_kernel<true><<<(unsigned)vrows, 256, 0, s>>>(M, X, gamma, mean, rstd, out, seg_w, seg_b, rows, (int)L, (int)G, (int)S);
    else norm_rules_block_kernel<false><<<(unsigned)vrows, 256, 0, s>>>(M, X, gamma, mean, rstd, out, seg_w, seg_b, rows, (int)L, (int)G, (int)S);
  }
  return launch_status();
}

int vivit_norm_position_sums_f32(const float *M, const float *X, const float *mean, const float *rstd, float *pw, float *pb, int64_t V,
                                 int64_t N, int64_t A, int64_t D, void *stream) {
  if (V < 0 || N < 0 || A <= 0 || D <= 0) return VIVIT_E_BADARG;
  if (V == 0 || N == 0) return VIVIT_OK;
  if (!M || !X || !mean || !rstd || (!pw && !pb)) return VIVIT_E_BADARG;
  const int64_t dblocks = cdiv(D, 256);
  if (A > 0x7fffffffLL || D > 0x7fffffffLL || V * N * dblocks > 0x7fffffffLL) return VIVIT_E_UNSUPPORTED;
  norm_position_sums_kernel<<<(unsigned)(V * N * dblocks), 256, 0, static_cast<hipStream_t>(stream)>>>(M, X, mean, rstd, pw, pb, N, (int)A,
                                                                                                      (int)D, (int)dblocks);
  return launch_status();
}

} // extern "C"
