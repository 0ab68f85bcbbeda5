// RMSNorm, the gated product and rotary position embeddings: the rules of the sqrt-GGN factor for the modules of a LLaMA-style
// decoder block (nn.RMSNorm, ProductModule and RotaryEmbedding of vivit_amd/backend/custom_module.py).  All fp32, memory-bound.
//
// RMSNorm.  A ROW is the set of L contiguous elements that share one statistic (rows = numel / L; A = rows / N rows per sample):
//   rms_norm_stats_*:            rstd[r] = 1 / sqrt(sum_l x^2 / L + eps)
//   rms_norm_rules_*:            xhat = x rstd, h = gamma o M (gamma = 1 when null),
//                                out = rstd (h - xhat mean_l(h o xhat)),  w = M xhat
//   rms_norm_position_sums_kernel:  pw[v, n, d] = sum_a M x rstd  (the weight rule when A > 1)
// The routes are those of csrc/norm_rules.hip: a row of L <= RMS_WAVE_L elements is held in the registers of ONE wavefront (16
// elements per lane, four rows per workgroup); a longer row belongs to one workgroup of 256 threads whose second sweep over M and
// x comes from cache.  Each route has a 16-byte body (L % 4 == 0 and every operand 16-byte aligned) and a scalar body.  No atomics;
// every sum is a per-lane serial sum in index order, a butterfly over the 64 lanes and -- on the workgroup route -- the four wave
// sums added in order, so the bytes of a row's results depend on (L, body) only: not on V, on the number of rows or on where the
// row sits in the launch.
//
// Gated product (a * b):  Ga = M b, Gb = M a from one read of M; every result is ONE rounded product.
// Rotary (half-split pairing, tables as inputs: no sine or cosine is evaluated here): the transpose of the rotation on the q and k
// thirds of the packed projection, the v third copied.
#include "common.h"

namespace vivit {
namespace {

constexpr int RMS_WAVE_L = 1024;   // 16 elements per lane
constexpr int RMS_PER_LANE = RMS_WAVE_L / 64;

// (wave_sum, block_sum, wave_pos, wave_load and wave_store are those of csrc/norm_rules.hip, repeated: the two files share no header)
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
__device__ __forceinline__ void wave_load(const float *__restrict__ p, int L, int lane, float (&v)[RMS_PER_LANE]) {
  if (VEC) {
    const float4 *p4 = reinterpret_cast<const float4 *>(p);
#pragma unroll
    for (int k = 0; k < RMS_PER_LANE / 4; ++k) {
      const int l4 = lane + 64 * k;
      const float4 q = 4 * l4 < L ? p4[l4] : make_float4(0.f, 0.f, 0.f, 0.f);
      v[4 * k] = q.x, v[4 * k + 1] = q.y, v[4 * k + 2] = q.z, v[4 * k + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < RMS_PER_LANE; ++e) v[e] = lane + 64 * e < L ? p[lane + 64 * e] : 0.f;
  }
}

template <bool VEC>
__device__ __forceinline__ void wave_store(float *__restrict__ p, int L, int lane, const float (&v)[RMS_PER_LANE]) {
  if (VEC) {
    float4 *p4 = reinterpret_cast<float4 *>(p);
#pragma unroll
    for (int k = 0; k < RMS_PER_LANE / 4; ++k) {
      const int l4 = lane + 64 * k;
      if (4 * l4 < L) p4[l4] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < RMS_PER_LANE; ++e)
      if (lane + 64 * e < L) p[lane + 64 * e] = v[e];
  }
}

// ---- RMSNorm: statistics --------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void rms_norm_stats_wave_kernel(const float *__restrict__ X, float *__restrict__ rstd, int64_t rows,
                                                                  int L, float eps) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  float x[RMS_PER_LANE];
  wave_load<VEC>(X + r * L, L, lane, x);
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < RMS_PER_LANE; ++e) q = fmaf(x[e], x[e], q);   // (positions beyond L hold 0)
  const float ms = wave_sum(q) / (float)L;
  if (lane == 0) rstd[r] = 1.f / sqrtf(ms + eps);
}

template <bool VEC>
__global__ __launch_bounds__(256) void rms_norm_stats_block_kernel(const float *__restrict__ X, float *__restrict__ rstd, int L, float eps) {
  __shared__ float red[4];
  const float *x = X + (int64_t)blockIdx.x * L;
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  const int tid = threadIdx.x, L4 = L >> 2;
  float q = 0.f;
  if (VEC) {
    for (int l = tid; l < L4; l += 256) {
      const float4 u = x4[l];
      q = fmaf(u.x, u.x, q), q = fmaf(u.y, u.y, q), q = fmaf(u.z, u.z, q), q = fmaf(u.w, u.w, q);
    }
  } else {
    for (int l = tid; l < L; l += 256) q = fmaf(x[l], x[l], q);
  }
  const float ms = block_sum(q, red) / (float)L;
  if (tid == 0) rstd[blockIdx.x] = 1.f / sqrtf(ms + eps);
}

// ---- RMSNorm: rules -------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void rms_norm_rules_wave_kernel(const float *__restrict__ M, const float *__restrict__ X,
                                                                  const float *__restrict__ gamma, const float *__restrict__ rstd,
                                                                  float *__restrict__ out, float *__restrict__ w, int64_t vrows,
                                                                  int64_t rows, int L) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= vrows) return;
  const int lane = threadIdx.x & 63;
  const int64_t rx = r % rows;
  const float rs = rstd[rx];
  float mv[RMS_PER_LANE], xh[RMS_PER_LANE];
  wave_load<VEC>(M + r * L, L, lane, mv);
  wave_load<VEC>(X + rx * L, L, lane, xh);
#pragma unroll
  for (int e = 0; e < RMS_PER_LANE; ++e) xh[e] *= rs;
  if (w) {
    float t[RMS_PER_LANE];
#pragma unroll
    for (int e = 0; e < RMS_PER_LANE; ++e) t[e] = mv[e] * xh[e];
    wave_store<VEC>(w + r * L, L, lane, t);
  }
  if (out) {
    if (gamma) {
      float g[RMS_PER_LANE];
      wave_load<VEC>(gamma, L, lane, g);
#pragma unroll
      for (int e = 0; e < RMS_PER_LANE; ++e) mv[e] = g[e] * mv[e];   // h; 0 beyond the row
    }
    float s2 = 0.f;
#pragma unroll
    for (int e = 0; e < RMS_PER_LANE; ++e) s2 = fmaf(mv[e], xh[e], s2);
    const float c2 = wave_sum(s2) / (float)L;
#pragma unroll
    for (int e = 0; e < RMS_PER_LANE; ++e) mv[e] = rs * (mv[e] - xh[e] * c2);
    wave_store<VEC>(out + r * L, L, lane, mv);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void rms_norm_rules_block_kernel(const float *__restrict__ M, const float *__restrict__ X,
                                                                   const float *__restrict__ gamma, const float *__restrict__ rstd,
                                                                   float *__restrict__ out, float *__restrict__ w, int64_t rows, int L) {
  __shared__ float red[4];
  const int64_t r = blockIdx.x, rx = r % rows;
  const int tid = threadIdx.x, L4 = L >> 2;
  const float rs = rstd[rx];
  const float *m = M + r * L, *x = X + rx * L;
  const float4 *m4 = reinterpret_cast<const float4 *>(m), *x4 = reinterpret_cast<const float4 *>(x);
  const float4 *g4 = reinterpret_cast<const float4 *>(gamma);
  float c2 = 0.f;
  if (out) {
    float s2 = 0.f;
    if (VEC) {
      for (int l = tid; l < L4; l += 256) {
        const float4 p = m4[l], u = x4[l], g = gamma ? g4[l] : make_float4(1.f, 1.f, 1.f, 1.f);
        s2 = fmaf(g.x * p.x, u.x * rs, s2), s2 = fmaf(g.y * p.y, u.y * rs, s2);
        s2 = fmaf(g.z * p.z, u.z * rs, s2), s2 = fmaf(g.w * p.w, u.w * rs, s2);
      }
    } else {
      for (int l = tid; l < L; l += 256) s2 = fmaf((gamma ? gamma[l] : 1.f) * m[l], x[l] * rs, s2);
    }
    c2 = block_sum(s2, red) / (float)L;
  }
  float *o = out ? out + r * L : nullptr, *wr = w ? w + r * L : nullptr;   // the second sweep over M and x: from cache
  if (VEC) {
    float4 *o4 = reinterpret_cast<float4 *>(o), *w4 = reinterpret_cast<float4 *>(wr);
    for (int l = tid; l < L4; l += 256) {
      const float4 p = m4[l], u = x4[l];
      const float4 xh = make_float4(u.x * rs, u.y * rs, u.z * rs, u.w * rs);
      if (o) {
        const float4 g = gamma ? g4[l] : make_float4(1.f, 1.f, 1.f, 1.f);
        o4[l] = make_float4(rs * (g.x * p.x - xh.x * c2), rs * (g.y * p.y - xh.y * c2), rs * (g.z * p.z - xh.z * c2),
                            rs * (g.w * p.w - xh.w * c2));
      }
      if (wr) w4[l] = make_float4(p.x * xh.x, p.y * xh.y, p.z * xh.z, p.w * xh.w);
    }
  } else {
    for (int l = tid; l < L; l += 256) {
      const float p = m[l], xh = x[l] * rs;
      if (o) o[l] = rs * ((gamma ? gamma[l] : 1.f) * p - xh * c2);
      if (wr) wr[l] = p * xh;
    }
  }
}

// RMSNorm with A > 1 rows per sample: one thread per d, a serial loop over a; neighbouring threads read neighbouring d
__global__ __launch_bounds__(256) void rms_norm_position_sums_kernel(const float *__restrict__ M, const float *__restrict__ X,
                                                                     const float *__restrict__ rstd, float *__restrict__ pw, int64_t N,
                                                                     int A, int D, int dblocks) {
  const int64_t vn = blockIdx.x / dblocks, n = vn % N;
  const int d = (int)(blockIdx.x % dblocks) * 256 + threadIdx.x;
  if (d >= D) return;
  const float *m = M + vn * A * D + d, *x = X + n * A * D + d;
  const float *rs = rstd + n * A;
  float aw = 0.f;
  for (int a = 0; a < A; ++a) aw = fmaf(m[(int64_t)a * D], x[(int64_t)a * D] * rs[a], aw);
  pw[vn * D + d] = aw;
}

// ---- gated product ----------------------------------------------------------------------------------------------------------------
// blockIdx.x strides over the positions i of a slice (float4 in the 16-byte body), blockIdx.y over the slices v: a and b are read
// once per thread and position, M once in all.
template <bool VEC>
__global__ __launch_bounds__(256) void gate_jac_t_kernel(const float *__restrict__ M, const float *__restrict__ a,
                                                         const float *__restrict__ b, float *__restrict__ Ga, float *__restrict__ Gb,
                                                         int64_t V, int64_t n) {
  const int64_t items = VEC ? n >> 2 : n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
    if (VEC) {
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 av = Gb ? reinterpret_cast<const float4 *>(a)[i] : z, bv = Ga ? reinterpret_cast<const float4 *>(b)[i] : z;
      for (int64_t v = blockIdx.y; v < V; v += gridDim.y) {
        const int64_t at = v * items + i;
        const float4 m = reinterpret_cast<const float4 *>(M)[at];
        if (Ga) reinterpret_cast<float4 *>(Ga)[at] = make_float4(m.x * bv.x, m.y * bv.y, m.z * bv.z, m.w * bv.w);
        if (Gb) reinterpret_cast<float4 *>(Gb)[at] = make_float4(m.x * av.x, m.y * av.y, m.z * av.z, m.w * av.w);
      }
    } else {
      const float av = Gb ? a[i] : 0.f, bv = Ga ? b[i] : 0.f;
      for (int64_t v = blockIdx.y; v < V; v += gridDim.y) {
        const float m = M[v * n + i];
        if (Ga) Ga[v * n + i] = m * bv;
        if (Gb) Gb[v * n + i] = m * av;
      }
    }
  }
}

// ---- rotary -----------------------------------------------------------------------------------------------------------------------
// A ROW here is one (r, t): (H + 2 Hkv) d floats, H query heads | Hkv key heads | Hkv value heads (Hkv == H: three equal thirds).
// Its work items: (H + Hkv) hp pair items (the q and k parts; hp = d / 2 pairs per head, a quarter of that in the 16-byte body) and
// then the copy items of the v part, Hkv d columns.  A workgroup takes rpb = max(1, 256 / items) rows per trip.
// Every item reads its operands before it writes, and no two items touch the same element: G may alias M (not __restrict__).
template <bool VEC>
__global__ __launch_bounds__(256) void rope_jac_t_kernel(const float *M, const float *__restrict__ cosT, const float *__restrict__ sinT,
                                                         float *G, int64_t rows, int T, int H, int Hkv, int d, int rpb) {
  constexpr int W = VEC ? 4 : 1;
  const int half = d >> 1, hp = half / W, pair_items = (H + Hkv) * hp, copy_items = M == G ? 0 : Hkv * d / W;
  const int items = pair_items + copy_items;
  const int64_t row_len = ((int64_t)H + 2 * Hkv) * d;
  for (int64_t row0 = (int64_t)blockIdx.x * rpb; row0 < rows; row0 += (int64_t)gridDim.x * rpb) {
    for (int it = threadIdx.x; it < rpb * items; it += 256) {
      const int lr = it / items, wi = it - lr * items;
      const int64_t row = row0 + lr;
      if (row >= rows) break;
      const float *m = M + row * row_len;
      float *g = G + row * row_len;
      if (wi < pair_items) {
        const int hh = wi / hp, j = (wi - hh * hp) * W;   // hh: head of the q | k part, which is H + Hkv heads of d columns
        const int t = (int)(row % T);
        const int64_t at = (int64_t)hh * d + j, tab = (int64_t)t * half + j;
        if (VEC) {
          const float4 m1 = *reinterpret_cast<const float4 *>(m + at), m2 = *reinterpret_cast<const float4 *>(m + at + half);
          const float4 c = *reinterpret_cast<const float4 *>(cosT + tab), s = *reinterpret_cast<const float4 *>(sinT + tab);
          *reinterpret_cast<float4 *>(g + at) = make_float4(fmaf(m2.x, s.x, m1.x * c.x), fmaf(m2.y, s.y, m1.y * c.y),
                                                            fmaf(m2.z, s.z, m1.z * c.z), fmaf(m2.w, s.w, m1.w * c.w));
          *reinterpret_cast<float4 *>(g + at + half) = make_float4(fmaf(-m1.x, s.x, m2.x * c.x), fmaf(-m1.y, s.y, m2.y * c.y),
                                                                   fmaf(-m1.z, s.z, m2.z * c.z), fmaf(-m1.w, s.w, m2.w * c.w));
        } else {
          const float m1 = m[at], m2 = m[at + half], c = cosT[tab], s = sinT[tab];
          g[at] = fmaf(m2, s, m1 * c);
          g[at + half] = fmaf(-m1, s, m2 * c);
        }
      } else {
        const int64_t at = ((int64_t)H + Hkv) * d + (int64_t)(wi - pair_items) * W;
        if (VEC) *reinterpret_cast<float4 *>(g + at) = *reinterpret_cast<const float4 *>(m + at);
        else g[at] = m[at];
      }
    }
  }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
constexpr int64_t I32_MAX = 0x7fffffffLL;
constexpr int64_t MAX_STRIDE_BLOCKS = 32768;   // the grid-stride launches (gate, rotary): 128 workgroups per CU, the rest in further trips

} // namespace
} // namespace vivit

using namespace vivit;

extern "C" {

int vivit_rms_norm_stats_f32(const float *X, float *rstd, int64_t rows, int64_t L, float eps, void *stream) {
  if (rows < 0 || L < 0 || !(eps >= 0.f)) return VIVIT_E_BADARG;
  if (rows == 0 || L == 0) return VIVIT_OK;
  if (!X || !rstd) return VIVIT_E_BADARG;
  if (L > I32_MAX || rows > I32_MAX) return VIVIT_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = (L & 3) == 0 && aligned16(X);
  if (L <= RMS_WAVE_L) {
    const unsigned grid = (unsigned)cdiv(rows, 4);
    if (vec) rms_norm_stats_wave_kernel<true><<<grid, 256, 0, s>>>(X, rstd, rows, (int)L, eps);
    else rms_norm_stats_wave_kernel<false><<<grid, 256, 0, s>>>(X, rstd, rows, (int)L, eps);
  } else {
    if (vec) rms_norm_stats_block_kernel<true><<<(unsigned)rows, 256, 0, s>>>(X, rstd, (int)L, eps);
    else rms_norm_stats_block_kernel<false><<<(unsigned)rows, 256, 0, s>>>(X, rstd, (int)L, eps);
  }
  return launch_status();
}

int vivit_rms_norm_rules_f32(const float *M, const float *X, const float *gamma, const float *rstd, float *out, float *w, int64_t V,
                             int64_t rows, int64_t L, void *stream) {
  if (V < 0 || rows < 0 || L < 0) return VIVIT_E_BADARG;
  if (V == 0 || rows == 0 || L == 0) return VIVIT_OK;
  if (!M || !X || !rstd || (!out && !w)) return VIVIT_E_BADARG;
  if (L > I32_MAX || V > I32_MAX || rows > I32_MAX || V * rows > I32_MAX) return VIVIT_E_UNSUPPORTED;
  const int64_t vrows = V * rows;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = (L & 3) == 0 && aligned16(M) && aligned16(X) && aligned16(gamma) && aligned16(out) && aligned16(w);
  if (L <= RMS_WAVE_L) {
    const unsigned grid = (unsigned)cdiv(vrows, 4);
    if (vec) rms_norm_rules_wave_kernel<true><<<grid, 256, 0, s>>>(M, X, gamma, rstd, out, w, vrows, rows, (int)L);
    else rms_norm_rules_wave_kernel<false><<<grid, 256, 0, s>>>(M, X, gamma, rstd, out, w, vrows, rows, (int)L);
  } else {
    if (vec) rms_norm_rules_block_kernel<true><<<(unsigned)vrows, 256, 0, s>>>(M, X, gamma, rstd, out, w, rows, (int)L);
    else rms_norm_rules_block_kernel<false><<<(unsigned)vrows, 256, 0, s>>>(M, X, gamma, rstd, out, w, rows, (int)L);
  }
  return launch_status();
}

int vivit_rms_norm_position_sums_f32(const float *M, const float *X, const float *rstd, float *pw, int64_t V, int64_t N, int64_t A,
                                     int64_t D, void *stream) {
  if (V < 0 || N < 0 || A < 0 || D < 0) return VIVIT_E_BADARG;
  if (V == 0 || N == 0 || A == 0 || D == 0) return VIVIT_OK;
  if (!M || !X || !rstd || !pw) return VIVIT_E_BADARG;
  const int64_t dblocks = cdiv(D, 256);
  if (V > I32_MAX || N > I32_MAX || A > I32_MAX || D > I32_MAX || V * N > I32_MAX || V * N * dblocks > I32_MAX) return VIVIT_E_UNSUPPORTED;
  rms_norm_position_sums_kernel<<<(unsigned)(V * N * dblocks), 256, 0, static_cast<hipStream_t>(stream)>>>(M, X, rstd, pw, N, (int)A, (int)D,
                                                                                                          (int)dblocks);
  return launch_status();
}

int vivit_gate_jac_t_f32(const float *M, const float *a, const float *b, float *Ga, float *Gb, int64_t V, int64_t n, void *stream) {
  if (V < 0 || n < 0) return VIVIT_E_BADARG;
  if (V == 0 || n == 0) return VIVIT_OK;
  if (!M || (!Ga && !Gb) || (Ga && !b) || (Gb && !a)) return VIVIT_E_BADARG;
  if (V > I32_MAX || n > I32_MAX) return VIVIT_E_UNSUPPORTED;
  // (the operand of a null output is not read: its alignment does not matter)
  const bool vec = (n & 3) == 0 && aligned16(M) && aligned16(Ga) && aligned16(Gb) && (!Gb || aligned16(a)) && (!Ga || aligned16(b));
  const int64_t blocks = cdiv(vec ? n >> 2 : n, 256);
  const unsigned gx = (unsigned)(blocks > MAX_STRIDE_BLOCKS ? MAX_STRIDE_BLOCKS : blocks);
  const int64_t want_y = cdiv(2048, (int64_t)gx);   // short slices: spread the V slices over workgroups as well
  const unsigned gy = (unsigned)(want_y < V ? want_y : V);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) gate_jac_t_kernel<true><<<dim3(gx, gy), 256, 0, s>>>(M, a, b, Ga, Gb, V, n);
  else gate_jac_t_kernel<false><<<dim3(gx, gy), 256, 0, s>>>(M, a, b, Ga, Gb, V, n);
  return launch_status();
}

// the rotary rule on H + Hkv rotated heads and Hkv d copied columns (H = 0 = Hkv: nothing to do)
static int rope_jac_t(const float *M, const float *cosT, const float *sinT, float *G, int64_t R, int64_t T, int64_t H, int64_t Hkv,
                      int64_t d, void *stream) {
  if (R < 0 || T < 0 || H < 0 || d < 0 || (d & 1)) return VIVIT_E_BADARG;
  if (R == 0 || T == 0 || H == 0 || d == 0) return VIVIT_OK;
  if (!M || !cosT || !sinT || !G) return VIVIT_E_BADARG;
  if (R > I32_MAX || T > I32_MAX || H > I32_MAX || d > I32_MAX || R * T > I32_MAX || H + 2 * Hkv > I32_MAX / d || T * d > I32_MAX)
    return VIVIT_E_UNSUPPORTED;
  const int64_t rows = R * T, half = d >> 1;
  const bool vec = (half & 3) == 0 && aligned16(M) && aligned16(G) && aligned16(cosT) && aligned16(sinT);
  const int64_t items = ((H + Hkv) * half + (M == G ? 0 : Hkv * d)) / (vec ? 4 : 1);
  const int rpb = items >= 256 ? 1 : (int)(256 / items);
  const int64_t blocks = cdiv(rows, rpb);
  const unsigned grid = (unsigned)(blocks > MAX_STRIDE_BLOCKS ? MAX_STRIDE_BLOCKS : blocks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) rope_jac_t_kernel<true><<<grid, 256, 0, s>>>(M, cosT, sinT, G, rows, (int)T, (int)H, (int)Hkv, (int)d, rpb);
  else rope_jac_t_kernel<false><<<grid, 256, 0, s>>>(M, cosT, sinT, G, rows, (int)T, (int)H, (int)Hkv, (int)d, rpb);
  return launch_status();
}

int vivit_rope_jac_t_f32(const float *M, const float *cosT, const float *sinT, float *G, int64_t R, int64_t T, int64_t H, int64_t d,
                         void *stream) {
  return rope_jac_t(M, cosT, sinT, G, R, T, H, H, d, stream);
}

int vivit_rope_gqa_jac_t_f32(const float *M, const float *cosT, const float *sinT, float *G, int64_t R, int64_t T, int64_t H, int64_t Hkv,
                             int64_t d, void *stream) {
  if (Hkv <= 0 || H < 0 || H % Hkv != 0) return VIVIT_E_BADARG;
  return rope_jac_t(M, cosT, sinT, G, R, T, H, Hkv, d, stream);
}

} // extern "C"
