// Gram matrix of a Linear weight on a sequence input [N, T, in] from the two Gram matrices of its factors (gfx950):
//   G[(c, n), (e, m)] = alpha * sum_{t, u < T} Gz[(n, t), (m, u)] * Gs[(c, n, t), (e, m, u)] + beta * G[(c, n), (e, m)]
// the Hadamard product of vivit_gram_hadamard_block_f32 with every T x T block summed (T = 1 is that kernel, bit for bit).
// HBM-bound on Gs, which is read once; the Gz block of a sample pair is read Cr * Cc times, from the L2.
//
// seq_reduce_kernel: one workgroup per output row (c, n) and span of SR_SPAN / T whole outputs (e, m), that is at most SR_SPAN
// consecutive columns (e, m, u) of the T rows (c, n, t) of Gs.  A lane owns four of those columns (one float4, or four dwords 256
// apart), walks down the T rows with one fma per element -- every wave-instruction reads 1 KiB (256 B scalar) of one row of Gs --
// and leaves the four column sums in LDS; then one lane per output adds its T column sums in the order u = 0 .. T - 1.
//
// SUMMATION ORDER of an entry: acc_u = fma chain over t = 0 .. T - 1 starting at 0, then ((acc_0 + acc_1) + ...) + acc_{T-1}, then
// alpha * sum, then fma(beta, G, .).  It depends on T alone: not on the position, the block's sizes, the span or the body (vector /
// scalar), so the bytes of an entry are a function of its two T x T operand blocks, alpha, beta and the prior entry.  No atomics.
#include "common.h"

namespace vivit {

constexpr int SR_BLOCK = 256;
constexpr int SR_SPAN = 1024;      // columns (e, m, u) per workgroup, at most; four per lane
constexpr int SR_T_MAX = SR_SPAN;  // a T x T block is never split over workgroups
constexpr int64_t SR_ROWS_MAX = (int64_t(1) << 24) - 1;  // one workgroup per row in grid.x: rows * SR_BLOCK stays below 2^32

// Outputs per workgroup: as many whole outputs as SR_SPAN columns hold, rounded down so that a span starts at a multiple of four
// columns whenever T allows it (the float4 body).  A function of T alone.
static inline int64_t sr_outputs(int64_t T) {
  int64_t jt = SR_SPAN / T;
  const int64_t q = (T % 4 == 0) ? 1 : (T % 2 == 0) ? 2 : 4;
  if (jt >= q) jt -= jt % q;
  return jt;
}

template <bool VEC>
__global__ __launch_bounds__(SR_BLOCK) void seq_reduce_kernel(const float *__restrict__ Gz, int64_t ldz,
                                                              const float *__restrict__ Gs, int64_t lds, float *__restrict__ G,
                                                              int64_t ldg, int Nr, int Nc, int cols, int T, int JT, float alpha,
                                                              float beta) {
  // column sums of the span, an output's T sums Tp apart (Tp odd: the lanes of the second phase hit distinct banks)
  __shared__ float part[SR_SPAN + SR_SPAN / 2 + 1];
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x;                 // output row (c, n)
  const int n = (int)(r % Nr);
  const int j0 = (int)blockIdx.y * JT;          // first output column (e, m) of the span
  const int jn = cols - j0 < JT ? cols - j0 : JT;
  const int L = jn * T;                         // columns (e, m, u) of the span
  const int Tp = T | 1;
  const int zw = Nc * T;                        // Gz's columns repeat with period Nc * T along (e, m, u)
  const float *zrow = Gz + (int64_t)n * T * ldz;
  const float *srow = Gs + r * T * lds + (int64_t)j0 * T;
  const int zfirst = (int)(((int64_t)j0 * T) % zw);

  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    const int q = 4 * tid;                      // L, zw and the span's first column are multiples of 4: no float4 straddles an end
    if (q < L) {
      const int zc = (zfirst + q) % zw;
#pragma unroll 4
      for (int t = 0; t < T; ++t) {
        const float4 z = *reinterpret_cast<const float4 *>(zrow + t * ldz + zc);
        const float4 s = *reinterpret_cast<const float4 *>(srow + t * lds + q);
        acc[0] = fmaf(z.x, s.x, acc[0]);
        acc[1] = fmaf(z.y, s.y, acc[1]);
        acc[2] = fmaf(z.z, s.z, acc[2]);
        acc[3] = fmaf(z.w, s.w, acc[3]);
      }
    }
  } else {
    int zc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) zc[k] = (zfirst + tid + SR_BLOCK * k) % zw;
#pragma unroll 2
    for (int t = 0; t < T; ++t) {
      const float *zr = zrow + t * ldz, *sr = srow + t * lds;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = tid + SR_BLOCK * k;
        if (q < L) acc[k] = fmaf(zr[zc[k]], sr[q], acc[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int q = VEC ? 4 * tid + k : tid + SR_BLOCK * k;
    if (q < L) {
      const int j = q / T;
      part[j * Tp + (q - j * T)] = acc[k];
    }
  }
  __syncthreads();
  for (int j = tid; j < jn; j += SR_BLOCK) {
    const float *p = part + j * Tp;
    float sum = p[0];
    for (int u = 1; u < T; ++u) sum += p[u];
    float *g = G + r * ldg + j0 + j;
    float o = alpha * sum;
    if (beta != 0.f) o = fmaf(beta, *g, o);
    *g = o;
  }
}

// T = 1: the arithmetic of hadamard_block_kernel (csrc/elementwise.hip) on operands with leading dimensions.
template <bool VEC>
__global__ __launch_bounds__(SR_BLOCK) void seq_hadamard_kernel(const float *__restrict__ Gz, int64_t ldz,
                                                                const float *__restrict__ Gs, int64_t lds, float *__restrict__ G,
                                                                int64_t ldg, int64_t rows, int64_t Nr, int64_t cols, int64_t Nc,
                                                                float alpha, float beta) {
  const int64_t total = VEC ? (rows * cols) >> 2 : rows * cols;
  for (int64_t idx = (int64_t)blockIdx.x * SR_BLOCK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * SR_BLOCK) {
    const int64_t flat = VEC ? idx << 2 : idx;
    const int64_t row = flat / cols, col = flat - row * cols;
    const int64_t nn = row % Nr, mm = col % Nc;
    float *g = G + row * ldg + col;
    if (VEC) {
      const float4 z = *reinterpret_cast<const float4 *>(Gz + nn * ldz + mm);
      const float4 sv = *reinterpret_cast<const float4 *>(Gs + row * lds + col);
      float4 o = make_float4(alpha * z.x * sv.x, alpha * z.y * sv.y, alpha * z.z * sv.z, alpha * z.w * sv.w);
      if (beta != 0.f) {
        const float4 old = *reinterpret_cast<const float4 *>(g);
        o.x += beta * old.x; o.y += beta * old.y; o.z += beta * old.z; o.w += beta * old.w;
      }
      *reinterpret_cast<float4 *>(g) = o;
    } else {
      float o = alpha * Gz[nn * ldz + mm] * Gs[row * lds + col];
      if (beta != 0.f) o += beta * *g;
      *g = o;
    }
  }
}

} // namespace vivit

using namespace vivit;

extern "C" {

int vivit_gram_seq_reduce_f32(const float *Gz, int64_t ldz, const float *Gs, int64_t lds, float *G, int64_t ldg, int64_t Cr,
                              int64_t Nr, int64_t Cc, int64_t Nc, int64_t T, float alpha, float beta, void *stream) {
  constexpr int64_t I32 = 2147483647;
  if (Cr < 0 || Nr < 0 || Cc < 0 || Nc < 0 || T < 0) return VIVIT_E_BADARG;
  if (Cr > I32 || Nr > I32 || Cc > I32 || Nc > I32 || T > I32) return VIVIT_E_UNSUPPORTED;
  const int64_t rows = Cr * Nr, cols = Cc * Nc;                     // (below 2^62)
  if (rows > I32 || cols > I32 || rows * T > I32 || cols * T > I32) return VIVIT_E_UNSUPPORTED;
  if (ldz < Nc * T || lds < cols * T || ldg < cols) return VIVIT_E_BADARG;
  if (rows == 0 || cols == 0 || T == 0) return VIVIT_OK;
  if (!Gz || !Gs || !G) return VIVIT_E_BADARG;
  if (ldz > I32 || lds > I32 || ldg > I32 || T > SR_T_MAX) return VIVIT_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool aligned = ((ldz | lds) % 4 == 0) && ((reinterpret_cast<uintptr_t>(Gz) | reinterpret_cast<uintptr_t>(Gs)) & 15) == 0;
  if (T == 1) {
    const bool vec = aligned && Nc % 4 == 0 && ldg % 4 == 0 && (reinterpret_cast<uintptr_t>(G) & 15) == 0;
    int64_t grid = cdiv(vec ? (rows * cols) >> 2 : rows * cols, SR_BLOCK);
    if (grid > 2048) grid = 2048;
    if (vec)
      seq_hadamard_kernel<true><<<(unsigned)grid, SR_BLOCK, 0, s>>>(Gz, ldz, Gs, lds, G, ldg, rows, Nr, cols, Nc, alpha, beta);
    else
      seq_hadamard_kernel<false><<<(unsigned)grid, SR_BLOCK, 0, s>>>(Gz, ldz, Gs, lds, G, ldg, rows, Nr, cols, Nc, alpha, beta);
    return launch_status();
  }
  const int64_t jt = sr_outputs(T);
  const int64_t spans = cdiv(cols, jt);
  if (spans > 65535 || rows > SR_ROWS_MAX) return VIVIT_E_UNSUPPORTED;
  const bool vec = aligned && (Nc * T) % 4 == 0 && (jt * T) % 4 == 0;
  const dim3 grid((unsigned)rows, (unsigned)spans);
  if (vec)
    seq_reduce_kernel<true><<<grid, SR_BLOCK, 0, s>>>(Gz, ldz, Gs, lds, G, ldg, (int)Nr, (int)Nc, (int)cols, (int)T, (int)jt, alpha,
                                                      beta);
  else
    seq_reduce_kernel<false><<<grid, SR_BLOCK, 0, s>>>(Gz, ldz, Gs, lds, G, ldg, (int)Nr, (int)Nc, (int)cols, (int)T, (int)jt, alpha,
                                                       beta);
  return launch_status();
}

} // extern "C"
