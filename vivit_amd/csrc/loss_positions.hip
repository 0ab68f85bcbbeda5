// Cross-entropy loss-Hessian square root for outputs with positions: logits [N, C, *D], L = prod(D) positions per sample, a softmax
// over the C classes at every position (next-token cross entropy on [N, C, T], segmentation on [N, C, H, W]).  All fp32, memory-bound.
//
// With p[n, :, l] = softmax_c(logits[n, :, l]):
//   exact   (idx == null, V = C L, row v = c' L + l'):  S[v, n, c, l] = [l = l'] sqrt(p[n, c', l]) ([c = c'] - p[n, c, l]) scale
//   sampled (idx [V, N, L] int32 class indices):        S[m, n, c, l] = (p[n, c, l] - [c = idx[m, n, l]]) scale
// An index outside [0, C) matches no class; no address is ever formed from an index.
// Non-finite logits, as torch.softmax and the [N, C] kernel of jacobians.hip: a class at -inf beside finite ones has p = 0 (exact zero
// rows and columns); a NaN or a +inf at any class, or nothing but -inf, makes every class of THAT position NaN in every slice that
// writes it (all M sampled slices; the C slices v = c' L + l of the exact factor) and touches no other position -- the structural zeros
// of the exact factor stay 0.0.
//
// Two memory layouts of a sample (of the logits and of every (v, n) slice of S alike), two kernels, lanes along the unit-stride axis:
//   NLC (class stride 1, position stride C), ce_pos_rows_kernel: a ROW is the C contiguous classes of one position.  Rows of up to
//     ROWS_WAVE_C classes belong to one wavefront (four rows per workgroup, no barrier), longer rows to a workgroup of 256 threads.
//   NCL (class stride L, position stride 1), ce_pos_lanes_kernel: the 64 lanes of a wavefront hold 64 neighbouring positions (or 64
//     groups of four), the four wavefronts of a workgroup share the classes (c = w, w + 4, ...) and exchange their part of the
//     statistics through LDS.
// Each has a 16-byte body (the unit-stride extent a multiple of 4 and every operand 16-byte aligned) and a scalar body.
//
// One visit of a position computes the maximum and the sum of exp in a single sweep (a running maximum, the sum rescaled when it
// grows), then writes every slice of S at that position, the structural zeros of the exact factor included; the probabilities are
// recomputed from (max, 1 / sum) in the write sweep, whose reads of the logits come from cache -- nothing of size C is kept in LDS, so
// C has no cap.  No atomics; every sum has a fixed order, so two calls give the same bytes.
//
// A scale per position (vivit_ce_pos_sqrt_hessian_w_f32; cross entropy with ignore_index, class weights, label smoothing): the loss
// Hessian at position i = (n, l) is omega_i (diag p_i - p_i p_i^T), so the factors are the two above with s_i = sqrt(omega_i) (exact)
// or sqrt(omega_i / M) (sampled) in the place of `scale` -- the same kernels with one more template parameter, PS, and the same
// operations in the same order: an array that holds one float s everywhere gives the bytes of the call with scale = s.  A position
// with s_i == 0 (padding) is written as exact zeros in every slice that covers it whatever its logits hold, NaN and +-inf included;
// in NLC its row of logits is not read at all, in NCL a select is enough (its neighbours in the lane share the cache lines).  A
// position with s_i != 0 follows the non-finite rules above.  The scales of class-index targets are computed on the device by
// vivit_ce_target_scales_f32, below the factor kernels.
#include "common.h"

namespace vivit {
namespace {

constexpr int ROWS_WAVE_C = 1024;
constexpr int64_t I32_MAX = 0x7fffffffLL;
constexpr int64_t MAX_STRIDE_BLOCKS = 32768;   // grid-stride launches: 128 workgroups per CU, the rest in further trips

__device__ __forceinline__ float wave_sum(float a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
  return a;
}

__device__ __forceinline__ float wave_max(float a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = fmaxf(a, __shfl_xor(a, off, 64));
  return a;
}

// running (max, sum of exp(z - max)) of one lane: fold in a value / the larger of several values first, so that the sum is rescaled
// at most once per step.  A maximum of -inf (nothing but masked classes so far) keeps the sum at zero.
__device__ __forceinline__ void fold_max(float &mx, float &sum, float bm) {
  if (bm > mx) {
    sum *= expf(mx - bm);   // (mx = -inf: exp(-inf) = 0, and the sum is still 0)
    mx = bm;
  }
}

// A NaN never becomes the maximum (NaN > mx is false), so it has to reach the sum through its own term: while the maximum is still
// -inf the term is exp(z) -- 0 for z = -inf as before, NaN for a NaN (exp(z - mx) would be exp(NaN) there too, but also for -inf).
__device__ __forceinline__ float exp_term(float z, float mx) { return expf(z - (mx > -INFINITY ? mx : 0.f)); }

// a lane's part rescaled to the common maximum; a lane whose maximum is still -inf holds a sum of 0, or NaN if it met one
__device__ __forceinline__ float rescaled(float mx, float sum, float common) { return mx > -INFINITY ? sum * expf(mx - common) : sum; }

// ---- NLC: one row of C contiguous classes per position -------------------------------------------------------------------------------
// rows = N L (row = n L + l); S[(v rows + row) C + c]; idx[m rows + row].  TPR threads per row: 64 or 256.
// PS: the scale of a row is pos_scale[row] (vivit_ce_pos_sqrt_hessian_w_f32) instead of the one float `scale`; a row whose scale is
// zero is written as zeros in every slice and its logits are not read (the threads of a row agree on it: no barrier is left out).
template <bool VEC, int TPR, bool PS>
__global__ __launch_bounds__(256) void ce_pos_rows_kernel(const float *__restrict__ logits, const int32_t *__restrict__ idx,
                                                          const float *__restrict__ pos_scale, float *__restrict__ S, int64_t rows, int C,
                                                          int64_t L, int64_t Vd, float scale) {
  __shared__ float red[8];
  constexpr int RPB = 256 / TPR;
  const int sub = threadIdx.x / TPR, t = threadIdx.x % TPR;
  const int C4 = C >> 2;
  for (int64_t row0 = (int64_t)blockIdx.x * RPB; row0 < rows; row0 += (int64_t)gridDim.x * RPB) {
    const int64_t row = row0 + sub;
    if (row >= rows) continue;   // (TPR = 64 only: a wavefront of its own, and that route has no barrier)
    if constexpr (PS) {
      scale = pos_scale[row];
      if (scale == 0.f) {        // an uncounted position: every slice that covers it is zero, whatever its logits hold
        const int64_t slices = idx ? Vd : (int64_t)C * L;
        for (int64_t v = 0; v < slices; ++v) {
          float *dst = S + (v * rows + row) * C;
          if (VEC) {
            for (int c4 = t; c4 < C4; c4 += TPR) reinterpret_cast<float4 *>(dst)[c4] = make_float4(0.f, 0.f, 0.f, 0.f);
          } else {
            for (int c = t; c < C; c += TPR) dst[c] = 0.f;
          }
        }
        continue;
      }
    }
    const float *z = logits + row * C;
    const float4 *z4 = reinterpret_cast<const float4 *>(z);
    float mx = -INFINITY, sum = 0.f;
    if (VEC) {
      for (int c4 = t; c4 < C4; c4 += TPR) {
        const float4 u = z4[c4];
        fold_max(mx, sum, fmaxf(fmaxf(u.x, u.y), fmaxf(u.z, u.w)));
        sum += (exp_term(u.x, mx) + exp_term(u.y, mx)) + (exp_term(u.z, mx) + exp_term(u.w, mx));
      }
    } else {
      for (int c = t; c < C; c += TPR) {
        const float u = z[c];
        fold_max(mx, sum, u);
        sum += exp_term(u, mx);
      }
    }
    float common = wave_max(mx);
    if (TPR == 256) {
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = common;
      __syncthreads();
      common = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
    float total = wave_sum(rescaled(mx, sum, common));
    if (TPR == 256) {
      if ((threadIdx.x & 63) == 0) red[4 + (threadIdx.x >> 6)] = total;
      __syncthreads();
      total = ((red[4] + red[5]) + red[6]) + red[7];
      __syncthreads();           // (red is written again in the next trip)
    }
    const float inv = 1.f / total;

    if (idx) {                   // sampled: p once per class, every slice m written from it
      if (VEC) {
        for (int c4 = t; c4 < C4; c4 += TPR) {
          const float4 u = z4[c4];
          const float4 p = make_float4(expf(u.x - common) * inv, expf(u.y - common) * inv, expf(u.z - common) * inv, expf(u.w - common) * inv);
          for (int64_t m = 0; m < Vd; ++m) {
            const int64_t d = (int64_t)idx[m * rows + row] - 4 * (int64_t)c4;
            reinterpret_cast<float4 *>(S + (m * rows + row) * C)[c4] =
                make_float4((p.x - (d == 0 ? 1.f : 0.f)) * scale, (p.y - (d == 1 ? 1.f : 0.f)) * scale, (p.z - (d == 2 ? 1.f : 0.f)) * scale,
                            (p.w - (d == 3 ? 1.f : 0.f)) * scale);
          }
        }
      } else {
        for (int c = t; c < C; c += TPR) {
          const float p = expf(z[c] - common) * inv;
          for (int64_t m = 0; m < Vd; ++m) S[(m * rows + row) * C + c] = (p - (idx[m * rows + row] == c ? 1.f : 0.f)) * scale;
        }
      }
    } else {                     // exact: the C L slices v = c' L + l' at this position; zero unless l' = l
      const int64_t l = row % L;
      for (int cp = 0; cp < C; ++cp) {
        const float sq = sqrtf(expf(z[cp] - common) * inv) * scale;
        for (int64_t lp = 0; lp < L; ++lp) {
          float *dst = S + (((int64_t)cp * L + lp) * rows + row) * C;
          const bool hit = lp == l;
          if (VEC) {
            for (int c4 = t; c4 < C4; c4 += TPR) {
              float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
              if (hit) {
                const float4 u = z4[c4];
                const int d = cp - 4 * c4;
                o.x = sq * ((d == 0 ? 1.f : 0.f) - expf(u.x - common) * inv);
                o.y = sq * ((d == 1 ? 1.f : 0.f) - expf(u.y - common) * inv);
                o.z = sq * ((d == 2 ? 1.f : 0.f) - expf(u.z - common) * inv);
                o.w = sq * ((d == 3 ? 1.f : 0.f) - expf(u.w - common) * inv);
              }
              reinterpret_cast<float4 *>(dst)[c4] = o;
            }
          } else {
            for (int c = t; c < C; c += TPR) dst[c] = hit ? sq * ((c == cp ? 1.f : 0.f) - expf(z[c] - common) * inv) : 0.f;
          }
        }
      }
    }
  }
}

// ---- NCL: lanes along the positions ----------------------------------------------------------------------------------------------------
// logits[(n C + c) L + l]; S[((v N + n) C + c) L + l]; idx[(m N + n) L + l].  W = 4 (16-byte body) or 1 positions per lane; a group of
// W positions never leaves its sample (L % 4 == 0 on the 16-byte body).
template <int W>
struct Pack {
  float v[W];
};

template <int W>
__device__ __forceinline__ Pack<W> load_pack(const float *p) {
  Pack<W> r;
  if constexpr (W == 4) {
    const float4 u = *reinterpret_cast<const float4 *>(p);
    r.v[0] = u.x, r.v[1] = u.y, r.v[2] = u.z, r.v[3] = u.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int W>
__device__ __forceinline__ void store_pack(float *p, const Pack<W> &r) {
  if constexpr (W == 4) *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else *p = r.v[0];
}

// PS: position g W + i has the scale pos_scale[g W + i]; where it is zero the element is written as zero by a select (the logits
// of the neighbouring positions share the cache lines, so nothing would be saved by not reading).
template <int W, bool PS>
__global__ __launch_bounds__(256) void ce_pos_lanes_kernel(const float *__restrict__ logits, const int32_t *__restrict__ idx,
                                                           const float *__restrict__ pos_scale, float *__restrict__ S, int64_t N, int C,
                                                           int64_t L, int64_t Vd, float scale) {
  __shared__ float red_m[4][64 * W], red_s[4][64 * W];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t groups = N * L / W;
  for (int64_t g0 = (int64_t)blockIdx.x * 64; g0 < groups; g0 += (int64_t)gridDim.x * 64) {
    const int64_t g = g0 + lane;
    const bool active = g < groups;
    const int64_t n = active ? g * W / L : 0, l = active ? g * W - n * L : 0;
    const float *z = logits + n * C * L + l;
    float mx[W], sum[W];
#pragma unroll
    for (int i = 0; i < W; ++i) mx[i] = -INFINITY, sum[i] = 0.f;
    if (active) {
      for (int c = w; c < C; c += 4) {
        const Pack<W> u = load_pack<W>(z + (int64_t)c * L);
#pragma unroll
        for (int i = 0; i < W; ++i) {
          fold_max(mx[i], sum[i], u.v[i]);
          sum[i] += exp_term(u.v[i], mx[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < W; ++i) red_m[w][lane * W + i] = mx[i], red_s[w][lane * W + i] = sum[i];
    __syncthreads();
    float common[W], inv[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const int k = lane * W + i;
      common[i] = fmaxf(fmaxf(red_m[0][k], red_m[1][k]), fmaxf(red_m[2][k], red_m[3][k]));
      const float total = ((rescaled(red_m[0][k], red_s[0][k], common[i]) + rescaled(red_m[1][k], red_s[1][k], common[i])) +
                           rescaled(red_m[2][k], red_s[2][k], common[i])) + rescaled(red_m[3][k], red_s[3][k], common[i]);
      inv[i] = 1.f / total;
    }
    __syncthreads();             // (the tables are written again in the next trip)
    if (!active) continue;       // (no barrier below)
    float sc[W];
#pragma unroll
    for (int i = 0; i < W; ++i) sc[i] = PS ? pos_scale[g * W + i] : scale;

    if (idx) {                   // sampled
      for (int c = w; c < C; c += 4) {
        const Pack<W> u = load_pack<W>(z + (int64_t)c * L);
        Pack<W> p;
#pragma unroll
        for (int i = 0; i < W; ++i) p.v[i] = expf(u.v[i] - common[i]) * inv[i];
        for (int64_t m = 0; m < Vd; ++m) {
          const int32_t *k = idx + (m * N + n) * L + l;
          int32_t ki[W];
          if constexpr (W == 4) {
            const int4 q = *reinterpret_cast<const int4 *>(k);
            ki[0] = q.x, ki[1] = q.y, ki[2] = q.z, ki[3] = q.w;
          } else {
            ki[0] = *k;
          }
          Pack<W> o;
#pragma unroll
          for (int i = 0; i < W; ++i) {
            o.v[i] = (p.v[i] - (ki[i] == c ? 1.f : 0.f)) * sc[i];
            if (PS && sc[i] == 0.f) o.v[i] = 0.f;
          }
          store_pack<W>(S + ((m * N + n) * C + c) * L + l, o);
        }
      }
    } else {                     // exact: the C L slices v = c' L + l' of this sample; zero unless l' is the lane's own position
      for (int cp = 0; cp < C; ++cp) {
        const Pack<W> up = load_pack<W>(z + (int64_t)cp * L);
        float sq[W];
#pragma unroll
        for (int i = 0; i < W; ++i) sq[i] = sqrtf(expf(up.v[i] - common[i]) * inv[i]) * sc[i];
        for (int64_t lp = 0; lp < L; ++lp) {
          const int64_t v = (int64_t)cp * L + lp;
          const bool hit = lp >= l && lp < l + W;
          for (int c = w; c < C; c += 4) {
            Pack<W> o;
#pragma unroll
            for (int i = 0; i < W; ++i) o.v[i] = 0.f;
            if (hit) {
              const Pack<W> u = load_pack<W>(z + (int64_t)c * L);
#pragma unroll
              for (int i = 0; i < W; ++i)
                if (l + i == lp && !(PS && sc[i] == 0.f)) o.v[i] = sq[i] * ((c == cp ? 1.f : 0.f) - expf(u.v[i] - common[i]) * inv[i]);
            }
            store_pack<W>(S + ((v * N + n) * C + c) * L + l, o);
          }
        }
      }
    }
  }
}

// ---- the scale of a position from its target (vivit_ce_target_scales_f32) ------------------------------------------------------------
// With class weights w (all ones if absent), wbar = mean_c w_c and eps the label smoothing, row r with target y counts iff
// y != ignore_index and 0 <= y < C; then a_r = (1 - eps) w[y] + eps wbar (exactly 1 without weights), else a_r = 0, and
//   pos_scale[r] = (float)(sqrt(a_r) / sqrt(mult norm)),  norm = sum over the counted rows of w[y] ('mean') or 1 ('sum'),
// all in fp64.  Decisions: a_r == 0 gives 0 even when norm == 0 (nothing counted); a_r < 0 (a negative weight) gives NaN; a target
// outside [0, C) that is not ignore_index has weight 0 and no address is formed from it.
// Two launches, no atomics: SCALE_PARTS workgroups each add their rows' w[y] (and their share of the classes' w) in a fixed order
// and leave one fp64 partial each; every thread of the second launch adds the partials in index order.  Nothing returns to the host.
constexpr int SCALE_PARTS = 256;

__device__ __forceinline__ bool counted(int64_t y, int64_t C, int64_t ignore_index) { return y != ignore_index && y >= 0 && y < C; }

__device__ __forceinline__ double block_sum(double a, double *red) {   // 256 threads, a fixed tree; the total in every thread
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double total = red[0];
  __syncthreads();
  return total;
}

// part[b] = sum of w[y] over the counted rows of workgroup b (need_norm), part[parts + b] = its share of sum_c w_c (need_wbar)
__global__ __launch_bounds__(256) void ce_scale_partials_kernel(const int64_t *__restrict__ target, const float *__restrict__ weight,
                                                                double *__restrict__ part, int64_t R, int64_t C, int64_t ignore_index,
                                                                int need_norm, int need_wbar) {
  __shared__ double red[256];
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (need_norm) {
    double acc = 0.0;
    for (int64_t r = first; r < R; r += step) {
      const int64_t y = target[r];
      if (counted(y, C, ignore_index)) acc += weight ? (double)weight[y] : 1.0;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
  }
  if (need_wbar) {
    double acc = 0.0;
    for (int64_t c = first; c < C; c += step) acc += (double)weight[c];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = acc;
  }
}

__global__ __launch_bounds__(256) void ce_scale_rows_kernel(const int64_t *__restrict__ target, const float *__restrict__ weight,
                                                            const double *__restrict__ part, float *__restrict__ pos_scale, int64_t R,
                                                            int64_t C, int64_t ignore_index, double eps, double mult, int parts,
                                                            int need_norm, int need_wbar) {
  double norm = 1.0, wbar = 0.0;
  if (need_norm) {
    norm = 0.0;
    for (int b = 0; b < parts; ++b) norm += part[b];
  }
  if (need_wbar) {
    for (int b = 0; b < parts; ++b) wbar += part[parts + b];
    wbar /= (double)C;
  }
  const double den = sqrt(mult * norm);
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
    const int64_t y = target[r];
    double a = 0.0;
    if (counted(y, C, ignore_index)) {
      if (!weight) a = 1.0;                                  // (1 - eps) + eps, exactly
      else if (need_wbar) a = (1.0 - eps) * (double)weight[y] + eps * wbar;
      else a = (double)weight[y];                            // eps == 0
    }
    pos_scale[r] = a == 0.0 ? 0.f : (float)(sqrt(a) / den);
  }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool VEC, bool PS>
void launch_rows(const float *logits, const int32_t *idx, const float *pos_scale, float *S, int64_t rows, int64_t C, int64_t L, int64_t V,
                 float scale, hipStream_t s) {
  if (C <= ROWS_WAVE_C) {
    const int64_t blocks = cdiv(rows, 4);
    ce_pos_rows_kernel<VEC, 64, PS><<<(unsigned)(blocks > MAX_STRIDE_BLOCKS ? MAX_STRIDE_BLOCKS : blocks), 256, 0, s>>>(
        logits, idx, pos_scale, S, rows, (int)C, L, V, scale);
  } else {
    ce_pos_rows_kernel<VEC, 256, PS><<<(unsigned)(rows > MAX_STRIDE_BLOCKS ? MAX_STRIDE_BLOCKS : rows), 256, 0, s>>>(
        logits, idx, pos_scale, S, rows, (int)C, L, V, scale);
  }
}

// both entry points: PS = a scale per position (pos_scale) instead of the one float
template <bool PS>
int ce_pos_sqrt_hessian(const float *logits, const int32_t *idx, const float *pos_scale, float *S, int64_t N, int64_t C, int64_t L,
                        int64_t V, int layout, float scale, void *stream) {
  if (N < 0 || C < 0 || L < 0 || V < 0 || (layout != 0 && layout != 1)) return VIVIT_E_BADARG;
  if (N == 0 || C == 0 || L == 0 || V == 0) return VIVIT_OK;
  if (!logits || !S || (PS && !pos_scale)) return VIVIT_E_BADARG;
  // every size and the number of positions N L fit 31 bits; the elements of S, V N C L, stay below 2^60 (offsets are 64-bit)
  if (N > I32_MAX || C > I32_MAX || L > I32_MAX || V > I32_MAX || N * L > I32_MAX) return VIVIT_E_UNSUPPORTED;
  if (!idx && V != C * L) return VIVIT_E_BADARG;
  const int64_t cap = (int64_t)1 << 60;
  if (C * L > cap / V || V * C * L > cap / N) return VIVIT_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (layout == 1 || L == 1) {   // (one position per sample: the two layouts are the same memory)
    const bool vec = (C & 3) == 0 && aligned16(logits) && aligned16(S);
    if (vec) launch_rows<true, PS>(logits, idx, pos_scale, S, N * L, C, L, V, scale, s);
    else launch_rows<false, PS>(logits, idx, pos_scale, S, N * L, C, L, V, scale, s);
  } else {
    const bool vec = (L & 3) == 0 && aligned16(logits) && aligned16(S) && aligned16(idx);
    const int64_t blocks = cdiv(N * L / (vec ? 4 : 1), 64);
    const unsigned grid = (unsigned)(blocks > MAX_STRIDE_BLOCKS ? MAX_STRIDE_BLOCKS : blocks);
    if (vec) ce_pos_lanes_kernel<4, PS><<<grid, 256, 0, s>>>(logits, idx, pos_scale, S, N, (int)C, L, V, scale);
    else ce_pos_lanes_kernel<1, PS><<<grid, 256, 0, s>>>(logits, idx, pos_scale, S, N, (int)C, L, V, scale);
  }
  return launch_status();
}

} // namespace
} // namespace vivit

using namespace vivit;

extern "C" {

int vivit_ce_pos_sqrt_hessian_f32(const float *logits, const int32_t *idx, float *S, int64_t N, int64_t C, int64_t L, int64_t V, int layout,
                                  float scale, void *stream) {
  return ce_pos_sqrt_hessian<false>(logits, idx, nullptr, S, N, C, L, V, layout, scale, stream);
}

int vivit_ce_pos_sqrt_hessian_w_f32(const float *logits, const int32_t *idx, const float *pos_scale, float *S, int64_t N, int64_t C,
                                    int64_t L, int64_t V, int layout, void *stream) {
  return ce_pos_sqrt_hessian<true>(logits, idx, pos_scale, S, N, C, L, V, layout, 0.f, stream);
}

size_t vivit_ce_target_scales_f32_workspace_bytes(int64_t R, int64_t C) {
  (void)R, (void)C;
  return 2 * SCALE_PARTS * sizeof(double);
}

int vivit_ce_target_scales_f32(const int64_t *target, const float *class_weight, float *pos_scale, int64_t R, int64_t C, int64_t ignore_index,
                               double label_smoothing, int mean, int64_t mult, void *workspace, size_t workspace_bytes, void *stream) {
  if (R < 0 || C < 0 || mult < 1 || (mean != 0 && mean != 1)) return VIVIT_E_BADARG;
  if (R == 0) return VIVIT_OK;
  if (!target || !pos_scale) return VIVIT_E_BADARG;
  if (R > I32_MAX || C > I32_MAX || mult > I32_MAX) return VIVIT_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < vivit_ce_target_scales_f32_workspace_bytes(R, C) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return VIVIT_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int need_norm = mean, need_wbar = class_weight && label_smoothing != 0.0 && C > 0;
  double *part = static_cast<double *>(workspace);
  const int64_t most = R > C ? R : C;
  const int parts = (int)(cdiv(most, 1024) > SCALE_PARTS ? SCALE_PARTS : cdiv(most, 1024));
  if (need_norm || need_wbar)
    ce_scale_partials_kernel<<<parts, 256, 0, s>>>(target, class_weight, part, R, C, ignore_index, need_norm, need_wbar);
  const int64_t blocks = cdiv(R, 256);
  ce_scale_rows_kernel<<<(unsigned)(blocks > MAX_STRIDE_BLOCKS ? MAX_STRIDE_BLOCKS : blocks), 256, 0, s>>>(
      target, class_weight, part, pos_scale, R, C, ignore_index, label_smoothing, (double)mult, parts, need_norm, need_wbar);
  return launch_status();
}

} // extern "C"

