// nn.Embedding: the weight factor in its token-sparse form.  With idx [N, T] the token ids and M [V, N, T, D] the sqrt-GGN factor at
// the module output, the weight factor is Vt[v, n, w, :] = sum_{t: idx[n, t] = w} M[v, n, t, :]: at most T non-zero rows of length D
// per (v, n) out of W = num_embeddings.  It is kept COMPACT:
//   ids [N, T]     sample n's distinct tokens, strictly increasing, in its first U_n slots, -1 in the rest
//   B [V, N, T, D] B[v, n, u, :] = the sum of the rows of M[v, n] whose token is ids[n, u] (ascending t); rows of -1 slots are zero
// and everything the extensions need is computed from (B, ids):
//   emb_compact_kernel      B from M and the per-sample sorted order (the sort itself is plumbing of the caller)
//   emb_gram_kernel         G[(v, n), (v', n')] = sum_{u, u'} [ids[n, u] = ids[n', u'] >= 0] <B[v, n, u], B[v', n', u']>
//   emb_vmp_kernel          out[f, w, :] = sum_{v, n, u: ids[n, u] = w} mat[f, v, n] B[v, n, u, :]
//   emb_vtmp_kernel         out[f, v, n] = sum_u <mat[f, ids[n, u], :], B[v, n, u, :]>
//   emb_weight_mjp_kernel   the explicit factor [V, N, W, D]: zero fill plus row copies
// The Gram kernel is output-stationary.  Samples are taken in blocks of 16.  Three small launches build, per sample block, the sorted
// union of its tokens and for each of them the slot u in each of the 16 samples, or -1 (emb_first_kernel, emb_prefix_kernel,
// emb_table_kernel: binary searches in the sorted id rows, no sort and no atomics).  A workgroup of four waves owns a pair of sample
// blocks (bj <= bi), four row classes (one per wave) and four column classes: it joins the two token tables 256 entries at a time
// (binary search, matches in LDS) and, for every common token in ascending order, each wave multiplies its class's 16 x D operand
// (zero rows for the samples that lack the token) with the operands of the four column classes on v_mfma_f32_16x16x4_f32 into four
// 16 x 16 accumulators.  Operands are read straight from B in the instruction's layout, 16 columns per step: lane (i, kq) holds the
// columns 16 cc + 4 kq .. + 3 of row i and feeds component j to the j-th of four instructions, on both sides alike (the loads of
// four steps are issued together).  No atomics; the value of an entry is the sum over the tokens in ascending order, per token
// over the columns in that fixed order, and tokens that
// one of the two samples lacks add exact zeros: the bytes of a sample pair's V x V block depend on the two samples only, and a pair
// without a common token stays exactly zero.  Only the entries on and below the diagonal of G are computed; each is written to its
// mirror position as well.
#include "common.h"

namespace vivit {

constexpr int EMB_SB = 16;         // samples per sample block = rows of an MFMA operand
constexpr int EMB_VC = 4;          // classes per chunk: row classes of a workgroup (one per wave) and column classes of a wave
constexpr int EMB_CU = 4;          // 16-column steps of a token whose operand loads are in flight together
typedef float emb_f32x4 __attribute__((ext_vector_type(4)));

// ---- compact form -----------------------------------------------------------------------------------------------------------------
// perm [N, T]: the positions t of sample n ordered by token (stable); slot u owns the seg_count[n, u] sorted positions from
// seg_start[n, u] on.  One thread per element of B.
__global__ __launch_bounds__(256) void emb_compact_kernel(const float *__restrict__ M, const int *__restrict__ perm,
                                                          const int *__restrict__ seg_start, const int *__restrict__ seg_count,
                                                          float *__restrict__ B, int64_t total, int N, int T, int D) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t row = e / D;            // (v N + n) T + u
  const int c = (int)(e - row * D);
  const int64_t vn = row / T;
  const int u = (int)(row - vn * T);
  const int64_t n = vn % N;
  const int *p = perm + n * T;
  int j0 = seg_start[n * T + u], cnt = seg_count[n * T + u];
  j0 = j0 < 0 ? 0 : (j0 > T ? T : j0);
  cnt = cnt < 0 ? 0 : (cnt > T - j0 ? T - j0 : cnt);
  const float *m = M + vn * T * D + c;
  float acc = 0.f;
  for (int j = j0; j < j0 + cnt; ++j) {
    const int t = p[j];
    if ((unsigned)t < (unsigned)T) acc += m[(int64_t)t * D];
  }
  B[e] = acc;
}

// ---- token tables of the sample blocks -------------------------------------------------------------------------------------------
// As unsigned numbers a row of ids (increasing tokens, then -1) is ascending as a whole.
__device__ __forceinline__ int emb_lower_bound(const int *__restrict__ row, int len, unsigned key) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)row[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// first[n, u] = 1 when no earlier sample of n's block holds the token ids[n, u]
__global__ __launch_bounds__(256) void emb_first_kernel(const int *__restrict__ ids, int *__restrict__ first, int N, int T) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N * T) return;
  const int n = e / T, tok = ids[e];
  int f = 0;
  if (tok >= 0) {
    f = 1;
    for (int m = n / EMB_SB * EMB_SB; m < n; ++m) {
      const int p = emb_lower_bound(ids + (int64_t)m * T, T, (unsigned)tok);
      if (p < T && ids[(int64_t)m * T + p] == tok) { f = 0; break; }
    }
  }
  first[e] = f;
}

// pf[n, u] = sum_{u' < u} first[n, u'], u <= T (one thread per sample, serial)
__global__ __launch_bounds__(256) void emb_prefix_kernel(const int *__restrict__ first, int *__restrict__ pf, int N, int T) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  int run = 0;
  for (int u = 0; u < T; ++u) {
    pf[(int64_t)n * (T + 1) + u] = run;
    run += first[(int64_t)n * T + u];
  }
  pf[(int64_t)n * (T + 1) + T] = run;
}

// The rank of a token in its block's sorted union = the number of `first` entries of the block with a smaller token.
// tab_tok [NB, 16 T]; tab_slot [NB, 16 T, 16] (filled with -1 before).
__global__ __launch_bounds__(256) void emb_table_kernel(const int *__restrict__ ids, const int *__restrict__ first,
                                                        const int *__restrict__ pf, int *__restrict__ tab_tok,
                                                        int *__restrict__ tab_slot, int N, int T) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N * T) return;
  const int tok = ids[e];
  if (tok < 0) return;
  const int n = e / T, u = e - n * T, b = n / EMB_SB, s = n - b * EMB_SB;
  const int m1 = (b + 1) * EMB_SB < N ? (b + 1) * EMB_SB : N;
  int rank = 0;
  for (int m = b * EMB_SB; m < m1; ++m) rank += pf[(int64_t)m * (T + 1) + emb_lower_bound(ids + (int64_t)m * T, T, (unsigned)tok)];
  const int64_t at = (int64_t)b * EMB_SB * T + rank;      // (rank < 16 T: there are at most 16 T first entries)
  tab_slot[at * EMB_SB + s] = u;
  if (first[e]) tab_tok[at] = tok;
}

// ---- Gram matrix ------------------------------------------------------------------------------------------------------------------
struct EmbGeom {
  int V, N, T, D, vec;
  float alpha, beta;
};

// columns c .. c + 3 of a row of B (null: a zero row); columns beyond D are zero.  vec: D % 4 == 0 and B is 16-byte aligned.
__device__ __forceinline__ emb_f32x4 emb_ld4(const float *__restrict__ row, int c, int D, bool vec) {
  emb_f32x4 r = {0.f, 0.f, 0.f, 0.f};
  if (row == nullptr || c >= D) return r;
  if (vec) {
    const float4 q = *reinterpret_cast<const float4 *>(row + c);
    r[0] = q.x, r[1] = q.y, r[2] = q.z, r[3] = q.w;
  } else {
    r[0] = row[c];
    if (c + 1 < D) r[1] = row[c + 1];
    if (c + 2 < D) r[2] = row[c + 2];
    if (c + 3 < D) r[3] = row[c + 3];
  }
  return r;
}

__device__ __forceinline__ void emb_store(float *__restrict__ G, int64_t at, float val, float beta) {
  G[at] = beta != 0.f ? val + beta * G[at] : val;
}

__global__ __launch_bounds__(256) void emb_gram_kernel(const float *__restrict__ B, const int *__restrict__ pf,
                                                       const int *__restrict__ tab_tok, const int *__restrict__ tab_slot,
                                                       float *__restrict__ G, EmbGeom g) {
  __shared__ int s_match[256];
  // blockIdx.x numbers the pairs of sample blocks bj <= bi row by row: pair = bi (bi + 1) / 2 + bj
  const int64_t pair = blockIdx.x;
  int bi = (int)((sqrt(8.0 * (double)pair + 1.0) - 1.0) * 0.5);
  while ((int64_t)bi * (bi + 1) / 2 > pair) --bi;
  while ((int64_t)(bi + 1) * (bi + 2) / 2 <= pair) ++bi;
  const int bj = (int)(pair - (int64_t)bi * (bi + 1) / 2);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nch = (g.V + EMB_VC - 1) / EMB_VC;
  const int zr = blockIdx.y / nch, zc = blockIdx.y - zr * nch;
  const int v = EMB_VC * zr + wave, vc0 = EMB_VC * zc;     // this wave's row class (idle beyond V), the first column class
  const int i = lane & 15, kq = lane >> 4;
  const int N = g.N, T = g.T, D = g.D;
  int La = 0, Lb = 0;                                       // lengths of the two token tables
  for (int s = 0; s < EMB_SB; ++s) {
    if (EMB_SB * bi + s < N) La += pf[(int64_t)(EMB_SB * bi + s) * (T + 1) + T];
    if (EMB_SB * bj + s < N) Lb += pf[(int64_t)(EMB_SB * bj + s) * (T + 1) + T];
  }
  const int64_t tabA = (int64_t)bi * EMB_SB * T, tabB = (int64_t)bj * EMB_SB * T;
  const int nA = EMB_SB * bi + i, nB = EMB_SB * bj + i;
  const bool active = v < g.V;
  const int steps = (D + 15) / 16;
  emb_f32x4 acc[EMB_VC];
#pragma unroll
  for (int q = 0; q < EMB_VC; ++q) acc[q] = (emb_f32x4){0.f, 0.f, 0.f, 0.f};
  for (int ia0 = 0; ia0 < La; ia0 += 256) {
    __syncthreads();   // the previous 256 matches have been read
    int match = -1;
    if (ia0 + tid < La) {
      const int tok = tab_tok[tabA + ia0 + tid];
      const int p = emb_lower_bound(tab_tok + tabB, Lb, (unsigned)tok);
      if (p < Lb && tab_tok[tabB + p] == tok) match = p;
    }
    s_match[tid] = match;
    __syncthreads();
    if (!active) continue;
    const int cnt = La - ia0 < 256 ? La - ia0 : 256;
    for (int t = 0; t < cnt; ++t) {
      const int ib = s_match[t];
      if (ib < 0) continue;
      const int ua = tab_slot[(tabA + ia0 + t) * EMB_SB + i], ub = tab_slot[(tabB + ib) * EMB_SB + i];
      const float *ra = ua >= 0 ? B + (((int64_t)v * N + nA) * T + ua) * D : nullptr;
      const float *rb[EMB_VC];
#pragma unroll
      for (int q = 0; q < EMB_VC; ++q) rb[q] = (ub >= 0 && vc0 + q < g.V) ? B + (((int64_t)(vc0 + q) * N + nB) * T + ub) * D : nullptr;
      for (int cc0 = 0; cc0 < steps; cc0 += EMB_CU) {     // the loads of EMB_CU steps are issued together, then their products
        emb_f32x4 a4[EMB_CU], b4[EMB_CU][EMB_VC];
#pragma unroll
        for (int s = 0; s < EMB_CU; ++s) {
          const int c = 16 * (cc0 + s) + 4 * kq;
          a4[s] = emb_ld4(ra, c, D, g.vec);
#pragma unroll
          for (int q = 0; q < EMB_VC; ++q) b4[s][q] = emb_ld4(rb[q], c, D, g.vec);
        }
#pragma unroll
        for (int s = 0; s < EMB_CU; ++s) {
          if (cc0 + s >= steps) break;
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < EMB_VC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[s][j], b4[s][q][j], acc[q], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  // the lane holds the entries (row sample 4 kq + e, column sample i) of the tiles (v, vc0 + q)
  const int64_t n2 = (int64_t)g.V * N;
#pragma unroll
  for (int q = 0; q < EMB_VC; ++q) {
    const int vc = vc0 + q;
    if (vc >= g.V || nB >= N) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int s = 4 * kq + e, n = EMB_SB * bi + s;
      if (n >= N) continue;
      if (bi == bj && !(s > i || (s == i && v >= vc))) continue;     // a diagonal block pair: its lower half, mirrored below
      const int64_t r = (int64_t)v * N + n, c = (int64_t)vc * N + nB;
      const float val = g.alpha * acc[q][e];
      emb_store(G, r * n2 + c, val, g.beta);
      if (r != c) emb_store(G, c * n2 + r, val, g.beta);
    }
  }
}

// ---- products with the factor and the explicit factor ---------------------------------------------------------------------------
// order [N T]: the entries (n, u) as n T + u, stably sorted by token; token w owns the positions tok_start[w] .. tok_start[w + 1].
// One wave per (token, f): its members in that order, per member the classes in ascending order.
__global__ __launch_bounds__(64) void emb_vmp_kernel(const float *__restrict__ B, const int *__restrict__ order,
                                                     const int *__restrict__ tok_start, const float *__restrict__ mat,
                                                     float *__restrict__ out, int V, int N, int T, int D, int W) {
  const int w = blockIdx.x, f = blockIdx.y, NT = N * T;
  int j0 = tok_start[w], j1 = tok_start[w + 1];
  j0 = j0 < 0 ? 0 : (j0 > NT ? NT : j0);
  j1 = j1 < j0 ? j0 : (j1 > NT ? NT : j1);
  const float *mf = mat + (int64_t)f * V * N;
  for (int c = threadIdx.x; c < D; c += 64) {
    float acc = 0.f;
    for (int j = j0; j < j1; ++j) {
      const int e = order[j];
      if ((unsigned)e >= (unsigned)NT) continue;
      const int n = e / T;
      for (int v = 0; v < V; ++v) acc = fmaf(mf[(int64_t)v * N + n], B[((int64_t)v * NT + e) * D + c], acc);
    }
    out[((int64_t)f * W + w) * D + c] = acc;
  }
}

// one wave per (f, v, n): the slots in ascending order, the columns strided over the lanes, then a butterfly over the lanes
__global__ __launch_bounds__(64) void emb_vtmp_kernel(const float *__restrict__ B, const int *__restrict__ ids,
                                                      const float *__restrict__ mat, float *__restrict__ out, int64_t VN, int N, int T,
                                                      int D, int W) {
  const int64_t row = blockIdx.x, f = row / VN, vn = row - f * VN, n = vn % N;
  float acc = 0.f;
  for (int u = 0; u < T; ++u) {
    const int tok = ids[n * T + u];
    if (tok < 0 || tok >= W) continue;
    const float *m = mat + (f * W + tok) * D, *b = B + (vn * T + u) * D;
    for (int c = threadIdx.x; c < D; c += 64) acc = fmaf(m[c], b[c], acc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (threadIdx.x == 0) out[row] = acc;
}

// out [V, N, W, D] was zero-filled; a sample's ids are distinct, so no two rows meet
__global__ __launch_bounds__(256) void emb_weight_mjp_kernel(const float *__restrict__ B, const int *__restrict__ ids,
                                                             float *__restrict__ out, int64_t total, int N, int T, int D, int W) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t row = e / D, vn = row / T;
  const int c = (int)(e - row * D), u = (int)(row - vn * T);
  const int tok = ids[(vn % N) * T + u];
  if (tok < 0 || tok >= W) return;
  out[(vn * W + tok) * D + c] = B[e];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static const int64_t EMB_LIM = 0x7fffffffLL;

// V N T D elements of B: every size below 2^31, the element count below 2^62, the one-thread-per-element grids below 2^31 blocks
static int emb_sizes_status(int64_t V, int64_t N, int64_t T, int64_t D) {
  if (V <= 0 || N <= 0 || T <= 0 || D <= 0) return VIVIT_E_BADARG;
  if (V > EMB_LIM || N > EMB_LIM || T > EMB_LIM || D > EMB_LIM - 128) return VIVIT_E_UNSUPPORTED;   // (16 (cc + EMB_CU) + 15 stays in 32 bits)
  if (N > (EMB_LIM - 256) / (T + 1)) return VIVIT_E_UNSUPPORTED;                 // n T + u, n (T + 1) + u in 32 bits
  const int64_t NT = N * T;
  if (V > (((int64_t)1 << 62) / NT) / D || cdiv(V * NT * D, 256) > EMB_LIM) return VIVIT_E_UNSUPPORTED;
  return VIVIT_OK;
}

struct EmbGramPlan {
  int status;            // VIVIT_OK, or why nothing is launched
  int64_t NB, nch;
  size_t pf_off, tok_off, slot_off, slot_bytes, bytes;   // first [N T] | pf [N (T + 1)] | tab_tok [NB 16 T] | tab_slot [NB 16 T 16]
};

static EmbGramPlan embedding_gram_plan(int64_t V, int64_t N, int64_t T, int64_t D) {
  EmbGramPlan p{emb_sizes_status(V, N, T, D), 0, 0, 0, 0, 0, 0, 0};
  if (p.status != VIVIT_OK) return p;
  p.NB = cdiv(N, EMB_SB), p.nch = cdiv(V, EMB_VC);
  // the launch grid: the NB (NB + 1) / 2 pairs of sample blocks in x (below 2^31 up to NB = 65535), pairs of class chunks in y
  if (p.NB > 65535 || p.nch * p.nch > 65535 || V * N > EMB_LIM) return p.status = VIVIT_E_UNSUPPORTED, p;
  p.pf_off = align_up((size_t)(N * T) * 4, 256);
  p.tok_off = p.pf_off + align_up((size_t)(N * (T + 1)) * 4, 256);
  p.slot_off = p.tok_off + align_up((size_t)(p.NB * EMB_SB * T) * 4, 256);
  p.slot_bytes = (size_t)(p.NB * EMB_SB * T) * EMB_SB * 4;
  p.bytes = p.slot_off + p.slot_bytes;
  return p;
}

static inline bool emb_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

} // namespace vivit

using namespace vivit;

extern "C" {

int vivit_embedding_compact_f32(const float *M, const int32_t *perm, const int32_t *seg_start, const int32_t *seg_count, float *B,
                                int64_t V, int64_t N, int64_t T, int64_t D, void *stream) {
  if (!M || !perm || !seg_start || !seg_count || !B) return VIVIT_E_BADARG;
  const int st = emb_sizes_status(V, N, T, D);
  if (st != VIVIT_OK) return st;
  const int64_t total = V * N * T * D;
  emb_compact_kernel<<<(unsigned)cdiv(total, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(M, perm, seg_start, seg_count, B, total,
                                                                                              (int)N, (int)T, (int)D);
  return launch_status();
}

size_t vivit_embedding_gram_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t D) {
  const EmbGramPlan p = embedding_gram_plan(V, N, T, D);
  return p.status == VIVIT_OK ? p.bytes : 0;
}

int vivit_embedding_gram_f32(const float *B, const int32_t *ids, float *G, int64_t V, int64_t N, int64_t T, int64_t D, float alpha,
                             float beta, void *workspace, size_t workspace_bytes, void *stream) {
  if (!B || !ids || !G) return VIVIT_E_BADARG;
  const EmbGramPlan p = embedding_gram_plan(V, N, T, D);
  if (p.status != VIVIT_OK) return p.status;
  if (!workspace || workspace_bytes < p.bytes) return VIVIT_E_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  int *first = reinterpret_cast<int *>(ws), *pf = reinterpret_cast<int *>(ws + p.pf_off);
  int *tab_tok = reinterpret_cast<int *>(ws + p.tok_off), *tab_slot = reinterpret_cast<int *>(ws + p.slot_off);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(tab_slot, 0xff, p.slot_bytes, s) != hipSuccess) return VIVIT_E_LAUNCH;
  const unsigned eblocks = (unsigned)cdiv(N * T, 256);
  emb_first_kernel<<<eblocks, 256, 0, s>>>(ids, first, (int)N, (int)T);
  emb_prefix_kernel<<<(unsigned)cdiv(N, 256), 256, 0, s>>>(first, pf, (int)N, (int)T);
  emb_table_kernel<<<eblocks, 256, 0, s>>>(ids, first, pf, tab_tok, tab_slot, (int)N, (int)T);
  EmbGeom g;
  g.V = (int)V, g.N = (int)N, g.T = (int)T, g.D = (int)D;
  g.vec = (D & 3) == 0 && emb_aligned16(B);
  g.alpha = alpha, g.beta = beta;
  const dim3 grid((unsigned)(p.NB * (p.NB + 1) / 2), (unsigned)(p.nch * p.nch));
  emb_gram_kernel<<<grid, 256, 0, s>>>(B, pf, tab_tok, tab_slot, G, g);
  return launch_status();
}

int vivit_embedding_vmp_f32(const float *B, const int32_t *order, const int32_t *tok_start, const float *mat, float *out, int64_t F,
                            int64_t V, int64_t N, int64_t T, int64_t D, int64_t W, void *stream) {
  if (!B || !order || !tok_start || !mat || !out) return VIVIT_E_BADARG;
  if (F <= 0 || W <= 0) return VIVIT_E_BADARG;
  const int st = emb_sizes_status(V, N, T, D);
  if (st != VIVIT_OK) return st;
  if (F > 65535 || W > EMB_LIM - 1 || F > (((int64_t)1 << 62) / W) / D) return VIVIT_E_UNSUPPORTED;
  emb_vmp_kernel<<<dim3((unsigned)W, (unsigned)F), 64, 0, static_cast<hipStream_t>(stream)>>>(B, order, tok_start, mat, out, (int)V, (int)N,
                                                                                             (int)T, (int)D, (int)W);
  return launch_status();
}

int vivit_embedding_vtmp_f32(const float *B, const int32_t *ids, const float *mat, float *out, int64_t F, int64_t V, int64_t N,
                             int64_t T, int64_t D, int64_t W, void *stream) {
  if (!B || !ids || !mat || !out) return VIVIT_E_BADARG;
  if (F <= 0 || W <= 0) return VIVIT_E_BADARG;
  const int st = emb_sizes_status(V, N, T, D);
  if (st != VIVIT_OK) return st;
  if (W > EMB_LIM || V * N > EMB_LIM || F > EMB_LIM / (V * N) || F > (((int64_t)1 << 62) / W) / D) return VIVIT_E_UNSUPPORTED;
  emb_vtmp_kernel<<<(unsigned)(F * V * N), 64, 0, static_cast<hipStream_t>(stream)>>>(B, ids, mat, out, V * N, (int)N, (int)T, (int)D,
                                                                                     (int)W);
  return launch_status();
}

int vivit_embedding_weight_mjp_f32(const float *B, const int32_t *ids, float *out, int64_t V, int64_t N, int64_t T, int64_t D,
                                   int64_t W, void *stream) {
  if (!B || !ids || !out) return VIVIT_E_BADARG;
  if (W <= 0) return VIVIT_E_BADARG;
  const int st = emb_sizes_status(V, N, T, D);
  if (st != VIVIT_OK) return st;
  if (W > EMB_LIM || V * N > (((int64_t)1 << 60) / W) / D) return VIVIT_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(out, 0, (size_t)(V * N * W * D) * 4, s) != hipSuccess) return VIVIT_E_LAUNCH;
  const int64_t total = V * N * T * D;
  emb_weight_mjp_kernel<<<(unsigned)cdiv(total, 256), 256, 0, s>>>(B, ids, out, total, (int)N, (int)T, (int)D, (int)W);
  return launch_status();
}

} // extern "C"
