// Multi-kernel symmetric eigensolver for n > SMALL_N_MAX:
//   sytrd.hip  blocked Householder tridiagonalisation          (HBM-bound symv + MFMA rank-2k)
//   stedc.hip  tridiagonal eigenproblem                         (bisection | divide & conquer)
//   here       Householder back-transformation  Z = Q_H Q_T     (compact-WY blocks, MFMA GEMMs)
//
// Eigenvectors are carried transposed (row = eigenvector) until the very end: the D&C produces
// Qt = Q_T^T, the back-transformation applies the block reflectors from the right,
//   Zt <- Zt (I - Y T Y^T)^T = Zt - ((Zt Y) T^T) Y^T,
// three GEMMs per block of KB reflectors whose rows Y^T are exactly the rows sytrd left in the
// upper triangle of A, and a final permuted transpose delivers Tensor.symeig's column layout.
#include <cstdlib>

#include "common.h"
#include "device_utils.h"
#include "eig_internal.h"

namespace vivit {

constexpr int KB = 128;  // reflectors per compact-WY block

// Yt[t][i] = v_{a+t}[i] (zero for i <= a+t and for reflector indices beyond n-3)
// (one-stage: shift = 1, jmax = n-3; two-stage stage-1 reflectors: shift = NB, jmax = n-NB-1)
__global__ __launch_bounds__(256) void bt_extract_kernel(const float *__restrict__ A, int64_t lda, int n, int a,
                                                         float *__restrict__ Yt, int shift, int jmax) {
  const int t = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = a + t;
  float v = 0.f;
  if (j <= jmax && i >= j + shift) v = A[(int64_t)j * lda + i];
  Yt[(int64_t)t * n + i] = v;
}

// T (upper triangular, forward/columnwise larft) of ONE block of KB reflectors from its Gram block
// S (ld lds) and tau, written into the diagonal block of the super-block factor (ld ldt): one thread per
// column (device_utils.h:tfactor_column), S and T staged in LDS (2 x 66 KB, dynamic)
constexpr int BT_LD = KB + 1;
constexpr int BT_TF_LDS = (2 * KB * BT_LD + KB) * 4;
__global__ __launch_bounds__(KB) void bt_tfactor_kernel(const float *__restrict__ S, int64_t lds_, const float *__restrict__ tau,
                                                        int jmax, int a, float *__restrict__ T, int64_t ldt) {
  extern __shared__ float tf_lds[];
  float *Ss = tf_lds, *Ts = Ss + KB * BT_LD, *taus = Ts + KB * BT_LD;
  const int r = threadIdx.x;
  // workgroup b factors diagonal block b of the super-block: reflectors a + b KB .., S and T blocks at (b KB, b KB)
  a += blockIdx.x * KB;
  S += (int64_t)blockIdx.x * KB * (lds_ + 1);
  T += (int64_t)blockIdx.x * KB * (ldt + 1);
  for (int idx = r; idx < KB * KB; idx += KB) Ss[(idx / KB) * BT_LD + (idx % KB)] = S[(int64_t)(idx / KB) * lds_ + (idx % KB)];
  taus[r] = (a + r <= jmax) ? tau[a + r] : 0.f;
  __syncthreads();
  tfactor_column(Ss, taus, Ts, BT_LD, KB, r);
  __syncthreads();
  for (int idx = r; idx < KB * KB; idx += KB) T[(int64_t)(idx / KB) * ldt + (idx % KB)] = Ts[(idx / KB) * BT_LD + (idx % KB)];
}

// Blocks of KB reflectors are merged into super-blocks of `nsub` blocks (a power of two, up to 8: 1024
// reflectors) so that the three products of the back-transformation have a long contraction / wide
// output (the 256 x 256 tile kernel; Zt is streamed once per 1024 instead of once per 128 reflectors):
//   H_1 H_2 = I - [Y1 Y2] [[T1, -T1 (Y1^T Y2) T2], [0, T2]] [Y1 Y2]^T        (applied recursively).
// The merge tree T12 = -T1 (Y1^T Y2) T2 as TWO batched products per level (all pairs of a level are independent) instead of
// two launches per pair: at 2048 reflectors 8 launches instead of 30 per super-block (Q1 at n = 40 960: 600 launches of 24 us).
// The descriptors only depend on the buffers, so one tiny kernel writes them once per back-transformation:
// per level (halves of size h, nb = KS / 2h pairs):  desc[at + q] : X_q = T1 S12,   desc[at + nb + q] : T12 = -X_q T2,   at += 2 nb.
constexpr int BT_MAX_DESC = 2 * 32;   // 2 (nsub - 1) descriptors, nsub <= 32
__global__ void bt_merge_desc_kernel(const float *S, float *T, float *X, int64_t KS, int64_t kb, GemmDesc *desc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int at = 0;
  for (int64_t h = kb; h < KS; h *= 2) {
    const int nb = (int)(KS / (2 * h));
    for (int64_t o = 0, q = 0; o < KS; o += 2 * h, ++q) {
      float *Xq = X + q * h * h;
      GemmDesc d1, d2;
      d1.A = T + o * (KS + 1); d1.B = S + o * KS + (o + h); d1.C = Xq;
      d1.M = h; d1.N = h; d1.K = h; d1.lda = KS; d1.ldb = KS; d1.ldc = h;
      d2.A = Xq; d2.B = T + (o + h) * (KS + 1); d2.C = T + o * KS + (o + h);
      d2.M = h; d2.N = h; d2.K = h; d2.lda = h; d2.ldb = KS; d2.ldc = KS;
      desc[at + q] = d1; desc[at + nb + q] = d2;
    }
    at += 2 * nb;
  }
}

static int bt_nsub(int64_t n) {   // largest super-block (workspace sizing)
  return n >= 16384 ? 16 : (n >= 8192 ? 8 : (n >= 4096 ? 4 : (n >= 2048 ? 2 : 1)));
}
// Super-block actually used for `nrows` rows of Zt: the read-modify-write of Zt per super-block favours 2048
// reflectors when (nearly) all rows are transformed (Q1 at n = 40 960: 1037 / 816 / 767 / 757 ms for 512 / 1024 /
// 2048 / 4096), while the T factor work (2 KS n^2 flop, independent of nrows) favours 1024 for a few selected rows.
static int bt_nsub_rows(int64_t n, int64_t nrows) {
  const int nmax = bt_nsub(n);
  return (nmax > 8 && nrows < 4096) ? 8 : nmax;
}

// split-K slab of the products for ANY nrows <= n (row-range mode): a one-tile-wide output gets up to
// 2048 / tiles splits, so splits * nrows <= 2048 * 128 and the slab is bounded by 2048 * 128 * KS floats
static size_t bt_gemm_ws_bytes(int64_t n) {
  const int64_t KS = (int64_t)KB * bt_nsub(n);
  size_t b = gemm_workspace_bytes(n, KS, n, false);
  const size_t b2 = gemm_workspace_bytes(KS, KS, n, false), b3 = gemm_workspace_bytes(KS, KS, n, true);
  const size_t bound = (size_t)2048 * 128 * KS * sizeof(float);
  if (b2 > b) b = b2;
  if (b3 > b) b = b3;
  return b > bound ? b : bound;
}

struct BtWs {
  float *Yt, *W1, *W2;   // [KS][n], [n][KS] x 2
  float *S, *T, *X;      // [KS][KS]
  GemmDesc *mdesc;       // merge-tree descriptors
  void *gws;
  size_t gws_bytes;
};

// (sized for the largest super-block, bt_nsub(n), whatever bt_nsub_rows picks for a call)
static BtWs bt_layout(Arena &a, int64_t n) {
  const int64_t KS = (int64_t)KB * bt_nsub(n);
  BtWs ws;
  ws.Yt = a.take<float>(KS * n);
  ws.W1 = a.take<float>(n * KS);
  ws.W2 = a.take<float>(n * KS);
  ws.S = a.take<float>(KS * KS);
  ws.T = a.take<float>(KS * KS);
  ws.X = a.take<float>(KS * KS);
  ws.mdesc = a.take<GemmDesc>(BT_MAX_DESC);
  ws.gws_bytes = bt_gemm_ws_bytes(n);
  ws.gws = a.take<char>(ws.gws_bytes);
  return ws;
}

static size_t bt_workspace_bytes(int64_t n) {
  Arena m;
  bt_layout(m, n);
  return m.used() + 512;
}

// Zt[nrows x n] (ld ldq) <- Zt * Q^T for Q = H_0 H_1 ... (reflector j in row j of A, support i >= j + shift,
// j <= jmax), compact-WY super-blocks, last one first.  Every row is transformed independently (nrows = n for
// the full eigenvector matrix, a slice of the rows when the back-transformation is sharded over GPUs).
static int backtransform_launch(const float *A, int64_t n, int64_t lda, const float *tau, int shift, int64_t jmax,
                                float *Qt, int64_t ldq, int64_t nrows, const BtWs &ws, hipStream_t stream) {
  const int ni = (int)n;
  const int nsub = bt_nsub_rows(n, nrows);
  const int64_t KS = (int64_t)KB * nsub;
  float *const Yt = ws.Yt, *const W1 = ws.W1, *const W2 = ws.W2, *const S = ws.S, *const T = ws.T, *const X = ws.X;
  GemmDesc *const mdesc = ws.mdesc;
  void *const gws = ws.gws;
  const size_t gws_bytes = ws.gws_bytes;
  if (jmax < 0 || nrows <= 0) return VIVIT_OK;
  static unsigned long long tf_done = 0;
  {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return VIVIT_E_LAUNCH;
    if (!(tf_done & (1ull << (dev & 63)))) {
      if (!ensure_dynamic_lds(reinterpret_cast<const void *>(bt_tfactor_kernel), BT_TF_LDS, tf_done)) return VIVIT_E_LAUNCH;
      tf_done |= 1ull << (dev & 63);
    }
  }
  int st;
  if (nsub > 1) {
    if (2 * (nsub - 1) > BT_MAX_DESC) return VIVIT_E_UNSUPPORTED;
    bt_merge_desc_kernel<<<1, 64, 0, stream>>>(S, T, X, KS, (int64_t)KB, mdesc);
  }
  for (int64_t a = (jmax / KS) * KS; a >= 0; a -= KS) {
    // reflector rows of the super-block (zero rows for indices beyond jmax), their Gram matrix, block T factors
    bt_extract_kernel<<<dim3((unsigned)cdiv(n, 256), (unsigned)KS), 256, 0, stream>>>(A, lda, ni, (int)a, Yt, shift, (int)jmax);
    st = gemm_launch(LAY_K, LAY_K, Yt, Yt, S, KS, KS, n, n, n, KS, 1.f, 0.f, true, gws, gws_bytes, stream);  // SYRK: lower tiles + mirror
    if (st != VIVIT_OK) return st;
    if (nsub > 1 && hipMemsetAsync(T, 0, sizeof(float) * KS * KS, stream) != hipSuccess) return VIVIT_E_LAUNCH;
    // block T factors of the nsub diagonal blocks: one workgroup each, one launch
    bt_tfactor_kernel<<<nsub, KB, BT_TF_LDS, stream>>>(S, KS, tau, (int)jmax, (int)a, T, KS);
    // merge tree: T12 = -T1 S12 T2 for halves of size h = KB, 2 KB, ...: the pairs of a level as one batched launch per product
    {
      int at = 0;
      for (int64_t h = KB; h < KS; h *= 2) {
        const int batch = (int)(KS / (2 * h));
        st = gemm_batched_launch(LAY_K, LAY_M, mdesc + at, batch, h, h, 1.f, 0.f, stream);
        if (st != VIVIT_OK) return st;
        st = gemm_batched_launch(LAY_K, LAY_M, mdesc + at + batch, batch, h, h, -1.f, 0.f, stream);
        if (st != VIVIT_OK) return st;
        at += 2 * batch;
      }
    }
    const int64_t m = n - a;  // components a+shift .. n-1 carry the super-block's reflectors (the columns before
                              // are zero in Yt: starting at the aligned offset a keeps the operands 16-byte aligned)
    // W1[nrows x KS] = Zt[:, a:] * Yt[:, a:]^T
    st = gemm_launch(LAY_K, LAY_K, Qt + a, Yt + a, W1, nrows, KS, m, ldq, n, KS, 1.f, 0.f, false, gws, gws_bytes, stream);
    if (st != VIVIT_OK) return st;
    // W2 = W1 * T^T
    st = gemm_launch(LAY_K, LAY_K, W1, T, W2, nrows, KS, KS, KS, KS, KS, 1.f, 0.f, false, gws, gws_bytes, stream);
    if (st != VIVIT_OK) return st;
    // Zt[:, a:] -= W2 * Yt[:, a:]
    st = gemm_launch(LAY_K, LAY_M, W2, Yt + a, Qt + a, nrows, m, KS, KS, n, ldq, -1.f, 1.f, false, gws, gws_bytes, stream);
    if (st != VIVIT_OK) return st;
  }
  return VIVIT_OK;
}

// ---- two-stage reduction (sy2sb + sb2st) --------------------------------------------------------
constexpr int TS_NB = 64;

// 1 = use the two-stage tridiagonalisation, with or without eigenvectors: where the persistent one-stage reduction
// applies (sytrd_persist_ok, n <= 2048) it wins (n = 2048: 24.9 / 31.1 ms against 37 / ~47 for the two stages), above
// it the two stages do (one-stage chain / two-stage, ms, eigvalsh | symeig: n = 2304: 61 / 43 | 65 / 52, 4096: 129 / 79
// | 136 / 96 -- scripts/probe/crossover2.py; earlier crossovers: profiles/HISTORY.md).  VIVIT_TWO_STAGE=0/1 overrides.
static bool use_two_stage(int64_t n) {
  static int forced = -2;
  if (forced == -2) {
    const char *e = getenv("VIVIT_TWO_STAGE");
    forced = e ? atoi(e) : -1;
  }
  if (forced >= 0) return forced != 0 && n > 2 * TS_NB;
  if (sytrd_persist_ok(n)) return false;
  return n >= 2048;
}

// What the users of the two-stage front half differ in.
struct TsMode {
  bool band_here;   // prescale, mirror and band reduction run here (false: the caller did them and gives tau1 and scal)
  bool keep_q2;     // R2 of n rows and tau2 cleared, for the Q2 back-transformation (false: the ring of a values-only solve)
  bool own_tau1;    // tau1 copied out of the band reduction's block (the reduce phase keeps it in its state)
};
constexpr TsMode TS_VALUES = {true, false, false}, TS_VECTORS = {true, true, false}, TS_STATE = {true, true, true},
                 TS_BANDED = {false, true, false};

struct TwoStageWs {
  TsMode mode;
  float *scal, *part;   // scaling record [16], scan partials [2n]
  Sy2sbWs sb;
  float *AB, *R2, *tau2, *tau1, *d, *e;
  int64_t r2rows;
};

static TwoStageWs two_stage_layout(Arena &a, int64_t n, TsMode m) {
  TwoStageWs L = {};
  L.mode = m;
  L.scal = a.take<float>(16);
  if (m.band_here) {
    L.part = a.take<float>(2 * n);
    Arena s = a.sub(sy2sb_workspace_bytes(n));
    L.sb = sy2sb_layout(s, n);
    a.absorb(s);
    L.tau1 = L.sb.tau1;
  }
  L.AB = a.take<float>(n * SB2ST_LDP);
  L.r2rows = m.keep_q2 ? n : sb2st_ring_rows(n);
  L.R2 = a.take<float>(L.r2rows * n);
  L.tau2 = a.take<float>(n * sb2st_num_levels(n));
  if (m.own_tau1) L.tau1 = a.take<float>(n);
  L.d = a.take<float>(n);
  L.e = a.take<float>(n);
  return L;
}

// [prescale -> mirror -> band] -> band extract -> tridiagonal (d, e; the Q2 reflectors in R2, tau2 when they are kept)
static int two_stage_reduce(float *A, int64_t n, int64_t lda, const TwoStageWs &L, hipStream_t stream) {
  prof_mark(PROF_STAGE_BEGIN, stream);
  int st;
  if (L.mode.band_here) {
    st = prescale_launch(A, n, lda, L.scal, L.part, stream);
    if (st != VIVIT_OK) return st;
    st = symmetrize_launch(A, n, lda, stream);
    if (st != VIVIT_OK) return st;
    prof_mark(PROF_STAGE_PREP, stream);
    st = sy2sb_launch(A, n, lda, L.sb, stream);
    if (st != VIVIT_OK) return st;
    if (L.mode.own_tau1 && hipMemcpyAsync(L.tau1, L.sb.tau1, sizeof(float) * n, hipMemcpyDeviceToDevice, stream) != hipSuccess)
      return VIVIT_E_LAUNCH;
  }
  st = sy2sb_extract_band_launch(A, lda, n, L.AB, SB2ST_LDP, stream);
  if (st != VIVIT_OK) return st;
  prof_mark(PROF_STAGE_SY2SB, stream);
  if (L.mode.keep_q2 && hipMemsetAsync(L.tau2, 0, sizeof(float) * n * sb2st_num_levels(n), stream) != hipSuccess)
    return VIVIT_E_LAUNCH;
  st = sb2st_launch(L.AB, n, L.d, L.e, L.R2, n, L.r2rows, L.tau2, stream);
  if (st != VIVIT_OK) return st;
  prof_mark(PROF_STAGE_SB2ST, stream);
  return VIVIT_OK;
}

// ---- one-stage reduction: the sytrd block on 16-byte regions inside the 256-byte ones of its caller
static SytrdLayout one_stage_layout(Arena &a, int64_t n) {
  Arena s = a.sub(sizeof(float) * sytrd_workspace_floats(n), 16);
  const SytrdLayout L = sytrd_layout(s, n);
  a.absorb(s);
  return L;
}

static int one_stage_reduce(float *A, int64_t n, int64_t lda, const SytrdLayout &L, hipStream_t stream) {
  prof_mark(PROF_STAGE_BEGIN, stream);
  const int st = sytrd_launch(A, n, lda, L, stream);
  if (st != VIVIT_OK) return st;
  prof_mark(PROF_STAGE_SYTRD, stream);
  return VIVIT_OK;
}

static size_t one_stage_workspace_bytes(int64_t n) {
  Arena m;
  one_stage_layout(m, n);
  return m.used() + 512;
}

static size_t two_stage_workspace_bytes(int64_t n, bool vectors) {
  Arena m;
  two_stage_layout(m, n, vectors ? TS_VECTORS : TS_VALUES);
  return m.used() + 1024;
}

// What either reduction leaves for the rest of a solve: the tridiagonal, the scaling record and the reflectors
// (those of sytrd / sy2sb are in A, scalars tau1; R2 != nullptr: two-stage, the bulge-chasing reflectors).
struct Reduced {
  const float *d, *e, *scal, *tau1, *R2, *tau2;
};
static Reduced reduced_of(const TwoStageWs &L) { return {L.d, L.e, L.scal, L.tau1, L.R2, L.tau2}; }
static Reduced reduced_of(const SytrdLayout &L) { return {L.ws.d, L.ws.e, L.ws.scal, L.ws.tau, nullptr, nullptr}; }

// Zt[nrows x n] <- Zt Q2^T (two-stage only) Q1^T
static int back_transform_rows(const float *A, int64_t n, int64_t lda, const Reduced &R, float *Zt, int64_t ldz, int64_t nrows,
                               void *q2ws, const BtWs &bt, hipStream_t stream) {
  int st;
  if (R.R2) {
    st = q2_apply_launch(Zt, ldz, nrows, n, R.R2, n, R.tau2, q2ws, stream);
    if (st != VIVIT_OK) return st;
    prof_mark(PROF_STAGE_Q2, stream);
    st = backtransform_launch(A, n, lda, R.tau1, TS_NB, n - TS_NB - 1, Zt, ldz, nrows, bt, stream);
  } else {
    st = backtransform_launch(A, n, lda, R.tau1, 1, n - 3, Zt, ldz, nrows, bt, stream);
  }
  if (st != VIVIT_OK) return st;
  prof_mark(PROF_STAGE_Q1, stream);
  return VIVIT_OK;
}

// ---- the back half of a solve with eigenvectors: divide & conquer, then the back-transformations
struct BackWs {
  DcWs dc;
  void *q2ws;
  BtWs bt;
};

static BackWs back_layout(Arena &a, int64_t n, bool two_stage) {
  BackWs B;
  Arena s = a.sub(stedc_workspace_bytes(n, true));
  B.dc = dc_layout(s, n);
  a.absorb(s);
  B.q2ws = two_stage ? a.take<char>(q2_workspace_bytes(n, n)) : nullptr;
  B.bt = bt_layout(a, n);
  return B;
}

// T = Q_T diag(w) Q_T^T by divide and conquer (Qt = Q_T^T, rows unsorted), then Zt = Qt Q2^T Q1^T on the rows of Qt.
// r1 < 0: all of them, Z = column eigenvectors.  Rows mode (r1 >= 0): Z receives the eigenvectors r0 .. r1-1 (ascending
// eigenvalue order) as ROWS, [r1-r0][ldz], and only those rows are back-transformed (rows of Zt are independent: this is
// what the multi-GPU path shards).
static int eigvec_back_half(const float *A, int64_t n, int64_t lda, const Reduced &R, const BackWs &B, float *w, float *Z,
                            int64_t ldz, int64_t r0, int64_t r1, int32_t *info, hipStream_t stream) {
  float *Qt, *dd;
  int *order;
  int st = stedc_dc_launch(R.d, R.e, n, B.dc, &Qt, &dd, &order, info, stream);
  if (st != VIVIT_OK) return st;
  if (r1 >= 0) {
    st = dc_rows_launch(n, dd, Qt, n, order, w, Z, ldz, r0, r1, R.scal, stream);
    if (st != VIVIT_OK) return st;
    prof_mark(PROF_STAGE_TRIDIAG, stream);
    st = back_transform_rows(A, n, lda, R, Z, ldz, r1 - r0, B.q2ws, B.bt, stream);
    if (st != VIVIT_OK) return st;
    return info_scal_launch(info, n, R.scal, stream);
  }
  prof_mark(PROF_STAGE_TRIDIAG, stream);
  st = back_transform_rows(A, n, lda, R, Qt, n, n, B.q2ws, B.bt, stream);
  if (st != VIVIT_OK) return st;
  // sort ascending, undo the scaling, deliver column eigenvectors
  st = dc_output_launch(n, dd, Qt, n, order, w, Z, ldz, R.scal, info, stream);
  prof_mark(PROF_STAGE_OUTPUT, stream);
  return st;
}

// values only: bisection, undo the scaling (lam64, optional: the eigenvalues in fp64)
static int values_launch(const Reduced &R, int64_t n, float *w, double *lam64, int32_t *info, hipStream_t stream) {
  int st = stebz_launch(R.d, R.e, n, w, R.scal, stream, lam64);
  if (st != VIVIT_OK) return st;
  st = info_finalize_launch(info, n, R.scal, stream);
  prof_mark(PROF_STAGE_TRIDIAG, stream);
  return st;
}

size_t symeig_large_workspace_bytes(int64_t n, bool vectors) {
  const size_t one = one_stage_workspace_bytes(n), two = two_stage_workspace_bytes(n, vectors);
  size_t b = one > two ? one : two;   // either reduction may be selected at run time
  b += stedc_workspace_bytes(n, vectors);
  if (vectors) b += bt_workspace_bytes(n) + q2_workspace_bytes(n, n) + 512;
  return b;
}

// Z == nullptr: eigenvalues only; otherwise eigenvectors as for eigvec_back_half.
static int symeig_large_impl(float *A, int64_t n, int64_t lda, float *w, float *Z, int64_t ldz, int64_t r0, int64_t r1,
                             void *ws, size_t ws_bytes, int32_t *info, hipStream_t stream) {
  const bool vectors = Z != nullptr;
  if (n > 0x7fffffffLL / 8) return VIVIT_E_UNSUPPORTED;
  if (!ws || ws_bytes < symeig_large_workspace_bytes(n, vectors)) return VIVIT_E_WORKSPACE;
  const bool two_stage = use_two_stage(n);
  Arena a(ws, ws_bytes);
  TwoStageWs ts = {};
  SytrdLayout trd = {};
  if (two_stage) ts = two_stage_layout(a, n, vectors ? TS_VECTORS : TS_VALUES);
  else trd = one_stage_layout(a, n);
  BackWs back = {};
  if (vectors) back = back_layout(a, n, two_stage);
  if (a.overflow()) return VIVIT_E_WORKSPACE;
  if (hipMemsetAsync(info, 0, sizeof(int32_t), stream) != hipSuccess) return VIVIT_E_LAUNCH;

  // A = Q1 B Q1^T (band), B = Q2 T Q2^T  |  A = Q_H T Q_H^T
  const int st = two_stage ? two_stage_reduce(A, n, lda, ts, stream) : one_stage_reduce(A, n, lda, trd, stream);
  if (st != VIVIT_OK) return st;
  const Reduced R = two_stage ? reduced_of(ts) : reduced_of(trd);
  if (!vectors) return values_launch(R, n, w, nullptr, info, stream);
  return eigvec_back_half(A, n, lda, R, back, w, Z, ldz, r0, r1, info, stream);
}

// ---- two-phase solver: reduction + all eigenvalues, host-side criterion, then only the selected eigenvectors --------
// Phase 1 (symeig_reduce_launch) leaves in the workspace everything phase 2 needs: the tridiagonal (d, e), the
// eigenvalues in fp64, the reflector scalars (the reflectors themselves are in A and, two-stage, in R2).
// Phase 2 (symeig_select_launch): K <= SELECT_STEIN_MAX eigenvectors by inverse iteration on T (stein.hip),
// otherwise divide & conquer + gather; then the back-transformations on those K rows only (4 K n^2 flop).
constexpr int64_t SELECT_STEIN_MAX = 256;

struct SelectLayout {
  bool two_stage;
  TwoStageWs ts;     // two-stage
  SytrdLayout trd;   // one-stage
  Reduced R;
  double *lam64;
};

static SelectLayout select_layout(Arena &a, int64_t n) {
  SelectLayout L = {};
  L.two_stage = use_two_stage(n);
  if (L.two_stage) {
    L.ts = two_stage_layout(a, n, TS_STATE);
    L.R = reduced_of(L.ts);
  } else {
    L.trd = one_stage_layout(a, n);
    L.R = reduced_of(L.trd);
  }
  L.lam64 = a.take<double>(n);
  return L;
}

// state workspace (phase 1 writes it, phase 2 reads it)
size_t symeig_reduce_workspace_bytes(int64_t n) {
  Arena m;
  select_layout(m, n);
  return m.used() + 1024;
}

// scratch workspace of phase 2 for K selected eigenvectors
size_t symeig_select_workspace_bytes(int64_t n, int64_t K) {
  if (K < 1) K = 1;
  if (K > n) K = n;
  size_t b = use_two_stage(n) ? q2_workspace_bytes(n, K) + 512 : 0;
  const size_t after = bt_workspace_bytes(n);
  if (K > SELECT_STEIN_MAX) {  // D&C buffers, reused by the back-transformations afterwards
    const size_t dc = align_up(stedc_workspace_bytes(n, true), 256);
    b += align_up(sizeof(float) * n, 256) + (dc > after ? dc : after);
  } else {
    b += align_up(stein_workspace_bytes(n, K), 256) + after;
  }
  return b + 1024;
}

int symeig_reduce_launch(float *A, int64_t n, int64_t lda, float *w, void *ws, size_t ws_bytes, int32_t *info,
                         hipStream_t stream) {
  if (n > 0x7fffffffLL / 8) return VIVIT_E_UNSUPPORTED;
  if (!ws || ws_bytes < symeig_reduce_workspace_bytes(n)) return VIVIT_E_WORKSPACE;
  Arena a(ws, ws_bytes);
  const SelectLayout L = select_layout(a, n);
  if (a.overflow()) return VIVIT_E_WORKSPACE;
  if (hipMemsetAsync(info, 0, sizeof(int32_t), stream) != hipSuccess) return VIVIT_E_LAUNCH;
  const int st = L.two_stage ? two_stage_reduce(A, n, lda, L.ts, stream) : one_stage_reduce(A, n, lda, L.trd, stream);
  if (st != VIVIT_OK) return st;
  return values_launch(L.R, n, w, L.lam64, info, stream);
}

int symeig_select_launch(const float *A, int64_t n, int64_t lda, const int *sel, int64_t K, float *Zt, int64_t ldz,
                         void *state, size_t state_bytes, void *ws, size_t ws_bytes, int32_t *info, hipStream_t stream) {
  if (K < 0 || K > n || (K > 0 && (!sel || !Zt || ldz < n))) return VIVIT_E_BADARG;
  if (!state || state_bytes < symeig_reduce_workspace_bytes(n)) return VIVIT_E_WORKSPACE;
  if (K == 0) return VIVIT_OK;
  if (!ws || ws_bytes < symeig_select_workspace_bytes(n, K)) return VIVIT_E_WORKSPACE;
  Arena sa(state, state_bytes), a(ws, ws_bytes);
  const SelectLayout L = select_layout(sa, n);
  const bool dc_route = K > SELECT_STEIN_MAX;   // many eigenvectors: divide & conquer for all of them, keep the selected rows
  SteinWs stw = {};
  DcWs dc = {};
  float *wscratch = nullptr;
  if (dc_route) {
    wscratch = a.take<float>(n);
    void *dc_base = a.mark();
    Arena s = a.sub(stedc_workspace_bytes(n, true));
    dc = dc_layout(s, n);
    a.absorb(s);
    a.rewind(dc_base);   // once the selected rows are in Zt the D&C block is free for the back-transformations
  } else {
    Arena s = a.sub(stein_workspace_bytes(n, K));
    stw = stein_layout(s, n, K);
    a.absorb(s);
  }
  void *q2ws = L.two_stage ? a.take<char>(q2_workspace_bytes(n, K)) : nullptr;
  const BtWs bt = bt_layout(a, n);
  if (sa.overflow() || a.overflow()) return VIVIT_E_WORKSPACE;
  // (not eigvec_back_half: the selection is a gather by index without eigenvalues, scaling or status, and the
  // back-transformations run on the D&C block's memory instead of behind it)
  prof_mark(PROF_STAGE_BEGIN, stream);
  int st;
  if (dc_route) {
    float *Qt, *dd;
    int *order;
    st = stedc_dc_launch(L.R.d, L.R.e, n, dc, &Qt, &dd, &order, info, stream);
    if (st != VIVIT_OK) return st;
    st = dc_select_launch(n, dd, Qt, n, order, wscratch, sel, K, Zt, ldz, stream);
  } else {
    st = stein_launch(L.R.d, L.R.e, n, L.lam64, sel, K, Zt, ldz, stw, info, stream);
  }
  if (st != VIVIT_OK) return st;
  prof_mark(PROF_STAGE_TRIDIAG, stream);
  return back_transform_rows(A, n, lda, L.R, Zt, ldz, K, q2ws, bt, stream);
}

int symeig_large_launch(float *A, int64_t n, int64_t lda, float *w, float *Z, int64_t ldz, void *ws, size_t ws_bytes,
                        int32_t *info, hipStream_t stream) {
  return symeig_large_impl(A, n, lda, w, Z, ldz, 0, -1, ws, ws_bytes, info, stream);
}

// ---- eigenvalues of `batch` matrices of one size 193 <= n <= 1280 (vivit_symeigvals_batched_f32) -------------------------
// One slot of symeig_large_workspace_bytes(n, false) per problem of a wave; the waves of PERSIST_MAX_BATCH follow each other
// on the stream and reuse the slots, so the size stops growing at eight.
static size_t batched_slot_bytes(int64_t n) { return align_up(symeig_large_workspace_bytes(n, false), 256); }

size_t symeigvals_batched_workspace_bytes(int64_t n, int64_t batch) {
  const int64_t slots = batch < PERSIST_MAX_BATCH ? batch : PERSIST_MAX_BATCH;
  return batched_slot_bytes(n) * (size_t)slots + 256;
}

// A wave of both batched reductions: prescale per problem -> ONE persistent launch, problem q on XCD q -> one bisection
// launch -> one status kernel.  Every per-problem kernel is the one the single solve launches, on the same kind of
// workspace: the eigenvalues are those of vivit_symeig_f32, bit for bit.  slot_of(i, q): where problem i, the q-th of its
// wave, has its sytrd block, and its fp64 eigenvalues if they are kept (all problems or none).
struct WaveSlot {
  SytrdLayout trd;
  double *lam64;
};

template <class SlotOf>
static int reduce_waves(float *const *A, int64_t batch, int64_t n, int64_t lda, float *W, SlotOf slot_of, int32_t *info,
                        hipStream_t stream) {
  if (hipMemsetAsync(info, 0, sizeof(int32_t) * batch, stream) != hipSuccess) return VIVIT_E_LAUNCH;
  for (int64_t i0 = 0; i0 < batch; i0 += PERSIST_MAX_BATCH) {
    const int nb = (int)(batch - i0 < PERSIST_MAX_BATCH ? batch - i0 : PERSIST_MAX_BATCH);
    SytrdLayout trd[PERSIST_MAX_BATCH];
    const float *dq[PERSIST_MAX_BATCH], *eq[PERSIST_MAX_BATCH], *scal[PERSIST_MAX_BATCH];
    float *wq[PERSIST_MAX_BATCH];
    double *lam[PERSIST_MAX_BATCH];
    for (int q = 0; q < nb; ++q) {
      const WaveSlot s = slot_of(i0 + q, q);
      trd[q] = s.trd;
      dq[q] = s.trd.ws.d; eq[q] = s.trd.ws.e; scal[q] = s.trd.ws.scal; lam[q] = s.lam64;
      wq[q] = W + (i0 + q) * n;
    }
    int st = sytrd_batched_launch(A + i0, nb, n, lda, trd, stream);
    if (st != VIVIT_OK) return st;
    st = stebz_batched_launch(nb, n, dq, eq, wq, scal, stream, lam[0] ? lam : nullptr);   // one bisection launch for the wave
    if (st != VIVIT_OK) return st;
    st = info_finalize_batched_launch(info + i0, nb, n, scal, stream);
    if (st != VIVIT_OK) return st;
  }
  return VIVIT_OK;
}

// Without the persistent kernels (or with the two-stage reduction forced) the problems run one after the other through
// the single solve itself.
int symeigvals_batched_launch(float *const *A, int64_t batch, int64_t n, int64_t lda, float *W, void *ws, size_t ws_bytes,
                              int32_t *info, hipStream_t stream) {
  if (!ws || ws_bytes < symeigvals_batched_workspace_bytes(n, batch)) return VIVIT_E_WORKSPACE;
  Arena a(ws, ws_bytes);
  const size_t slot = batched_slot_bytes(n);
  WaveSlot slots[PERSIST_MAX_BATCH] = {};
  void *base = a.mark();
  for (int q = 0; q < PERSIST_MAX_BATCH && q < batch; ++q) {
    Arena s = a.sub(slot);
    slots[q].trd = one_stage_layout(s, n);
    a.absorb(s);
  }
  if (a.overflow()) return VIVIT_E_WORKSPACE;
  if (use_two_stage(n) || !sytrd_persist_ok(n)) {
    for (int64_t i = 0; i < batch; ++i) {
      const int st = symeig_large_impl(A[i], n, lda, W + i * n, nullptr, 0, 0, -1, base, slot, info + i, stream);
      if (st != VIVIT_OK) return st;
    }
    return VIVIT_OK;
  }
  return reduce_waves(A, batch, n, lda, W, [&](int64_t, int q) { return slots[q]; }, info, stream);
}

// ---- eigenpairs of `batch` matrices of one size 193 <= n <= 1280 in two phases (vivit_symeig_reduce_batched_f32 /
// vivit_symeig_select_batched_f32): the batched reduction above with every problem's workspace inside ITS state block,
// laid out by select_layout, so that state[b] + A[b] is what symeig_reduce_launch would have left (the single select accepts
// it); then inverse iteration and the back-transformation of the few selected rows for the whole wave at once.

// Zt_q[K_q x n] <- Zt_q Q_q^T = Zt_q H_{n-3} ... H_1 H_0 (H_j = I - tau_j v_j v_j^T, v_j = A_q[j][j+1:]) for all problems of a
// wave in ONE launch.  The rows are independent: one wavefront keeps one row of Zt in registers (lane l: components l + 64 t)
// and applies the reflectors one after the other, last first -- a dot product (wave butterfly, fixed order) and an axpy each.
// The four waves of a workgroup share the reflector rows, staged BT_JB at a time in LDS.  Workgroup b serves problem b % 8:
// with the round-robin placement of workgroups that is one XCD per problem, whose L2 then holds that problem's reflectors
// for all of its rows.  No cross-problem data, no atomics; 2 K n^2 flop per problem where the compact-WY chain of
// backtransform_launch pays 2 KB n^2 for the T factors alone (K ~ 10, KB = 128) in six launches per block.
constexpr int BT_JB = 8;         // reflectors staged per round
constexpr int BT_ROWS_WG = 4;    // rows of Zt (waves) per workgroup
struct BtRowsProblem {
  const float *A, *tau;
  float *Zt;
  int K;
};
struct BtRowsBatch {
  BtRowsProblem p[PERSIST_MAX_BATCH];
};

template <int NT>   // n <= 64 NT
__global__ __launch_bounds__(64 * BT_ROWS_WG) void bt_rows_batched_kernel(int n, int64_t lda, int64_t ldz, BtRowsBatch bb) {
  __shared__ float sv[BT_JB][64 * NT];
  __shared__ float stau[BT_JB];
  const BtRowsProblem &p = bb.p[blockIdx.x % PERSIST_MAX_BATCH];
  const int row0 = (int)(blockIdx.x / PERSIST_MAX_BATCH) * BT_ROWS_WG;
  if (row0 >= p.K) return;   // (the whole workgroup: no barrier is missed)
  const int tid = threadIdx.x, lane = tid & 63, row = row0 + (tid >> 6);
  const bool active = row < p.K;
  const float *__restrict__ A = p.A;
  float z[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int i = lane + 64 * t;
    z[t] = (active && i < n) ? p.Zt[(int64_t)row * ldz + i] : 0.f;
  }
  const int jmax = n - 3;
  for (int jb = (jmax / BT_JB) * BT_JB; jb >= 0; jb -= BT_JB) {
    __syncthreads();   // the previous round's readers are done
    for (int idx = tid; idx < BT_JB * 64 * NT; idx += 64 * BT_ROWS_WG) {
      const int jj = idx / (64 * NT), i = idx % (64 * NT), j = jb + jj;
      sv[jj][i] = (j <= jmax && i > j && i < n) ? A[(int64_t)j * lda + i] : 0.f;
    }
    if (tid < BT_JB) stau[tid] = (jb + tid <= jmax) ? p.tau[jb + tid] : 0.f;
    __syncthreads();
    const int t0 = (jb + 1) / 64;   // tiles below hold no component of these reflectors
    for (int jj = BT_JB - 1; jj >= 0; --jj) {
      float dot = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t >= t0) dot += z[t] * sv[jj][lane + 64 * t];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
      const float s = stau[jj] * dot;
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t >= t0) z[t] -= s * sv[jj][lane + 64 * t];
    }
  }
  if (active) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int i = lane + 64 * t;
      if (i < n) p.Zt[(int64_t)row * ldz + i] = z[t];
    }
  }
}

// A, tau, Zt, K: host arrays of `batch` <= PERSIST_MAX_BATCH (K[q] = 0: problem not touched); one launch
static int bt_rows_batched_launch(int batch, int64_t n, int64_t lda, const float *const *A, const float *const *tau,
                                  float *const *Zt, int64_t ldz, const int64_t *K, hipStream_t stream) {
  if (batch < 1 || batch > PERSIST_MAX_BATCH || n > 64 * 20 || n < 3) return VIVIT_E_UNSUPPORTED;
  BtRowsBatch bb = {};
  int64_t kmax = 0;
  for (int q = 0; q < batch; ++q) {
    if (K[q] <= 0) continue;
    bb.p[q].A = A[q]; bb.p[q].tau = tau[q]; bb.p[q].Zt = Zt[q]; bb.p[q].K = (int)K[q];
    if (K[q] > kmax) kmax = K[q];
  }
  if (kmax == 0) return VIVIT_OK;
  const dim3 grid((unsigned)(PERSIST_MAX_BATCH * cdiv(kmax, BT_ROWS_WG)));
  const int ni = (int)n;
  const int nt = (int)cdiv(n, 256) * 4;   // instantiated widths: 256, 512, 768, 1024, 1280 columns
  switch (nt) {
    case 4: bt_rows_batched_kernel<4><<<grid, 64 * BT_ROWS_WG, 0, stream>>>(ni, lda, ldz, bb); break;
    case 8: bt_rows_batched_kernel<8><<<grid, 64 * BT_ROWS_WG, 0, stream>>>(ni, lda, ldz, bb); break;
    case 12: bt_rows_batched_kernel<12><<<grid, 64 * BT_ROWS_WG, 0, stream>>>(ni, lda, ldz, bb); break;
    case 16: bt_rows_batched_kernel<16><<<grid, 64 * BT_ROWS_WG, 0, stream>>>(ni, lda, ldz, bb); break;
    case 20: bt_rows_batched_kernel<20><<<grid, 64 * BT_ROWS_WG, 0, stream>>>(ni, lda, ldz, bb); break;
    default: return VIVIT_E_UNSUPPORTED;
  }
  return launch_status();
}

// the batched reduction needs the persistent kernel (one XCD per problem), the batched select only the one-stage state
// layout; otherwise the entries loop over the single ones
static bool batched_select_ok(int64_t n) { return !use_two_stage(n) && n <= 64 * 20; }
static bool batched_pairs_ok(int64_t n) { return batched_select_ok(n) && sytrd_persist_ok(n); }

// every state block holds its layout (the blocks may sit differently against a 256-byte boundary)
static bool states_fit(void *const *state, int64_t batch, size_t state_bytes_each, int64_t n) {
  for (int64_t i = 0; i < batch; ++i) {
    Arena s(state[i], state_bytes_each);
    select_layout(s, n);
    if (s.overflow()) return false;
  }
  return true;
}

int symeig_reduce_batched_launch(float *const *A, int64_t batch, int64_t n, int64_t lda, float *W, void *const *state,
                                 size_t state_bytes_each, int32_t *info, hipStream_t stream) {
  if (state_bytes_each < symeig_reduce_workspace_bytes(n)) return VIVIT_E_WORKSPACE;
  if (!batched_pairs_ok(n)) {
    for (int64_t i = 0; i < batch; ++i) {
      const int st = symeig_reduce_launch(A[i], n, lda, W + i * n, state[i], state_bytes_each, info + i, stream);
      if (st != VIVIT_OK) return st;
    }
    return VIVIT_OK;
  }
  if (!states_fit(state, batch, state_bytes_each, n)) return VIVIT_E_WORKSPACE;
  auto slot_of = [&](int64_t i, int) {
    Arena s(state[i], state_bytes_each);
    const SelectLayout L = select_layout(s, n);
    return WaveSlot{L.trd, L.lam64};
  };
  return reduce_waves(A, batch, n, lda, W, slot_of, info, stream);
}

// One slot of inverse-iteration scratch per problem of a wave (sized for the largest selection the batched kernels take);
// a selection above SELECT_STEIN_MAX goes through the single select, whose scratch follows the slots.
static int64_t batched_stein_k(int64_t kmax) { return kmax < 1 ? 1 : (kmax > SELECT_STEIN_MAX ? SELECT_STEIN_MAX : kmax); }

size_t symeig_select_batched_workspace_bytes(int64_t n, int64_t batch, int64_t kmax) {
  if (kmax > n) kmax = n;
  const int64_t slots = batch < PERSIST_MAX_BATCH ? batch : PERSIST_MAX_BATCH;
  size_t b = align_up(stein_workspace_bytes(n, batched_stein_k(kmax)), 256) * (size_t)slots;
  if (kmax > SELECT_STEIN_MAX || !batched_select_ok(n)) b += align_up(symeig_select_workspace_bytes(n, kmax), 256);
  return b + 256;
}

int symeig_select_batched_launch(const float *const *A, int64_t batch, int64_t n, int64_t lda, const int *idx, const int64_t *K,
                                 float *const *Zt, int64_t ldz, void *const *state, size_t state_bytes_each, void *ws,
                                 size_t ws_bytes, int32_t *info, hipStream_t stream) {
  int64_t kmax = 0, ktot = 0;
  for (int64_t i = 0; i < batch; ++i) kmax = K[i] > kmax ? K[i] : kmax;
  if (state_bytes_each < symeig_reduce_workspace_bytes(n)) return VIVIT_E_WORKSPACE;
  if (kmax > 0 && (!ws || ws_bytes < symeig_select_batched_workspace_bytes(n, batch, kmax))) return VIVIT_E_WORKSPACE;
  Arena slots[PERSIST_MAX_BATCH];
  void *single_ws = nullptr;
  size_t single_bytes = 0;
  if (kmax > 0) {
    Arena a(ws, ws_bytes);
    const size_t slot = align_up(stein_workspace_bytes(n, batched_stein_k(kmax)), 256);
    for (int q = 0; q < PERSIST_MAX_BATCH && q < batch; ++q) {
      slots[q] = a.sub(slot);
      Arena s = slots[q];
      stein_layout(s, n, batched_stein_k(kmax));   // (the largest layout a slot is asked for)
      a.absorb(s);
    }
    single_ws = a.mark();
    single_bytes = a.left();
    if (a.overflow() || !states_fit(state, batch, state_bytes_each, n)) return VIVIT_E_WORKSPACE;
  }
  if (hipMemsetAsync(info, 0, sizeof(int32_t) * batch, stream) != hipSuccess) return VIVIT_E_LAUNCH;
  if (kmax == 0) return VIVIT_OK;
  const bool batched = batched_select_ok(n);
  for (int64_t i0 = 0; i0 < batch; i0 += PERSIST_MAX_BATCH) {
    const int nb = (int)(batch - i0 < PERSIST_MAX_BATCH ? batch - i0 : PERSIST_MAX_BATCH);
    const float *dq[PERSIST_MAX_BATCH], *eq[PERSIST_MAX_BATCH], *tauq[PERSIST_MAX_BATCH];
    const double *lam[PERSIST_MAX_BATCH];
    const int *sel[PERSIST_MAX_BATCH];
    int64_t Kq[PERSIST_MAX_BATCH];
    SteinWs stws[PERSIST_MAX_BATCH];
    int32_t *infq[PERSIST_MAX_BATCH];
    for (int q = 0; q < nb; ++q) {
      const int64_t i = i0 + q;
      Arena sa(state[i], state_bytes_each), s = slots[q];
      const SelectLayout L = select_layout(sa, n);
      dq[q] = L.R.d; eq[q] = L.R.e; tauq[q] = L.R.tau1; lam[q] = L.lam64;
      sel[q] = idx + ktot;
      ktot += K[i];
      stws[q] = stein_layout(s, n, K[i]);
      infq[q] = info + i;
      Kq[q] = K[i];
      if (K[i] > 0 && (!batched || K[i] > SELECT_STEIN_MAX)) {   // out of the wave: the single select (divide & conquer route)
        const int st = symeig_select_launch(A[i], n, lda, sel[q], K[i], Zt[i], ldz, state[i], state_bytes_each, single_ws,
                                            single_bytes, info + i, stream);
        if (st != VIVIT_OK) return st;
        Kq[q] = 0;
      }
    }
    int st = stein_batched_launch(nb, n, dq, eq, lam, sel, Kq, Zt + i0, ldz, stws, infq, stream);
    if (st != VIVIT_OK) return st;
    st = bt_rows_batched_launch(nb, n, lda, A + i0, tauq, Zt + i0, ldz, Kq, stream);
    if (st != VIVIT_OK) return st;
  }
  return VIVIT_OK;
}

int symeig_large_rows_launch(float *A, int64_t n, int64_t lda, float *w, float *Zt, int64_t ldz, int64_t r0, int64_t r1,
                             void *ws, size_t ws_bytes, int32_t *info, hipStream_t stream) {
  if (!Zt || r0 < 0 || r1 < r0 || r1 > n) return VIVIT_E_BADARG;
  return symeig_large_impl(A, n, lda, w, Zt, ldz, r0, r1, ws, ws_bytes, info, stream);
}

// ---- the two-stage solver in two halves, for a band reduction done elsewhere (multi-GPU: vivit_amd/distributed.py).
// prepare: LAPACK-style scaling + mirror (what two_stage_reduce does in front of sy2sb_launch); scal: device [16].
int symeig_prepare_launch(float *A, int64_t n, int64_t lda, float *scal, void *ws, size_t ws_bytes, hipStream_t stream) {
  if (ws_bytes < sizeof(float) * 2 * (size_t)n + 256) return VIVIT_E_WORKSPACE;
  Arena a(ws, ws_bytes);
  float *part = a.take<float>(2 * n);
  if (a.overflow()) return VIVIT_E_WORKSPACE;
  int st = prescale_launch(A, n, lda, scal, part, stream);
  if (st != VIVIT_OK) return st;
  return symmetrize_launch(A, n, lda, stream);
}

int symeig_banded_rows_launch(float *A, int64_t n, int64_t lda, const float *tau1, const float *scal_in, float *w, float *Zt,
                              int64_t ldz, int64_t r0, int64_t r1, void *ws, size_t ws_bytes, int32_t *info, hipStream_t stream) {
  if (!Zt || r0 < 0 || r1 < r0 || r1 > n || n <= 2 * TS_NB) return VIVIT_E_BADARG;
  if (!ws || ws_bytes < symeig_large_workspace_bytes(n, true)) return VIVIT_E_WORKSPACE;
  Arena a(ws, ws_bytes);
  TwoStageWs ts = two_stage_layout(a, n, TS_BANDED);
  ts.tau1 = const_cast<float *>(tau1);
  const BackWs back = back_layout(a, n, true);
  if (a.overflow()) return VIVIT_E_WORKSPACE;
  if (hipMemsetAsync(info, 0, sizeof(int32_t), stream) != hipSuccess) return VIVIT_E_LAUNCH;
  if (hipMemcpyAsync(ts.scal, scal_in, sizeof(float) * 16, hipMemcpyDeviceToDevice, stream) != hipSuccess) return VIVIT_E_LAUNCH;
  const int st = two_stage_reduce(A, n, lda, ts, stream);
  if (st != VIVIT_OK) return st;
  return eigvec_back_half(A, n, lda, reduced_of(ts), back, w, Zt, ldz, r0, r1, info, stream);
}

} // namespace vivit

using namespace vivit;

extern "C" {

// The two halves of the two-stage solver around an externally computed band reduction (see vivit_hip.h).
int vivit_symeig_prepare_f32(float *A, int64_t n, int64_t lda, float *scal, void *workspace, size_t workspace_bytes, void *stream) {
  if (n < 1 || !A || !scal || lda < n || !workspace) return VIVIT_E_BADARG;
  return symeig_prepare_launch(A, n, lda, scal, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int vivit_symeig_banded_rows_f32(float *A, int64_t n, int64_t lda, const float *tau1, const float *scal, float *w, float *Zt,
                                 int64_t ldz, int64_t row_begin, int64_t row_end, void *workspace, size_t workspace_bytes,
                                 int32_t *info, void *stream) {
  if (n < 1 || !A || !tau1 || !scal || !w || !info || lda < n || ldz < n) return VIVIT_E_BADARG;
  return symeig_banded_rows_launch(A, n, lda, tau1, scal, w, Zt, ldz, row_begin, row_end, workspace, workspace_bytes, info,
                                   static_cast<hipStream_t>(stream));
}

size_t vivit_sytrd_f32_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return one_stage_workspace_bytes(n);
}

int vivit_sytrd_f32(float *A, int64_t n, int64_t lda, float *d, float *e, float *tau, void *workspace,
                    size_t workspace_bytes, void *stream) {
  if (n < 3 || !A || !d || !e || !tau || lda < n) return VIVIT_E_BADARG;
  if (!workspace || workspace_bytes < vivit_sytrd_f32_workspace_bytes(n)) return VIVIT_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  Arena a(workspace, workspace_bytes);
  const SytrdLayout L = one_stage_layout(a, n);
  if (a.overflow()) return VIVIT_E_WORKSPACE;
  const SytrdWs &tw = L.ws;
  int st = sytrd_launch(A, n, lda, L, s);
  if (st != VIVIT_OK) return st;
  if (hipMemcpyAsync(d, tw.d, sizeof(float) * n, hipMemcpyDeviceToDevice, s) != hipSuccess) return VIVIT_E_LAUNCH;
  if (hipMemcpyAsync(e, tw.e, sizeof(float) * (n - 1), hipMemcpyDeviceToDevice, s) != hipSuccess) return VIVIT_E_LAUNCH;
  if (hipMemcpyAsync(tau, tw.tau, sizeof(float) * n, hipMemcpyDeviceToDevice, s) != hipSuccess) return VIVIT_E_LAUNCH;
  return VIVIT_OK;
}

} // extern "C"
