// Internal interfaces between the eigensolver translation units (host-side launch wrappers only:
// kernels are launched from the file that defines them).
#pragma once
#include "common.h"

namespace vivit {

// One workspace, handed out front to back.  Built from (base, bytes) it returns regions; built without memory it only
// measures, so the function that lays a workspace out is also the one that sizes it.  Regions start on `align` bytes,
// the first at `base` rounded up.  A region that would end past base + bytes sets overflow(): its pointer is still
// returned, so every entry point checks the flag after laying out and before its first HIP call.
class Arena {
 public:
  explicit Arena(size_t align = 256) : align_(align) {}
  Arena(void *base, size_t bytes, size_t align = 256)
      : align_(align), real_(true), begin_(align_up(reinterpret_cast<uintptr_t>(base), align)), at_(begin_),
        end_(reinterpret_cast<uintptr_t>(base) + bytes) {
    overflow_ = at_ > end_;
  }
  template <class T> T *take(size_t count) {
    const uintptr_t r = at_;
    if (real_ && r + sizeof(T) * count > end_) overflow_ = true;   // (the region itself: the padding behind the last one is not used)
    at_ += align_up(sizeof(T) * count, align_);
    return reinterpret_cast<T *>(r);
  }
  // the next `bytes` as an arena of their own: the block of a stage that carries its own alignment and slack
  Arena sub(size_t bytes, size_t align = 256) {
    Arena s = real_ ? Arena(reinterpret_cast<void *>(at_), bytes, align) : Arena(align);
    take<char>(bytes);
    s.overflow_ |= overflow_;
    return s;
  }
  void absorb(const Arena &s) { overflow_ |= s.overflow_; }   // a sub-arena's overflow is this one's too
  size_t used() const { return at_ - begin_; }
  size_t left() const { return end_ > at_ ? end_ - at_ : 0; }
  bool overflow() const { return overflow_; }
  // position, to hand a finished stage's regions to the next one: p = mark() ... rewind(p)
  void *mark() const { return reinterpret_cast<void *>(at_); }
  void rewind(void *m) { at_ = reinterpret_cast<uintptr_t>(m); }

 private:
  size_t align_;
  bool real_ = false, overflow_ = false;
  uintptr_t begin_ = 0, at_ = 0, end_ = 0;
};

struct SytrdWs {
  float *vw;        // [3*PB][n]: V (PB rows) | W (PB rows) | V again  (so [V;W] and [W;V] are both contiguous)
  float *xbuf;      // [n]
  float *rowpart;   // [nct][n]
  float *colpart;   // [nrt][n]
  float *dotpart;   // [nct][2*PB]
  float *cvw;       // [2*PB]   c_v = V^T v | c_w = W^T v
  float *ssqpart;   // [nwg]
  float *wdotpart;  // [nwg]
  float *scal;      // [16]  0: alpha  1: sigma  2: bad-input flag  3: amax
  float *d, *e, *tau;
};

struct SytrdLayout {
  SytrdWs ws;
  float *scanpart;  // [2n] partials of the prescale scan
};

// sytrd.hip: the block is sytrd_workspace_floats(n) floats, laid out on an arena of 16-byte regions
SytrdLayout sytrd_layout(Arena &a, int64_t n);
size_t sytrd_workspace_floats(int64_t n);
int sytrd_launch(float *A, int64_t n, int64_t lda, const SytrdLayout &L, hipStream_t stream);
// the same for `batch` <= PERSIST_MAX_BATCH matrices of one size with the persistent reduction (sytrd_persist_ok(n), n <= 1280):
// prescale per problem, then one batched persistent launch (A, L: host arrays of `batch`)
int sytrd_batched_launch(float *const *A, int batch, int64_t n, int64_t lda, const SytrdLayout *L, hipStream_t stream);

// sytrd_persist.hip: the same reduction as one persistent launch on the 32 CUs of one XCD (n <= 1280; after prescale_launch)
bool sytrd_persist_ok(int64_t n);
int sytrd_persist_launch(float *A, int64_t n, int64_t lda, const SytrdWs &ws, hipStream_t stream);
// up to PERSIST_MAX_BATCH problems of one size n <= 1280 in ONE launch, problem q on XCD q (A, ws: host arrays of `batch`)
constexpr int PERSIST_MAX_BATCH = 8;
int sytrd_persist_batched_launch(float *const *A, int batch, int64_t n, int64_t lda, const SytrdWs *ws, hipStream_t stream);

struct DcWs {
  float *dcur, *dnew;   // [n] eigenvalues of the current / next level (physical row order)
  float *z;             // [n] rank-one vector
  float *ds, *zs;       // [n] sorted copies (modified by the deflation scan)
  float *dk, *zk;       // [n] compacted non-deflated poles / weights
  float *rot;           // [n][4]  (tp, tq) as ints in [0],[1]; c, s in [2],[3]
  float *rho, *tol;     // [nmerge]
  float *tnorm;         // [1] norm of the whole tridiagonal matrix (written by the leaves)
  int *order;           // [n] sorted position -> local physical row
  int *ndpos, *dfpos;   // [n] sorted positions of the non-deflated / deflated poles, in output order
  int *kcount, *nrot;   // [nmerge]
  int *org;             // [n] origin pole of each secular root
  double *mu, *zhat;    // [n]
  float **rowptr;       // [n] destination row of each sorted position (after gather)
  GemmDesc *desc;       // [nmerge]
  float *Qt0, *Qt1;     // [n][n] eigenvectors (rows), block diagonal per node, ping-pong
  float *G;             // [n][n] gathered non-deflated rows
  float *U;             // [n * smax] secular eigenvectors, U_q[j * s + i]
};

// stedc.hip
DcWs dc_layout(Arena &a, int64_t n);
size_t stedc_workspace_bytes(int64_t n, bool vectors);
int stedc_dc_launch(const float *d, const float *e, int64_t n, DcWs ws, float **Qt_out, float **d_out,
                    int **order_scratch, int32_t *info, hipStream_t stream);
// w[m] = m-th smallest eigenvalue of (d, e) by bisection, divided by scal[1] when scal != nullptr
// (w64, optional: the same eigenvalues in fp64, NOT divided by the scale)
int stebz_launch(const float *d, const float *e, int64_t n, float *w, const float *scal, hipStream_t stream,
                 double *w64 = nullptr);
// the same for `batch` <= PERSIST_MAX_BATCH tridiagonals of one size in one launch (host arrays of `batch`; scal / w64: null or
// arrays without null entries): the kernel of stebz_launch with the problem as a grid dimension
int stebz_batched_launch(int batch, int64_t n, const float *const *d, const float *const *e, float *const *w,
                         const float *const *scal, hipStream_t stream, double *const *w64 = nullptr);
// stein.hip: selected eigenvectors of the tridiagonal (d, e) by inverse iteration, rows of Zt
struct SteinWs {
  double *a, *b, *c, *d2, *y;  // [n][Kp]
  unsigned char *piv;          // [n][Kp]
  double *span;                // [2]: Gershgorin span, norm bound
};
SteinWs stein_layout(Arena &a, int64_t n, int64_t K);
size_t stein_workspace_bytes(int64_t n, int64_t K);
int stein_launch(const float *d, const float *e, int64_t n, const double *lam64, const int *sel, int64_t K, float *Zt,
                 int64_t ldz, const SteinWs &ws, int32_t *info, hipStream_t stream);
// the same for `batch` <= PERSIST_MAX_BATCH tridiagonals of one size n: three launches for all (problem, eigenvalue) pairs.
// Host arrays of `batch`; K[q] may differ, K[q] = 0 is legal (its other entries are not read); ws[q]: stein_layout(., n, K[q])
int stein_batched_launch(int batch, int64_t n, const float *const *d, const float *const *e, const double *const *lam64,
                         const int *const *sel, const int64_t *K, float *const *Zt, int64_t ldz, const SteinWs *ws,
                         int32_t *const *info, hipStream_t stream);
// two-phase eigensolver for criterion-selected eigenvectors (symeig_large.hip)
size_t symeig_reduce_workspace_bytes(int64_t n);
size_t symeig_select_workspace_bytes(int64_t n, int64_t K);
int symeig_reduce_launch(float *A, int64_t n, int64_t lda, float *w, void *ws, size_t ws_bytes, int32_t *info,
                         hipStream_t stream);
int symeig_select_launch(const float *A, int64_t n, int64_t lda, const int *sel, int64_t K, float *Zt, int64_t ldz,
                         void *state, size_t state_bytes, void *ws, size_t ws_bytes, int32_t *info, hipStream_t stream);
// w = sorted(dcur) / sigma;  Z[i][p] = Qt[order[p]][i];  info = n if the input was non-finite
int symeig_large_rows_launch(float *A, int64_t n, int64_t lda, float *w, float *Zt, int64_t ldz, int64_t r0, int64_t r1,
                             void *ws, size_t ws_bytes, int32_t *info, hipStream_t stream);
int dc_rows_launch(int64_t n, const float *dcur, const float *Qt, int64_t ldq, int *order, float *w, float *Zs,
                   int64_t ldz, int64_t r0, int64_t r1, const float *scal, hipStream_t stream);
int info_scal_launch(int32_t *info, int64_t n, const float *scal, hipStream_t stream);
// rows Zs[s] = eigenvector at ascending position sel[s] (device int32 [K]) of a finished divide & conquer
int dc_select_launch(int64_t n, const float *dcur, const float *Qt, int64_t ldq, int *order, float *wscratch,
                     const int *sel, int64_t K, float *Zs, int64_t ldz, hipStream_t stream);
int dc_output_launch(int64_t n, const float *dcur, const float *Qt, int64_t ldq, int *order, float *w, float *Z,
                     int64_t ldz, const float *scal, int32_t *info, hipStream_t stream);

// sy2sb.hip / sb2st.hip (two-stage tridiagonalisation)
struct QrPart {
  float *u;     // [2][nwg][SNB]
  float *diag;  // [2][SNB]
};

struct Sy2sbWs {
  float *pan;      // [n][SNB]   compact copy of the current panel block
  float *stackA;   // [2*SGRP*SNB][n]  V1 | W1 | V2 | W2 ...  (k-major, ld = n)
  float *stackB;   // [2*SGRP*SNB][n]  W1 | V1 | W2 | V2 ...
  float *xt;       // [SNB][n]    scratch (X^T)
  float *G12;      // [SNB][2*SNB*(SGRP-1)]
  float *S, *T, *Y3, *S2;  // [SNB*SNB] each
  float *tau1;     // [n]
  float *betas;    // [SNB] diagonal of R of the current panel
  QrPart qp;       // partials of the fused panel QR
  void *qpw;       // exchange buffers of the persistent panel QR
  void *gws;       // split-K workspace
  size_t gws_bytes;
};
Sy2sbWs sy2sb_layout(Arena &a, int64_t n);
size_t sy2sb_workspace_bytes(int64_t n);
// (the reflector scalars are left in ws.tau1)
int sy2sb_launch(float *A, int64_t n, int64_t lda, const Sy2sbWs &ws, hipStream_t stream);
// Row stride of the band array INSIDE the library: the 2 NB + 1 = 129 entries of a band row + 3 floats of padding, so that the
// bulge chase can write a row's [E | D] segment with 16-byte stores (what such a store writes beyond the diagonal entry lands in
// the padding).  The public entry points (vivit_sy2sb_f32, vivit_sb2st_f32) keep rows of 129.
constexpr int SB2ST_LDP = 132;
int sy2sb_extract_band_launch(const float *A, int64_t lda, int64_t n, float *AB, int64_t ldab, hipStream_t stream);
size_t sy2sb_panel_qr_workspace_bytes(int64_t mp);
int sy2sb_panel_qr_launch(float *pan, int64_t mp, float *Vt, int64_t ldv, float *tau, float *betas, float *T, void *wsbase,
                          size_t ws_bytes, hipStream_t stream);
// symeig_large.hip: the two-stage solver entered AFTER the band reduction (A holds band + first-stage reflectors, as
// sy2sb_launch leaves it; tau1, scal: device) -- rows r0 .. r1-1 of the eigenvector matrix
int symeig_banded_rows_launch(float *A, int64_t n, int64_t lda, const float *tau1, const float *scal_in, float *w, float *Zt,
                              int64_t ldz, int64_t r0, int64_t r1, void *ws, size_t ws_bytes, int32_t *info, hipStream_t stream);
int symeig_prepare_launch(float *A, int64_t n, int64_t lda, float *scal, void *ws, size_t ws_bytes, hipStream_t stream);
int sb2st_num_levels(int64_t n);
int64_t sb2st_ring_rows(int64_t n);
int sb2st_launch(float *AB, int64_t n, float *d, float *e, float *R2, int64_t ldr, int64_t r2rows, float *tau2,
                 hipStream_t stream);
// sytrd.hip: scan (amax, non-finite flag) + LAPACK-style scaling of the lower triangle; scal: [16], part: [2n]
int prescale_launch(float *A, int64_t n, int64_t lda, float *scal, float *part, hipStream_t stream);
// elementwise.hip
int symmetrize_launch(float *G, int64_t n, int64_t ldg, hipStream_t stream);

// q2apply.hip: Zt[nrows x n] <- Zt * Q2^T (Q2 = bulge-chasing reflectors of sb2st_launch, R2 with r2rows = n)
size_t q2_workspace_bytes(int64_t n, int64_t max_rows);   // max_rows: most rows one call will transform (< 0: unknown)
int q2_apply_launch(float *Zt, int64_t ldz, int64_t nrows, int64_t n, const float *R2, int64_t ldr, const float *tau2,
                    void *ws, hipStream_t stream, int mode = -1);
// q2slide.hip: the same transformation with a sliding window per row slab on the bf16 matrix pipe (many rows)
size_t q2_slide_workspace_bytes(int64_t n);
bool q2_slide_possible(int64_t nrows, int64_t n);   // by shape and environment only (workspace queries)
bool q2_slide_ok(int64_t nrows, int64_t n, const float *Zt, int64_t ldz);
int q2_slide_launch(float *Zt, int64_t ldz, int64_t nrows, int64_t n, const float *R2, int64_t ldr, const float *tau2, void *ws,
                    size_t ws_bytes, hipStream_t stream);

// info = n when the scan flagged non-finite input (scal[2] != 0)
int info_finalize_launch(int32_t *info, int64_t n, const float *scal, hipStream_t stream);
// the same for info[0 .. batch-1] (batch <= PERSIST_MAX_BATCH, scal: host array): the sticky failure word is one per
// stream, so a set bit fails EVERY problem of the batch
int info_finalize_batched_launch(int32_t *info, int batch, int64_t n, const float *const *scal, hipStream_t stream);
// symeig_large.hip: the two-phase solver for `batch` matrices of one size 193 <= n <= 1280 (vivit_symeig_*_batched_f32)
size_t symeig_select_batched_workspace_bytes(int64_t n, int64_t batch, int64_t kmax);
int symeig_reduce_batched_launch(float *const *A, int64_t batch, int64_t n, int64_t lda, float *W, void *const *state,
                                 size_t state_bytes_each, int32_t *info, hipStream_t stream);
int symeig_select_batched_launch(const float *const *A, int64_t batch, int64_t n, int64_t lda, const int *idx, const int64_t *K,
                                 float *const *Zt, int64_t ldz, void *const *state, size_t state_bytes_each, void *ws,
                                 size_t ws_bytes, int32_t *info, hipStream_t stream);
// symeig_large.hip: eigenvalues of `batch` matrices of one size 193 <= n <= 1280, in waves of PERSIST_MAX_BATCH
size_t symeigvals_batched_workspace_bytes(int64_t n, int64_t batch);
int symeigvals_batched_launch(float *const *A, int64_t batch, int64_t n, int64_t lda, float *W, void *ws, size_t ws_bytes,
                              int32_t *info, hipStream_t stream);

} // namespace vivit
